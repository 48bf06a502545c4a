// ktab_range.h -- the count range of a table operand, "<path>[:<lo>-<hi>]", for the tools that take one (tabop, tabbin, tabcmp):
// one parser, one message.  Plain C++; no device code.
#pragma once
#include <cerrno>
#include "host_io.h"

// splits "<path>[:<lo>-<hi>]": the range into r[0], r[1] when the text after the last ':' matches [0-9]*-[0-9]*
static std::string split_range(const std::string &arg, int64_t *r)
{ r[0] = 1;
  r[1] = INT64_MAX;
  const size_t c = arg.rfind(':');
  if (c == std::string::npos) return arg;
  const std::string t = arg.substr(c+1);
  const size_t dash = t.find('-');
  if (dash == std::string::npos) return arg;
  for (size_t i = 0; i < t.size(); i++)
    if (i != dash && (t[i] < '0' || t[i] > '9')) return arg;
  errno = 0;
  if (dash > 0) r[0] = strtoll(t.c_str(),nullptr,10);                // past 2^63-1 it is 2^63-1
  if (dash+1 < t.size()) r[1] = strtoll(t.c_str()+dash+1,nullptr,10);
  if (r[0] < 1 || r[1] < r[0])
    die("%s: Count range of %s needs 1 <= lo <= hi (%s)\n",PROG,arg.substr(0,c).c_str(),t.c_str());
  return arg.substr(0,c);
}

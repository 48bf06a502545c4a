// class_record.h -- the header of a FASTX read as the reference's tools print it and one record of a .class file, for
// every tool that writes one.
#pragma once
#include "host_io.h"

static const int CLASS_FASTX_RLEN_MAX = 60000;               // prof2class.c:154-160: the bound for FASTX sources

// "@name comment"; kseq keeps the previous comment buffer, and a source without any comment so far prints "(null)"
static std::string fastx_class_header(const FastxReader &fx)
{ return "@"+fx.name+" "+(fx.have_comment ? fx.comment : std::string("(null)")); }

// "@header\nseq\n+\nlabels\n"
static void write_class_record(FILE *out, const std::string &header, const char *seq, size_t rlen, const char *labels,
                               size_t nlabels)
{ fputs(header.c_str(),out); fputc('\n',out);
  fwrite(seq,1,rlen,out);
  fputs("\n+\n",out);
  fwrite(labels,1,nlabels,out);
  fputc('\n',out);
}

// window_check.cpp -- classpro_amd/csrc/host/unitig_window.h on the host, at windows of a few elements: the refill points
// and sizes of a Window, base ranges written across refills, and write_unitig_fasta and write_gfa byte for byte against a
// writer that holds everything, at every small window.  The fetch copies from host arrays of the exact size, so that under
// AddressSanitizer a range outside its array fails.  Built and run by tests/test_unitig_graph_host.py; prints "ok" and
// returns 0, or says what differed and returns 1.
#include <cstring>
#include <string>
#include <utility>
#include "host/unitig_window.h"

typedef std::vector<std::pair<int64_t,int64_t>> Log;

struct HostFetch
  { Log *log;
    template <class T> void operator()(T *dst, const T *src, int64_t first, int64_t count) const
    { if (log) log->push_back({ first, count });
      memcpy(dst,src+first,(size_t)count*sizeof(T));
    }
  };

static int fail(const char *what, const std::string &got, const std::string &want)
{ printf("%s:\n--- got\n%s\n--- want\n%s\n",what,got.c_str(),want.c_str());
  return 1;
}

static std::string slurp(FILE *f)
{ std::string s;
  char buf[256];
  size_t n;
  rewind(f);
  while ((n = fread(buf,1,sizeof(buf),f)) > 0) s.append(buf,n);
  fclose(f);
  return s;
}

static std::string show(const Log &l)
{ std::string s;
  for (const auto &p : l) s += "(" + std::to_string(p.first) + "," + std::to_string(p.second) + ")";
  return s;
}

// unitigs of 1, 3, 4, 5 and 9 bases: at a window of 4 the second ends exactly at a refill, the third starts at one, the
// fourth spans two windows and the fifth three
static const int64_t OFF[6] = { 0, 1, 4, 8, 13, 22 };
static const char *BASES = "ACCGTACGTTGACCATGGTACA";

static int check_windows()
{ const std::vector<char> seq(BASES,BASES+22);              // no terminator: one byte past the end is out of bounds
  for (int64_t cap : { 4, 1, 100 })
    { Log log, want;
      Window<char,HostFetch> w(seq.data(),22,cap,HostFetch{ &log });
      FILE *f = tmpfile();
      if (!f) return fail("tmpfile","","");
      bool ok = true;
      for (int u = 0; u < 5; u++)
        { ok = w.write(f,OFF[u],OFF[u+1]) && ok;
          ok = fputc('\n',f) != EOF && ok;
        }
      const std::string got = slurp(f);
      std::string text;
      for (int u = 0; u < 5; u++) text += std::string(BASES+OFF[u],BASES+OFF[u+1]) + "\n";
      if (!ok || got != text) return fail("bases through a window",got,text);
      for (int64_t p = 0; p < 22; p += cap) want.push_back({ p, std::min(cap,22-p) });
      if (log != want) return fail("refills of the base window",show(log),show(want));
    }
  // at(): a refill starts at the index asked for, not at a multiple of the window
  const std::vector<int64_t> v = { 10, 11, 12, 13, 14, 15, 16 };
  Log log;
  Window<int64_t,HostFetch> w(v.data(),7,3,HostFetch{ &log });
  int64_t sum = 0;
  for (int64_t i : { 1, 2, 3, 5, 6 }) sum += w.at(i);
  const Log want = { { 1, 3 }, { 5, 2 } };
  if (sum != 11+12+13+15+16 || log != want) return fail("at()",show(log),show(want));
  return 0;
}

// 5 unitigs (the bases above), 7 links: orientation 1 has none, orientation 2 has three
static const std::vector<int64_t> KC = { 7, 30, 41, 5, 900 }, COMP = { 0, 0, 2, 0, 4 }, COV = { 3, 0, 1, 0, 12 };
static const std::vector<uint8_t> FLAG = { 0, 1, 0, 0, 1 };
static const std::vector<int64_t> LOFF = { 0, 1, 1, 4, 5, 5, 6, 6, 7, 7, 7 }, LINK = { 2, 0, 7, 9, 3, 6, 1 }, SUP = { 1, 0, 0, 5, 2, 0, 9 };
static const int K = 4;

static std::string gfa_text(int64_t count, bool rc)
{ std::string s = "H\tVN:Z:1.0\n";
  for (int64_t u = 0; u < count; u++)
    { s += "S\t" + std::to_string(u) + "\t" + std::string(BASES+OFF[u],BASES+OFF[u+1]) + "\tLN:i:" + std::to_string(OFF[u+1]-OFF[u])
           + "\tKC:i:" + std::to_string(KC[u]) + "\tco:i:" + std::to_string(COMP[u]);
      if (rc) s += "\tRC:i:" + std::to_string(COV[u]);
      s += "\n";
    }
  for (int64_t x = 0; x < 2*count; x++)
    for (int64_t k = LOFF[x]; k < LOFF[x+1]; k++)
      { s += "L\t" + std::to_string(x >> 1) + "\t" + ((x & 1) ? "-" : "+") + "\t" + std::to_string(LINK[k] >> 1) + "\t"
             + ((LINK[k] & 1) ? "-" : "+") + "\t" + std::to_string(K-1) + "M";
        if (rc) s += "\tRC:i:" + std::to_string(SUP[k]);
        s += "\n";
      }
  return s;
}

static int check_gfa()
{ const std::vector<char> seq(BASES,BASES+22);
  for (bool rc : { false, true })
    { const UnitigArrays a = { seq.data(), KC.data(), FLAG.data(), COMP.data(), LOFF.data(), LINK.data(), rc ? COV.data() : nullptr,
                               rc ? SUP.data() : nullptr };
      const std::string want = gfa_text(5,rc);
      const DumpCaps caps[] = { { 100, 100, 100 }, { 4, 2, 2 }, { 4, 2, 3 }, { 1, 1, 1 }, { 100, 2, 100 }, { 3, 100, 2 } };
      for (const DumpCaps &c : caps)
        { FILE *f = tmpfile();
          if (!f) return fail("tmpfile","","");
          const bool ok = write_gfa(f,K,5,7,OFF,a,HostFetch{ nullptr },c);
          const std::string got = slurp(f);
          if (!ok || got != want) return fail("write_gfa",got,want);
        }
    }
  // no unitig: the H line alone, and no array is touched
  const int64_t off0[1] = { 0 };
  const UnitigArrays none = {};
  FILE *f = tmpfile();
  if (!f) return fail("tmpfile","","");
  const bool ok = write_gfa(f,K,0,0,off0,none,HostFetch{ nullptr },DumpCaps{ 4, 2, 2 });
  const std::string got = slurp(f);
  if (!ok || got != "H\tVN:Z:1.0\n") return fail("write_gfa of no unitig",got,"H\tVN:Z:1.0\n");
  return 0;
}

static int check_fasta()
{ const std::vector<char> seq(BASES,BASES+22);
  const UnitigArrays a = { seq.data(), KC.data(), FLAG.data(), nullptr, nullptr, nullptr, nullptr, nullptr };
  std::string want;
  for (int u = 0; u < 5; u++)
    want += ">" + std::to_string(u) + " LN:i:" + std::to_string(OFF[u+1]-OFF[u]) + " KC:i:" + std::to_string(KC[u])
            + (FLAG[u] ? " CL:Z:circular" : "") + "\n" + std::string(BASES+OFF[u],BASES+OFF[u+1]) + "\n";
  const DumpCaps caps[] = { { 100, 100, 100 }, { 4, 2, 1 }, { 1, 1, 1 }, { 5, 3, 1 } };
  for (const DumpCaps &c : caps)
    { FILE *f = tmpfile();
      if (!f) return fail("tmpfile","","");
      const bool ok = write_unitig_fasta(f,5,OFF,a,HostFetch{ nullptr },c);
      const std::string got = slurp(f);
      if (!ok || got != want) return fail("write_unitig_fasta",got,want);
    }
  return 0;
}

int main()
{ if (check_windows() || check_gfa() || check_fasta()) return 1;
  printf("ok\n");
  return 0;
}

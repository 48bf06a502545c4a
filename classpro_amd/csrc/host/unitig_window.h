// unitig_window.h -- the unitigs of a table and their graph written out as FASTA and GFA through windows of a fixed size
// (tabunitig, tabgraph, tabpath): the arrays lie on the device and may be larger than the host wants to hold, so a range
// of each comes down at a time.  Nothing here knows the device: how a range comes down is the template argument FETCH,
//   fetch(T *dst, const T *src, int64_t first, int64_t count)       dst[0..count) = src[first..first+count)
// for T = char, uint8_t and int64_t, which unitig_dump.h fills with hipMemcpy and tests/window_check.cpp with memcpy at
// windows of a few elements.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

// Elements [have0, have1) of src[0..total) in a buffer of cap elements, for increasing indices: an index at or past have1
// brings the next range down, from that index on.
template <class T, class FETCH>
struct Window
  { const T *src;
    int64_t total, cap, have0 = 0, have1 = 0;
    FETCH fetch;
    std::vector<T> buf;
    Window(const T *src, int64_t total, int64_t cap, FETCH fetch) : src(src), total(total), cap(cap), fetch(fetch), buf((size_t)cap) {}

    const T &at(int64_t i)
    { if (i >= have1)
        { have0 = i;
          have1 = std::min(i+cap,total);
          fetch(buf.data(),src,have0,have1-have0);
        }
      return buf[(size_t)(i-have0)];
    }

    // elements [first, last) to f, in as many pieces as windows they lie in
    bool write(FILE *f, int64_t first, int64_t last)
    { bool ok = true;
      for (int64_t p = first; p < last; )
        { const T *from = &at(p);
          const int64_t e = std::min(have1,last);
          ok = fwrite(from,sizeof(T),(size_t)(e-p),f) == (size_t)(e-p) && ok;
          p = e;
        }
      return ok;
    }
  };

struct DumpCaps { int64_t seq, utg, lnk; };       // bases, per-unitig values and links held on the host at a time

// the arrays of count unitigs and their links; all but off lie where fetch reads.  cov and sup are null or both given.
struct UnitigArrays
  { const char *seq;
    const int64_t *kc;
    const uint8_t *flag;                          // FASTA only
    const int64_t *comp, *loff, *link;            // GFA only
    const int64_t *cov, *sup;                     // GFA, RC:i: tags: the coverage of a unitig and the support of a link
  };

// per unitig ">ordinal LN:i: KC:i:[ CL:Z:circular]" and the sequence on one line; off[0..count] is on the host
template <class FETCH>
bool write_unitig_fasta(FILE *f, int64_t count, const int64_t *off, const UnitigArrays &a, FETCH fetch, DumpCaps caps)
{ Window<char,FETCH> seq(a.seq,off[count],caps.seq,fetch);
  Window<int64_t,FETCH> kc(a.kc,count,caps.utg,fetch);
  Window<uint8_t,FETCH> flag(a.flag,count,caps.utg,fetch);
  bool ok = true;
  for (int64_t u = 0; u < count; u++)
    { const long long kcu = kc.at(u);
      const bool circular = flag.at(u) & 1;
      ok = fprintf(f,">%lld LN:i:%lld KC:i:%lld%s\n",(long long)u,(long long)(off[u+1]-off[u]),kcu,circular ? " CL:Z:circular" : "") > 0 && ok;
      ok = seq.write(f,off[u],off[u+1]) && ok;
      ok = fputc('\n',f) != EOF && ok;
    }
  return ok;
}

// H, then an S line per unitig, then an L line per link in the order of loff[0..2*count]; RC:i: tags with cov and sup
template <class FETCH>
bool write_gfa(FILE *f, int K, int64_t count, int64_t links, const int64_t *off, const UnitigArrays &a, FETCH fetch,
               DumpCaps caps)
{ bool ok = fputs("H\tVN:Z:1.0\n",f) != EOF;
  { Window<char,FETCH> seq(a.seq,off[count],caps.seq,fetch);
    Window<int64_t,FETCH> kc(a.kc,count,caps.utg,fetch), comp(a.comp,count,caps.utg,fetch), cov(a.cov,count,a.cov ? caps.utg : 0,fetch);
    for (int64_t u = 0; u < count; u++)
      { const long long kcu = kc.at(u), cu = comp.at(u), rc = a.cov ? cov.at(u) : 0;
        ok = fprintf(f,"S\t%lld\t",(long long)u) > 0 && ok;
        ok = seq.write(f,off[u],off[u+1]) && ok;
        ok = fprintf(f,"\tLN:i:%lld\tKC:i:%lld\tco:i:%lld",(long long)(off[u+1]-off[u]),kcu,cu) > 0 && ok;
        if (a.cov) ok = fprintf(f,"\tRC:i:%lld",rc) > 0 && ok;
        ok = fputc('\n',f) != EOF && ok;
      }
  }
  std::vector<int64_t> loff((size_t)2*caps.utg+1);
  Window<int64_t,FETCH> link(a.link,links,caps.lnk,fetch), sup(a.sup,links,a.sup ? caps.lnk : 0,fetch);
  for (int64_t u0 = 0; u0 < count; u0 += caps.utg)       // the link offsets of so many unitigs, and the one that ends the last
    { const int64_t nu = std::min(caps.utg,count-u0);
      fetch(loff.data(),a.loff,2*u0,2*nu+1);
      for (int64_t x = 2*u0; x < 2*(u0+nu); x++)
        for (int64_t k = loff[(size_t)(x-2*u0)]; k < loff[(size_t)(x-2*u0)+1] && k < links; k++)
          { const int64_t y = link.at(k);
            ok = fprintf(f,"L\t%lld\t%c\t%lld\t%c\t%dM",(long long)(x >> 1),(x & 1) ? '-' : '+',(long long)(y >> 1),
                         (y & 1) ? '-' : '+',K-1) > 0 && ok;
            if (a.sup) ok = fprintf(f,"\tRC:i:%lld",(long long)sup.at(k)) > 0 && ok;
            ok = fputc('\n',f) != EOF && ok;
          }
    }
  return ok;
}

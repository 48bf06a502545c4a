// kr_sum_check.cpp -- classpro_amd/csrc/kr_sum.h on the host: the summary algebra and the walk that kr_write_kernel runs.
// Random reads with a random state per k-mer position go through the three passes of kmer_runs.hip with small shapes
// (lanes of 1, 2 or 4 positions, blocks of 1, 2 or 4 lanes): lane summaries by kr_push, block summaries by kr_join, the
// block summaries scanned in groups of random size (which also checks that kr_join is associative), then kr_walk_begin,
// kr_walk_step and kr_walk_end per lane with a capacity that may be too small.  The records, the offsets and the total are
// held against a plain loop over each read, and nothing beyond the capacity may be touched.
// Prints "ok <cases>", or the first case that differs.  Usage: _kr_sum_check <cases>
#include "kr_sum.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static const kr_rec UNTOUCHED = { -9, -9, -9, -9, -9 };

static bool same(const kr_rec &a, const kr_rec &b)
{ return a.first == b.first && a.last == b.last && a.n == b.n && a.read == b.read && a.state == b.state; }

static bool same_sum(const kr_sum &a, const kr_sum &b)
{ if (a.flags != b.flags || a.heads != b.heads) return false;
  return !(a.flags & KR_TAIL) || (a.p == b.p && a.n == b.n);
}

struct Case
  { int K, chunk, lanes, nreads;
    unsigned int skip, emit;
    std::vector<int64_t> off;              // seq_off
    std::vector<uint8_t> state;            // one byte per base, as kr_state_kernel leaves them
    std::vector<kr_rec> want;              // by the plain loop
    std::vector<int64_t> want_off;
  };

static Case make_case(std::mt19937 &g)
{ Case c;
  c.K = 1+g()%4;
  c.chunk = 1 << (g()%3);
  c.lanes = 1 << (g()%3);
  c.nreads = 1+g()%8;
  c.off.assign(1,0);
  for (int r = 0; r < c.nreads; r++)       // one read in three is shorter than K or just K long
    c.off.push_back(c.off.back()+(g()%3 ? g()%40 : g()%(c.K+1)));
  c.skip = g()%32;
  c.emit = (g()%32) & ~c.skip;
  if (!c.emit) { c.skip &= ~1u; c.emit = 1; }
  if (g()%3 == 0) { c.skip = 0x19; c.emit = 6; }          // the phase masks
  c.state.assign((size_t)c.off.back(),(uint8_t)KR_NOKMER);
  c.want_off.assign((size_t)c.nreads+1,0);
  int sticky = 0;
  for (int r = 0; r < c.nreads; r++)
    { c.want_off[(size_t)r] = (int64_t)c.want.size();
      int prev = -1;
      kr_rec cur = UNTOUCHED;
      for (int64_t j = c.off[(size_t)r]+c.K-1; j < c.off[(size_t)r+1]; j++)
        { if (g()%3 == 0) sticky = (int)(g()%5);
          const int s = g()%4 ? sticky : (int)(g()%5);
          const int64_t ord = j-c.off[(size_t)r]-(c.K-1);
          c.state[(size_t)j] = (uint8_t)(s | (ord == 0 ? KR_FIRST : 0u));
          if ((c.skip >> s) & 1u) continue;
          if (s != prev)
            { if (prev >= 0 && ((c.emit >> prev) & 1u)) c.want.push_back(cur);
              cur = kr_rec{ ord, ord, 0, r, s };
              prev = s;
            }
          cur.last = ord;
          cur.n++;
        }
      if (prev >= 0 && ((c.emit >> prev) & 1u)) c.want.push_back(cur);
    }
  c.want_off[(size_t)c.nreads] = (int64_t)c.want.size();
  return c;
}

// the summary of the lane that begins at p0
static kr_sum lane_sum(const Case &c, int64_t p0)
{ const int64_t total = c.off.back();
  kr_sum s{ 0, 0, 0, 0, 0 };
  for (int i = 0; i < c.chunk && p0+i < total; i++)
    { const uint8_t b = c.state[(size_t)(p0+i)];
      kr_push(s,(b & KR_FIRST) != 0,b & 7u,p0+i,c.skip,c.emit);
    }
  return s;
}

// the three passes; false when the scan in groups disagrees with the scan one by one
static bool run_case(const Case &c, std::mt19937 &g, int64_t cap, std::vector<kr_rec> &got, std::vector<int64_t> &got_off,
                     int64_t &got_total)
{ const int64_t total = c.off.back(), cells = (int64_t)c.chunk*c.lanes;
  got.assign((size_t)cap,UNTOUCHED);
  got_off.assign((size_t)c.nreads+1,0);
  got_total = 0;
  if (total == 0) return true;
  const int64_t nblk = (total+cells-1)/cells;
  // pass 1: one summary per block
  std::vector<kr_sum> part((size_t)nblk+1);
  for (int64_t b = 0; b < nblk; b++)
    { kr_sum all{ 0, 0, 0, 0, 0 };
      for (int l = 0; l < c.lanes; l++) all = kr_join(all,lane_sum(c,b*cells+(int64_t)l*c.chunk),c.emit);
      part[(size_t)b] = all;
    }
  // pass 2: part[b] = a reset joined with everything before b, in groups of one to three blocks
  kr_sum run{ 0, 0, 0, KR_RESET, 0 };
  for (int64_t b = 0; b < nblk; )
    { const int64_t e = std::min<int64_t>(nblk,b+1+g()%3);
      const std::vector<kr_sum> mine(part.begin()+b,part.begin()+e);
      kr_sum group{ 0, 0, 0, 0, 0 }, acc = run;
      for (size_t i = 0; i < mine.size(); i++)
        { group = kr_join(group,mine[i],c.emit);
          part[(size_t)b+i] = acc;
          acc = kr_join(acc,mine[i],c.emit);
        }
      run = kr_join(run,group,c.emit);
      if (!same_sum(run,acc)) return false;
      b = e;
    }
  part[(size_t)nblk] = run;
  got_total = run.heads;
  // pass 3: the walk of every lane
  for (int64_t b = 0; b < nblk; b++)
    { kr_sum in = part[(size_t)b];
      for (int l = 0; l < c.lanes; l++)
        { const int64_t p0 = b*cells+(int64_t)l*c.chunk;
          const int np = (int)std::min<int64_t>(std::max<int64_t>(total-p0,0),c.chunk);
          if (np > 0)
            { kr_walk x = kr_walk_begin(in,c.off.data(),c.nreads,p0);
              for (int i = 0; i < np; i++)
                kr_walk_step(x,c.state[(size_t)(p0+i)],p0+i,c.skip,c.emit,c.off.data(),c.nreads,c.K,got.data(),cap,got_off.data());
              if (p0+np == total) kr_walk_end(x,c.emit,c.off.data(),c.nreads,c.K,got.data(),cap,got_off.data());
            }
          in = kr_join(in,lane_sum(c,p0),c.emit);
        }
    }
  return true;
}

int main(int argc, char **argv)
{ std::mt19937 g(1);
  const int cases = argc > 1 ? atoi(argv[1]) : 20000;
  int64_t nruns = 0;
  for (int it = 0; it < cases; it++)
    { const Case c = make_case(g);
      const int64_t n = (int64_t)c.want.size();
      const int64_t cap = n ? (int64_t)(g()%(uint64_t)(n+2)) : 0;
      std::vector<kr_rec> got;
      std::vector<int64_t> got_off;
      int64_t got_total;
      bool ok = run_case(c,g,cap,got,got_off,got_total);
      ok = ok && got_total == n && got_off == c.want_off;
      for (int64_t i = 0; ok && i < cap; i++) ok = same(got[(size_t)i],i < n ? c.want[(size_t)i] : UNTOUCHED);
      if (!ok)
        { printf("case %d differs: K %d, lanes of %d, blocks of %d lanes, %lld bases, skip %x, emit %x, %lld runs, got %lld\n",it,
                 c.K,c.chunk,c.lanes,(long long)c.off.back(),c.skip,c.emit,(long long)n,(long long)got_total);
          return 1;
        }
      nruns += n;
    }
  if (nruns < 2*(int64_t)cases) { printf("too few runs: %lld\n",(long long)nruns); return 1; }
  printf("ok %d\n",cases);
  return 0;
}

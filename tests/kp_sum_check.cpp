// kp_sum_check.cpp -- classpro_amd/csrc/kp_sum.h on the host: the words, the summary algebra and the walk that
// kp_write_kernel runs.  Random reads over a handful of made-up unitigs and arcs get a random step per k-mer position
// (continuing the one before more often than not) and go through the three passes of kmer_paths.hip with small shapes
// (lanes of 1, 2 or 4 positions, blocks of 1, 2 or 4 lanes): lane summaries by kp_push, block summaries by kp_join, the
// block summaries scanned in groups of random size (which also checks that kp_join is associative), then kp_walk_begin,
// kp_walk_step and kp_walk_end per lane with a capacity that may be too small.  The records, the offsets, the totals, the
// coverage and the support are held against a plain loop over each read; nothing beyond the capacity may be touched, and
// a capacity that is too small must leave the two sums alone.
// Prints "ok <cases>", or the first case that differs.  Usage: _kp_sum_check <cases>
#include "kp_sum.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static const kp_seg UNTOUCHED = { -9, -9, -9, -9, -9, -9 };

static bool same(const kp_seg &a, const kp_seg &b)
{ return a.first == b.first && a.x == b.x && a.n == b.n && a.q == b.q && a.read == b.read && a.flags == b.flags; }

struct Case
  { int K, chunk, lanes, nreads;
    std::vector<int64_t> off;              // seq_off
    std::vector<char> seq;
    std::vector<int64_t> uoff;             // the unitigs: offsets of their sequences
    std::vector<int64_t> loff;             // the arcs
    std::vector<uint8_t> lbase;
    std::vector<unsigned long long> word;  // one per base, as kp_step_kernel leaves them
    std::vector<kp_seg> want;              // by the plain loop
    std::vector<int64_t> want_off, want_cov, want_sup;
    int64_t joined;
  };

static Case make_case(std::mt19937 &g)
{ Case c;
  c.K = 2+g()%4;
  c.chunk = 1 << (g()%3);
  c.lanes = 1 << (g()%3);
  c.nreads = 1+g()%8;
  c.off.assign(1,0);
  for (int r = 0; r < c.nreads; r++)       // one read in three is shorter than K or just K long
    c.off.push_back(c.off.back()+(g()%3 ? g()%40 : g()%(c.K+1)));
  const int64_t total = c.off.back();
  for (int64_t j = 0; j < total; j++) c.seq.push_back("ACGT"[g()%4]);
  const int nu = 1+g()%4;
  c.uoff.assign(1,0);
  for (int u = 0; u < nu; u++) c.uoff.push_back(c.uoff.back()+(c.K-1)+1+g()%6);
  c.loff.assign(1,0);
  for (int x = 0; x < 2*nu; x++)
    { for (unsigned int b = 0; b < 4; b++)
        if (g()%2) c.lbase.push_back((uint8_t)b);
      c.loff.push_back((int64_t)c.lbase.size());
    }
  c.word.assign((size_t)total,KP_NOKMER);
  c.want_off.assign((size_t)c.nreads+1,0);
  c.want_cov.assign((size_t)nu,0);
  c.want_sup.assign(c.lbase.size(),0);
  c.joined = 0;
  for (int r = 0; r < c.nreads; r++)
    { c.want_off[(size_t)r] = (int64_t)c.want.size();
      int64_t px = -1, pq = -1;                            // the step before: -1 none
      bool open = false;
      for (int64_t j = c.off[(size_t)r]+c.K-1; j < c.off[(size_t)r+1]; j++)
        { const int64_t ord = j-c.off[(size_t)r]-(c.K-1);
          int64_t x = -1, q = -1;
          unsigned long long w;
          const unsigned int pick = g()%10;
          if (pick < 6 && px >= 0 && pq+1 < c.uoff[(size_t)(px >> 1)+1]-c.uoff[(size_t)(px >> 1)]-(c.K-1)) { x = px; q = pq+1; }
          else if (pick == 6) w = KP_OTHER;
          else if (pick == 7) w = KP_ABSENT;
          else
            { x = (int64_t)(g()%(unsigned int)(2*nu));
              q = (int64_t)(g()%(unsigned int)(c.uoff[(size_t)(x >> 1)+1]-c.uoff[(size_t)(x >> 1)]-(c.K-1)));
            }
          if (x >= 0)
            { const int64_t nodes = c.uoff[(size_t)(x >> 1)+1]-c.uoff[(size_t)(x >> 1)]-(c.K-1);
              w = ((unsigned long long)x << 32) | (unsigned long long)((x & 1) ? nodes-1-q : q);
              if (open && x == px && q == pq+1) c.want.back().n++;
              else
                { const bool joined = px >= 0;
                  c.want.push_back(kp_seg{ ord, x, 1, (int32_t)q, r, joined ? 1 : 0 });
                  if (joined)
                    { c.joined++;
                      const unsigned int code = c.seq[(size_t)j] == 'A' ? 0 : c.seq[(size_t)j] == 'C' ? 1 : c.seq[(size_t)j] == 'G' ? 2 : 3;
                      for (int64_t e = c.loff[(size_t)px]; e < c.loff[(size_t)px+1]; e++)
                        if (c.lbase[(size_t)e] == code) c.want_sup[(size_t)e]++;
                    }
                  open = true;
                }
              c.want_cov[(size_t)(x >> 1)]++;
            }
          else open = false;
          c.word[(size_t)j] = w | (ord == 0 ? KP_FIRST : 0ull);
          px = x; pq = q;
        }
    }
  c.want_off[(size_t)c.nreads] = (int64_t)c.want.size();
  return c;
}

// the summary of the lane that begins at p0
static kp_sum lane_sum(const Case &c, int64_t p0)
{ const int64_t total = c.off.back();
  kp_sum s{ 0, 0, 0, 0 };
  if (p0 >= total) return s;                               // a lane past the batch's end, as in kp_lane_sum
  unsigned long long pw = p0 > 0 ? c.word[(size_t)(p0-1)] : KP_NOKMER;
  for (int i = 0; i < c.chunk && p0+i < total; i++)
    { kp_push(s,pw,c.word[(size_t)(p0+i)],p0+i);
      pw = c.word[(size_t)(p0+i)];
    }
  return s;
}

static bool same_sum(const kp_sum &a, const kp_sum &b)
{ return a.heads == b.heads && a.joined == b.joined && (a.heads == 0 || a.last == b.last); }

struct Got
  { std::vector<kp_seg> segs;
    std::vector<int64_t> off, cov, sup;
    int64_t total, joined;
  };

// the three passes; false when the scan in groups disagrees with the scan one by one
static bool run_case(const Case &c, std::mt19937 &g, int64_t cap, Got &o)
{ const int64_t total = c.off.back(), cells = (int64_t)c.chunk*c.lanes;
  o.segs.assign((size_t)cap,UNTOUCHED);
  o.off.assign((size_t)c.nreads+1,0);
  o.cov.assign(c.want_cov.size(),0);
  o.sup.assign(c.want_sup.size()+1,0);
  o.total = o.joined = 0;
  if (total == 0) return true;
  const int64_t nblk = (total+cells-1)/cells;
  std::vector<kp_sum> part((size_t)nblk+1);
  for (int64_t b = 0; b < nblk; b++)
    { kp_sum all{ 0, 0, 0, 0 };
      for (int l = 0; l < c.lanes; l++) all = kp_join(all,lane_sum(c,b*cells+(int64_t)l*c.chunk));
      part[(size_t)b] = all;
    }
  kp_sum run{ 0, 0, 0, 0 };
  for (int64_t b = 0; b < nblk; )
    { const int64_t e = std::min<int64_t>(nblk,b+1+g()%3);
      const std::vector<kp_sum> mine(part.begin()+b,part.begin()+e);
      kp_sum group{ 0, 0, 0, 0 }, acc = run;
      for (size_t i = 0; i < mine.size(); i++)
        { group = kp_join(group,mine[i]);
          part[(size_t)b+i] = acc;
          acc = kp_join(acc,mine[i]);
        }
      run = kp_join(run,group);
      if (!same_sum(run,acc)) return false;
      b = e;
    }
  part[(size_t)nblk] = run;
  o.total = run.heads;
  o.joined = run.joined;
  kp_args a;
  a.seq = c.seq.data(); a.seq_off = c.off.data(); a.nreads = c.nreads; a.K = c.K;
  a.uoff = c.uoff.data(); a.ucount = (int64_t)c.uoff.size()-1;
  a.loff = c.loff.data(); a.lbase = c.lbase.data(); a.gcount = a.ucount; a.links = (int64_t)c.lbase.size();
  a.segs = o.segs.data(); a.capacity = cap; a.seg_off = o.off.data();
  a.cov = o.cov.data(); a.support = o.sup.data();
  if (run.heads > cap) { a.cov = nullptr; a.support = nullptr; }
  for (int64_t b = 0; b < nblk; b++)
    { kp_sum in = part[(size_t)b];
      for (int l = 0; l < c.lanes; l++)
        { const int64_t p0 = b*cells+(int64_t)l*c.chunk;
          const int np = (int)std::min<int64_t>(std::max<int64_t>(total-p0,0),c.chunk);
          if (np > 0)
            { kp_walk x = kp_walk_begin(in,a,p0);
              unsigned long long pw = p0 > 0 ? c.word[(size_t)(p0-1)] : KP_NOKMER;
              for (int i = 0; i < np; i++)
                { kp_walk_step(x,pw,c.word[(size_t)(p0+i)],p0+i,a);
                  pw = c.word[(size_t)(p0+i)];
                }
              if (p0+np == total) kp_walk_end(x,pw,total,a);
            }
          in = kp_join(in,lane_sum(c,p0));
        }
    }
  return true;
}

int main(int argc, char **argv)
{ std::mt19937 g(1);
  const int cases = argc > 1 ? atoi(argv[1]) : 20000;
  int64_t nsegs = 0, njoined = 0, nsup = 0;
  for (int it = 0; it < cases; it++)
    { const Case c = make_case(g);
      const int64_t n = (int64_t)c.want.size();
      const int64_t cap = n ? (g()%2 ? n : (int64_t)(g()%(uint64_t)(n+2))) : 0;
      Got o;
      bool ok = run_case(c,g,cap,o);
      ok = ok && o.total == n && o.joined == c.joined && o.off == c.want_off;
      for (int64_t i = 0; ok && i < cap; i++) ok = same(o.segs[(size_t)i],i < n ? c.want[(size_t)i] : UNTOUCHED);
      const bool fits = n <= cap;
      for (size_t u = 0; ok && u < c.want_cov.size(); u++) ok = o.cov[u] == (fits ? c.want_cov[u] : 0);
      for (size_t e = 0; ok && e < c.want_sup.size(); e++) ok = o.sup[e] == (fits ? c.want_sup[e] : 0);
      ok = ok && o.sup.back() == 0;
      if (!ok)
        { printf("case %d differs: K %d, lanes of %d, blocks of %d lanes, %lld bases, %lld segments, got %lld, capacity %lld\n",it,
                 c.K,c.chunk,c.lanes,(long long)c.off.back(),(long long)n,(long long)o.total,(long long)cap);
          return 1;
        }
      nsegs += n;
      njoined += c.joined;
      for (const int64_t v : c.want_sup) nsup += v;
    }
  if (nsegs < 2*(int64_t)cases || njoined < cases || nsup < cases/2)
    { printf("too little: %lld segments, %lld joined, %lld supported\n",(long long)nsegs,(long long)njoined,(long long)nsup); return 1; }
  printf("ok %d\n",cases);
  return 0;
}

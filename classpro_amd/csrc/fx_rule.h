// fx_rule.h -- the rule of kmer_fixes.hip ("Fixing reads from a k-mer table" in include/classpro_amd.h) as plain functions
// that compile for the host as well, so that the rule can be checked without a device (tests/fx_rule_check.cpp).
//
//   gap      a maximal run [i, j] of absent k-mer positions of a read of n bases.  e = i+K-1 is the first base a
//            left-to-right reading cannot explain, f = j the last base a right-to-left reading cannot explain,
//            g = f-e+1 = (j-i+1)-K+1 and t = -g.
//   cand     the candidate edits of a closed gap, by ordinal and in the fixed order of the header: (del, ins) replaces
//            s[e, e+del) by ins.  fx_ncand counts the ordinals, fx_cand gives one; it needs the five bases s[e-4 .. e]
//            (K >= 5 and i >= 1, so they exist and are A C G T).  A candidate with e+del > n does not exist (fx_exists).
//   window   the k-mer positions of the edited sequence that are checked, clipped to the positions it has (fx_window),
//            and where a base of the edited sequence comes from (fx_source).
//   clash    fx_clash: two fixes that stand so close that the bases one removes lie behind the other's e.
//   apply    fx_applies says whether a record is an edit at all -- anything read from a record is checked here, so that no
//            content of a record makes a walk leave its arrays -- and fx_walk is the map from a read's bases to the
//            bases of the corrected read: a walk may begin at any base (the 64-base chunk of a lane), finds the records
//            at or behind it by a binary search, and then takes base after base.  cum[] is the INCLUSIVE scan of
//            fx_delta over all records of the batch.
#pragma once
#include <stdint.h>

#ifndef CP_HDM
#ifdef __HIPCC__
#define CP_HDM __host__ __device__ __forceinline__
#else
#define CP_HDM inline
#endif
#endif

#define FX_MAXD   4                        // max_indel at most
#define FX_MAXC   (2*FX_MAXD+3)            // candidates of one gap at most
#define FX_BACK   4                        // records before a walk's first whose removed bases may reach into it

enum { FX_NONE = 0, FX_ONE = 1, FX_MANY = 2, FX_OPEN = 3, FX_NOCAND = 4, FX_CLASH = 5 };

struct fx_fix { int64_t first, last; int32_t read; uint8_t status, del, nins, nacc; char ins[8]; };     // cp_kmer_fix

struct fx_edit { int del, nins; char ins[FX_MAXD]; };

CP_HDM int64_t fx_e(int64_t i, int K) { return i+(K-1); }
CP_HDM int64_t fx_g(int64_t i, int64_t j, int K) { return (j-i+1)-K+1; }

// the number of candidate ordinals of a closed gap
CP_HDM int fx_ncand(int64_t g, int D)
{ if (g >= 1) return (g <= D ? (int)(D-g+1) : 0)+(g == 1 ? 3 : 0);
  if (D < 1) return 0;
  const int64_t t = -g;
  const int m = (int)(t < D ? t : D);
  return D+4+(m >= 2 ? m-1 : 0);
}

// candidate c of fx_ncand(g, D); near[k] = s[e-4+k] for k = 0 .. 4, upper-case A C G T
CP_HDM fx_edit fx_cand(int c, int64_t g, int D, const char *near)
{ fx_edit x;
  x.del = 0; x.nins = 0;
  for (int k = 0; k < FX_MAXD; k++) x.ins[k] = 0;
  if (g >= 1)
    { const int nrem = g <= D ? (int)(D-g+1) : 0;
      if (c < nrem) { x.del = (int)g+c; return x; }       // the read had an insertion
      int k = c-nrem;                                      // a substitution: the k-th base that is not s[e]
      for (int b = 0; b < 4; b++)
        { const char ch = "ACGT"[b];
          if (ch == near[4]) continue;
          if (k-- == 0) { x.del = 1; x.nins = 1; x.ins[0] = ch; return x; }
        }
      x.del = 1; x.nins = 1; x.ins[0] = 'T';               // s[e] is none of the four: cannot be in a gap
      return x;
    }
  if (c < D) { x.del = c+1; return x; }
  if (c < D+4) { x.nins = 1; x.ins[0] = "ACGT"[c-D]; return x; }          // the read lost a base
  const int d = c-(D+4)+2;                                 // the read lost a copy of a tandem unit of d bases
  x.nins = d < FX_MAXD ? d : FX_MAXD;
  for (int k = 0; k < x.nins; k++) x.ins[k] = near[4-x.nins+k];
  return x;
}

CP_HDM bool fx_exists(int64_t e, int del, int64_t n) { return e+del <= n; }

// the checked positions [q0, q1] of the edited sequence, empty when q1 < q0
CP_HDM void fx_window(int64_t i, int K, int del, int nins, int64_t n, int64_t *q0, int64_t *q1)
{ const int64_t e = fx_e(i,K), len = n-del+nins;
  const int64_t hi = nins ? e+nins-1 : e-1;
  *q0 = i < 0 ? 0 : i;
  *q1 = hi < len-K ? hi : len-K;
}

// where base x of the edited sequence comes from: an index into s when >= 0, ins[-1-v] otherwise
CP_HDM int64_t fx_source(int64_t x, int64_t e, int del, int nins)
{ return x < e ? x : x < e+nins ? -1-(x-e) : x-nins+del; }

// a fix at e that removes del bases, and the fix at e_next > e behind it: they clash when e+del > e_next
CP_HDM bool fx_clash(int64_t e, int del, int64_t e_next) { return e+del > e_next; }

// ---------------------------------------------------------------------------------------------------------------------
// applying

// whether record k, one of the records [lo, hi) of read r of n bases, is an edit; *e its place
CP_HDM bool fx_applies(const fx_fix &x, int r, int64_t n, int K, int64_t *e)
{ *e = 0;
  if (x.status != FX_ONE || x.del > FX_MAXD || x.nins > FX_MAXD || x.read != r) return false;
  if (x.first < 0 || x.first >= n) return false;           // also: first+K-1 does not overflow
  *e = fx_e(x.first,K);
  return *e < n && *e+x.del <= n;
}

CP_HDM int64_t fx_delta(const fx_fix &x, int r, int64_t n, int K)
{ int64_t e;
  return fx_applies(x,r,n,K,&e) ? (int64_t)x.nins-(int64_t)x.del : 0;
}

CP_HDM int64_t fx_excl(const int64_t *cum, int64_t k) { return k > 0 ? cum[k-1] : 0; }

struct fx_walk
  { int64_t k, hi;                         // the next record and the end of the read's records
    int64_t shift;                         // output position - input position of a base that is kept
    int64_t skip_to;                       // bases before this one are removed
    int r, K;
    int64_t n;
  };

// a walk over read r (n bases, records [lo, hi)) that begins at base a
CP_HDM fx_walk fx_walk_begin(const fx_fix *fix, const int64_t *cum, int64_t lo, int64_t hi, int r, int64_t n, int K, int64_t a)
{ fx_walk w;
  w.r = r; w.K = K; w.n = n; w.hi = hi;
  int64_t x = lo, y = hi;                                  // the first record whose e is a or behind it
  while (x < y)
    { const int64_t mid = (x+y) >> 1;
      const int64_t f = fix[mid].first;
      if (f >= a-(K-1)) y = mid; else x = mid+1;
    }
  w.k = x;
  w.shift = fx_excl(cum,x)-fx_excl(cum,lo);
  w.skip_to = 0;
  for (int64_t m = 1; m <= FX_BACK && x-m >= lo; m++)
    { int64_t e;
      if (fx_applies(fix[x-m],r,n,K,&e) && e+fix[x-m].del > w.skip_to) w.skip_to = e+fix[x-m].del;
    }
  return w;
}

// base p of the read, in order: put(o, ch) is called for every base of the corrected read that base p brings, o its
// place in the corrected read
template <class PUT>
CP_HDM void fx_walk_step(fx_walk &w, const fx_fix *fix, int64_t p, char base, PUT put)
{ while (w.k < w.hi)
    { const fx_fix &x = fix[w.k];
      if (x.first > p-(w.K-1)) break;
      int64_t e;
      if (fx_applies(x,w.r,w.n,w.K,&e))
        { if (e == p)
            { for (int c = 0; c < (int)x.nins; c++) put(p+w.shift+c,x.ins[c]);
              if (p+x.del > w.skip_to) w.skip_to = p+x.del;
            }
          w.shift += (int64_t)x.nins-(int64_t)x.del;
        }
      w.k++;
    }
  if (p >= w.skip_to) put(p+w.shift,base);
}

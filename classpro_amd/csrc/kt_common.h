// kt_common.h -- what the two device k-mer tables share on the device: the label table of kmer_table.hip (class2cns)
// and the count table of kmer_counts.hip (kprof).  Keys, the hash, the lock-free claim protocol over any slot type that
// begins with the two key words, the read-only lookup, and the rolling walk over the k-mers of a flat batch.  The host
// side they share (creation, growth by rehash, the add driver, destruction) is kt_store.h, which includes this file.
//
// Both tables are open addressing with linear probing.  A slot starts with hi = key bits 125..63 and lo = key bits
// 62..0.  A key has at most 126 bits, so the all-ones word never is a half of a key and marks an EMPTY half.  An
// insert never waits on another lane: it CASes hi from EMPTY (or finds it equal), then lo from EMPTY (or finds it
// equal); a slot's (hi, lo) once set never changes, so every insert of one key stops at the same slot (the first one
// of its probe sequence whose final key is that key).  Probing is bounded (KT_PROBE).
#pragma once
#include <algorithm>

typedef unsigned __int128 kt_u128;

#define KT_EMPTY  0xFFFFFFFFFFFFFFFFull
#define KT_M63    0x7FFFFFFFFFFFFFFFull
#define KT_PROBE  64                       // slots looked at per insert / lookup before an insert counts as failed
#define KT_CHUNK  64                       // consecutive k-mer positions one lane rolls its key over
#define KT_BLOCK  256

__host__ __device__ static inline unsigned long long kt_mix(unsigned long long x)
{ x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

__device__ static inline unsigned long long kt_home(unsigned long long hi, unsigned long long lo)
{ return kt_mix(lo ^ kt_mix(hi ^ 0x9e3779b97f4a7c15ull)); }

__device__ static inline int kt_base(unsigned char c)                        // A C G T -> 0..3, anything else -1
{ return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

__device__ static inline unsigned long long kt_load(const unsigned long long *p)
{ return __hip_atomic_load(p,__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT); }

// Finds or claims the slot of (hi, lo); returns it, or NULL after KT_PROBE slots.  *claimed: this lane set lo.
template <class SLOT>
__device__ static inline SLOT *kt_find_or_claim(SLOT *tab, unsigned long long mask, unsigned long long hi,
                                                unsigned long long lo, bool *claimed)
{ unsigned long long s = kt_home(hi,lo) & mask;
  for (int p = 0; p < KT_PROBE; p++, s = (s+1) & mask)
    { SLOT *e = tab+s;
      unsigned long long h = kt_load(&e->hi);
      if (h == KT_EMPTY)
        { const unsigned long long o = atomicCAS(&e->hi,KT_EMPTY,hi);
          h = (o == KT_EMPTY) ? hi : o;
        }
      if (h != hi) continue;
      unsigned long long w = kt_load(&e->lo);
      if (w == KT_EMPTY)
        { const unsigned long long o = atomicCAS(&e->lo,KT_EMPTY,lo);
          if (o == KT_EMPTY) { w = lo; *claimed = true; }
          else w = o;
        }
      if (w == lo) return e;
    }
  return nullptr;
}

// Read-only lookup (the table is not written while it runs).
template <class SLOT>
__device__ static inline const SLOT *kt_lookup(const SLOT *tab, unsigned long long mask, unsigned long long hi,
                                               unsigned long long lo)
{ unsigned long long s = kt_home(hi,lo) & mask;
  for (int p = 0; p < KT_PROBE; p++, s = (s+1) & mask)
    { const SLOT *e = tab+s;
      const unsigned long long h = e->hi;
      if (h == KT_EMPTY) return nullptr;
      if (h == hi && e->lo == lo) return e;
    }
  return nullptr;
}

// Walks the k-mer positions [p0, p0+KT_CHUNK) of the flat batch (global base index j, k-mer = seq[j-K+1..j] of j's
// read r, j >= read start + K-1), rolling the forward key and its reverse complement one base at a time.  Calls
// f(r, j, ok, hi, lo) for every k-mer position; ok is false (and the key meaningless) for a k-mer that holds a byte
// other than upper-case A C G T.
template <bool CANON, class F>
__device__ static inline void kt_walk_all(const char *seq, const int64_t *seq_off, int nreads, int64_t total, int K,
                                          int64_t p0, F f)
{ const int64_t p1 = min(p0+(int64_t)KT_CHUNK,total);
  int lo_r = 0, hi_r = nreads;                          // the read holding p0: seq_off[r] <= p0 < seq_off[r+1]
  while (hi_r-lo_r > 1)
    { const int mid = (lo_r+hi_r) >> 1;
      if (seq_off[mid] <= p0) lo_r = mid; else hi_r = mid;
    }
  const kt_u128 kmask = (((kt_u128)1) << (2*K))-1;
  const int rshift = 2*K-2;
  int r = lo_r;
  for (int64_t p = p0; p < p1 && r < nreads; r++)
    { const int64_t rs = seq_off[r], re = seq_off[r+1];
      if (re <= p) continue;                            // empty reads
      const int64_t q1 = min(p1,re);
      const int64_t first = max(p,rs+K-1);
      if (first < q1)
        { kt_u128 fw = 0, rc = 0;
          int valid = 0;
          for (int64_t j = first-K+1; j < q1; j++)
            { const int b = kt_base((unsigned char)seq[j]);
              if (b < 0) { valid = 0; fw = 0; rc = 0; }
              else
                { fw = ((fw << 2) | (kt_u128)b) & kmask;
                  rc = (rc >> 2) | (((kt_u128)(3-b)) << rshift);
                  valid++;
                }
              if (j < first) continue;
              const kt_u128 key = (CANON && rc < fw) ? rc : fw;
              f(r,j,valid >= K,(unsigned long long)(key >> 63),(unsigned long long)key & KT_M63);
            }
        }
      p = q1;
    }
}

// The canonical walk for callers that must know WHICH strand gave the key: calls f(r, j, ok, hi, lo, rc_won) for every
// k-mer position; rc_won says that the reverse complement is strictly the smaller of the two strings, so it is false for a
// palindromic k-mer (and meaningless, like the key, when ok is false).  Positions and keys are those of kt_walk_all<true>.
template <class F>
__device__ static inline void kt_walk_strand(const char *seq, const int64_t *seq_off, int nreads, int64_t total, int K,
                                             int64_t p0, F f)
{ const int64_t p1 = min(p0+(int64_t)KT_CHUNK,total);
  int lo_r = 0, hi_r = nreads;                          // the read holding p0: seq_off[r] <= p0 < seq_off[r+1]
  while (hi_r-lo_r > 1)
    { const int mid = (lo_r+hi_r) >> 1;
      if (seq_off[mid] <= p0) lo_r = mid; else hi_r = mid;
    }
  const kt_u128 kmask = (((kt_u128)1) << (2*K))-1;
  const int rshift = 2*K-2;
  int r = lo_r;
  for (int64_t p = p0; p < p1 && r < nreads; r++)
    { const int64_t rs = seq_off[r], re = seq_off[r+1];
      if (re <= p) continue;                            // empty reads
      const int64_t q1 = min(p1,re);
      const int64_t first = max(p,rs+K-1);
      if (first < q1)
        { kt_u128 fw = 0, rc = 0;
          int valid = 0;
          for (int64_t j = first-K+1; j < q1; j++)
            { const int b = kt_base((unsigned char)seq[j]);
              if (b < 0) { valid = 0; fw = 0; rc = 0; }
              else
                { fw = ((fw << 2) | (kt_u128)b) & kmask;
                  rc = (rc >> 2) | (((kt_u128)(3-b)) << rshift);
                  valid++;
                }
              if (j < first) continue;
              const bool won = rc < fw;
              const kt_u128 key = won ? rc : fw;
              f(r,j,valid >= K,(unsigned long long)(key >> 63),(unsigned long long)key & KT_M63,won);
            }
        }
      p = q1;
    }
}

// The same walk for callers that only want the k-mers of upper-case A C G T: calls f(j, hi, lo) for each of them and
// returns the number of the others.
template <bool CANON, class F>
__device__ static inline unsigned long long kt_walk(const char *seq, const int64_t *seq_off, int nreads, int64_t total,
                                                    int K, int64_t p0, F f)
{ unsigned long long nskip = 0;
  kt_walk_all<CANON>(seq,seq_off,nreads,total,K,p0,
    [&](int, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
    { if (!ok) { nskip++; return; }
      f(j,hi,lo);
    });
  return nskip;
}

static int kt_grid(unsigned long long n)
{ return (int)std::min<unsigned long long>((n+KT_BLOCK-1)/KT_BLOCK,8192); }

static unsigned long long kt_pow2_at_least(unsigned long long n)
{ unsigned long long s = 64;
  while (s < n) s <<= 1;
  return s;
}

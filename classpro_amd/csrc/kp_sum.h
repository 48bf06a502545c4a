// kp_sum.h -- the words, the summary algebra and the walk of kmer_paths.hip ("Reads through the unitig graph" in
// include/classpro_amd.h), as plain functions that compile for the host as well, so that the three passes can be checked
// without a device (tests/kp_sum_check.cpp).
//
// Every base position j of the flat batch has one 64-bit WORD.  A step (x, k) is x << 32 | k: x the oriented unitig (below
// 2^31), k the RAW place d_at >> 1 (below 2^30), so bit 31 is free and marks the three words that are no step: KP_ABSENT,
// KP_OTHER and KP_NOKMER (no k-mer ends at j).  Bit 63, KP_FIRST, is set on the first k-mer position of a read, whatever its
// word.  A word CONTINUES the word before it when both are steps of one x, the later one is no first position, and k went
// up by one on '+' (x even) or down by one on '-' (x odd): that is q + 1 in both cases, without the unitig's length.  A
// HEAD is a step that does not continue the word before it; it is JOINED when that word is a step all the same.  Because
// K >= 2, the position before a first k-mer position and the position after a read's last are never steps, so reads need
// no rule of their own.
//   kp_sum   of a stretch of positions: its heads, its joined heads and the position of its last head (meaningless without
//            a head).  Whether a position is a head depends on its own word and the one before, which every lane can load,
//            so nothing is left undecided: kp_join adds the counts and keeps the later `last`.  Associative, the all-zero
//            summary is its identity.
//   kp_walk  the record index and the last head before a position, and the read the walk is in.  kp_walk_step takes one
//            word: a boundary (the word before is a step, this one does not continue it) stores n of the record before and
//            adds it to cov; a head stores first, x, q, read and flags of its own record and, when joined, adds one to the
//            support of the arc it came by.  kp_walk_end closes the batch.  The same lanes store seg_off, as kr_walk does.
#pragma once
#include <stdint.h>

#ifndef CP_HDM
#ifdef __HIPCC__
#define CP_HDM __host__ __device__ __forceinline__
#else
#define CP_HDM inline
#endif
#endif

#define KP_FIRST   (1ull << 63)
#define KP_NOSTEP  0x80000000ull           // bit 31 of a word: no step
#define KP_ABSENT  0x80000000ull
#define KP_OTHER   0x80000001ull
#define KP_NOKMER  0x80000002ull
#define KP_KMASK   0x3fffffffull

struct kp_seg { int64_t first, x; int32_t n, q, read, flags; };          // cp_path_seg

struct kp_sum { int64_t heads, joined, last, pad; };

CP_HDM bool kp_step(unsigned long long w) { return !(w & KP_NOSTEP); }
CP_HDM int64_t kp_x(unsigned long long w) { return (int64_t)((w >> 32) & 0x7fffffffull); }

CP_HDM bool kp_cont(unsigned long long pw, unsigned long long w)
{ if (((pw | w) & KP_NOSTEP) || (w & KP_FIRST) || kp_x(pw) != kp_x(w)) return false;
  const unsigned int kp = (unsigned int)pw, k = (unsigned int)w;
  return (kp_x(w) & 1) ? k+1 == kp : kp+1 == k;
}

// the stretch followed by position j with word w, the word before it being pw
CP_HDM void kp_push(kp_sum &a, unsigned long long pw, unsigned long long w, int64_t j)
{ if (!kp_step(w) || kp_cont(pw,w)) return;
  a.heads++;
  a.joined += (kp_step(pw) && !(w & KP_FIRST)) ? 1 : 0;
  a.last = j;
}

CP_HDM kp_sum kp_join(const kp_sum &l, const kp_sum &r)
{ kp_sum o;
  o.heads = l.heads+r.heads;
  o.joined = l.joined+r.joined;
  o.last = r.heads ? r.last : l.last;
  o.pad = 0;
  return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// the walk

CP_HDM void kp_add(int64_t *dst, int64_t v)
{
#ifdef __HIP_DEVICE_COMPILE__
  atomicAdd((unsigned long long *)dst,(unsigned long long)v);
#else
  *dst += v;
#endif
}

struct kp_args
  { const char *seq;
    const int64_t *seq_off;
    int nreads, K;
    const int64_t *uoff;                   // the offsets of the unitigs' sequences, ucount+1
    int64_t ucount;
    const int64_t *loff;                   // the arcs: 2*gcount+1 offsets, the base of each of `links`
    const uint8_t *lbase;
    int64_t gcount, links;
    kp_seg *segs;
    int64_t capacity;
    int64_t *seg_off, *cov, *support;      // cov and support null: not added to
  };

struct kp_walk
  { int64_t H;                             // records before the next head
    int64_t last;                          // the position of the last head
    int r;                                 // the read the walk is in
    int64_t rs;                            // seq_off[r]
  };

CP_HDM int64_t kp_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : v > n-1 ? n-1 : v; }

// the largest r in [0, nreads) with seq_off[r] <= p (p >= 0 = seq_off[0])
CP_HDM int kp_read_of(const int64_t *seq_off, int nreads, int64_t p)
{ int lo_r = 0, hi_r = nreads;
  while (hi_r-lo_r > 1)
    { const int mid = (lo_r+hi_r) >> 1;
      if (seq_off[mid] <= p) lo_r = mid; else hi_r = mid;
    }
  return lo_r;
}

// a walk that begins at position p0, before which lies the stretch summarised by `in`
CP_HDM kp_walk kp_walk_begin(const kp_sum &in, const kp_args &a, int64_t p0)
{ kp_walk x;
  x.H = in.heads; x.last = in.last;
  x.r = kp_read_of(a.seq_off,a.nreads,p0);
  x.rs = a.seq_off[x.r];
  return x;
}

// the segment under way, whose last word is pw, ends before position j
CP_HDM void kp_walk_close(const kp_walk &x, unsigned long long pw, int64_t j, const kp_args &a)
{ const int64_t n = j-x.last;
  if (x.H >= 1 && x.H-1 < a.capacity) a.segs[x.H-1].n = (int32_t)n;
  if (a.cov && a.ucount > 0) kp_add(a.cov+kp_clamp(kp_x(pw) >> 1,a.ucount),n);
}

// seg_off[q] = H for q and for the reads without a k-mer position just before it
CP_HDM void kp_walk_offsets(int q, int64_t H, const kp_args &a)
{ for (; ; q--)
    { a.seg_off[q] = H;
      if (q == 0 || a.seq_off[q]-a.seq_off[q-1] >= a.K) break;
    }
}

// the word w of position j, the word before it being pw
CP_HDM void kp_walk_step(kp_walk &x, unsigned long long pw, unsigned long long w, int64_t j, const kp_args &a)
{ if (w & KP_FIRST)                                        // a read begins
    { while (x.r+1 < a.nreads && a.seq_off[x.r+1] <= j) x.r++;
      x.rs = a.seq_off[x.r];
      kp_walk_offsets(x.r,x.H,a);
    }
  if (kp_cont(pw,w)) return;
  if (kp_step(pw)) kp_walk_close(x,pw,j,a);
  if (!kp_step(w)) return;
  const bool joined = kp_step(pw) && !(w & KP_FIRST);
  if (x.H < a.capacity && a.ucount > 0)
    { const int64_t xo = kp_x(w), u = kp_clamp(xo >> 1,a.ucount);
      const int64_t nodes = a.uoff[u+1]-a.uoff[u]-(a.K-1), k = (int64_t)(w & KP_KMASK);
      kp_seg *o = a.segs+x.H;
      o->first = j-x.rs-(a.K-1);
      o->x = xo;
      o->q = (int32_t)((xo & 1) ? nodes-1-k : k);
      o->read = x.r;
      o->flags = joined ? 1 : 0;
    }
  if (joined && a.support && a.gcount > 0 && a.links > 0)
    { const int64_t xp = kp_clamp(kp_x(pw),2*a.gcount);
      const int64_t a0 = kp_clamp(a.loff[xp],a.links+1);
      int64_t a1 = kp_clamp(a.loff[xp+1],a.links+1);
      if (a1 > a0+4) a1 = a0+4;
      const unsigned char ch = (unsigned char)a.seq[j];
      const unsigned int c = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : 3u;
      for (int64_t e = a0; e < a1; e++)
        if (a.lbase[e] == c) { kp_add(a.support+e,1); break; }
    }
  x.last = j;
  x.H++;
}

// the batch of `total` positions ends behind the walk's last position, whose word is pw
CP_HDM void kp_walk_end(const kp_walk &x, unsigned long long pw, int64_t total, const kp_args &a)
{ if (kp_step(pw)) kp_walk_close(x,pw,total,a);
  kp_walk_offsets(a.nreads,x.H,a);
}

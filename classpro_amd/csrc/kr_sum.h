// kr_sum.h -- the summary algebra of kmer_runs.hip ("Runs of k-mer states along reads" in include/classpro_amd.h), as
// plain functions that compile for the host as well, so that the algebra can be checked without a device.
//
// A stretch of consecutive positions of the flat batch is summarised by what a walk over it would need to know of the
// stretch before it, and what it leaves for the stretch after it.  A position is a TOKEN: optionally a RESET (it is the
// first k-mer position of a read, so nothing before it matters any more), then either a state that counts or nothing (a
// state in `skip`, or no k-mer position at all).  A HEAD is a counting position that begins a run: the first of its read,
// or one whose state differs from that of the counting position before it.
//   reset    the stretch holds a reset.
//   pre      the state of the first counting position that lies before any reset.  Whether it is a head depends on the
//            stretch before, so it is not in `heads`; every other head of the stretch is decided inside it.
//   heads    the decided heads whose state is in `emit`.
//   tail     the last counting position after the last reset: its state, its position in the batch and n, the number of
//            counting positions of its run inside the stretch.
//   open     that run begins at the stretch's first counting position and there is no reset: it may go on to the left,
//            and then the n of the stretch before is added to it.
// kr_join is associative, not commutative, and the all-zero summary is its identity; a lane pushes its positions one by
// one, a block joins its lanes, a single small kernel joins the blocks.  A summary whose left end is a reset has nothing
// undecided: its tail is the run under way and its `heads` the number of records before the next position.
//
// The second half is the WALK that stores the records: kr_walk holds the run under way, the number of records so far and the
// read a lane is in; kr_walk_step takes one state byte, kr_walk_end closes the batch.  kr_write_kernel and the host check
// of tests/kr_sum_check.cpp run the same functions.
#pragma once
#include <stdint.h>

#ifndef CP_HDM
#ifdef __HIPCC__
#define CP_HDM __host__ __device__ __forceinline__
#else
#define CP_HDM inline
#endif
#endif

#define KR_NOKMER   5u                     // state byte of a position that is no k-mer position
#define KR_FIRST    0x80u                  // in a state byte: the first k-mer position of a read
#define KR_RESET    1u                     // flags of a summary
#define KR_PRE      2u
#define KR_TAIL     32u
#define KR_OPEN     512u

struct kr_sum
  { int64_t p, n, heads;
    unsigned int flags;                    // KR_RESET | KR_PRE | pre state << 2 | KR_TAIL | tail state << 6 | KR_OPEN
    unsigned int pad;
  };

CP_HDM unsigned int kr_pre_s(unsigned int f)  { return (f >> 2) & 7u; }
CP_HDM unsigned int kr_tail_s(unsigned int f) { return (f >> 6) & 7u; }

// the stretch followed by one position: `first` a reset, `s` its state (KR_NOKMER or a state in skip: nothing counts)
CP_HDM void kr_push(kr_sum &a, bool first, unsigned int s, int64_t j, unsigned int skip, unsigned int emit)
{ if (first) a.flags = (a.flags | KR_RESET) & ~(KR_TAIL | KR_OPEN | (7u << 6));
  if (s >= KR_NOKMER || ((skip >> s) & 1u)) return;
  if (!(a.flags & (KR_RESET | KR_PRE)))
    { a.flags |= KR_PRE | (s << 2) | KR_TAIL | (s << 6) | KR_OPEN;
      a.p = j; a.n = 1;
      return;
    }
  if ((a.flags & KR_TAIL) && kr_tail_s(a.flags) == s) { a.p = j; a.n++; return; }
  a.heads += (emit >> s) & 1u;
  a.flags = (a.flags & ~(KR_OPEN | (7u << 6))) | KR_TAIL | (s << 6);
  a.p = j; a.n = 1;
}

CP_HDM kr_sum kr_join(const kr_sum &l, const kr_sum &r, unsigned int emit)
{ kr_sum o;
  o.pad = 0;
  o.heads = l.heads+r.heads;
  unsigned int f = (l.flags | r.flags) & KR_RESET;
  if (l.flags & (KR_RESET | KR_PRE)) f |= l.flags & (KR_PRE | (7u << 2));
  else f |= r.flags & (KR_PRE | (7u << 2));
  if (r.flags & KR_PRE)                                   // the first counting position of r: decided by l, if l can
    { if (l.flags & KR_TAIL) o.heads += (kr_tail_s(l.flags) != kr_pre_s(r.flags)) ? ((emit >> kr_pre_s(r.flags)) & 1u) : 0u;
      else if (l.flags & KR_RESET) o.heads += (emit >> kr_pre_s(r.flags)) & 1u;
    }
  if (r.flags & KR_TAIL)
    { const bool cont = (r.flags & KR_OPEN) && (l.flags & KR_TAIL) && kr_tail_s(l.flags) == kr_tail_s(r.flags);
      const bool open = (r.flags & KR_OPEN) && ((l.flags & KR_TAIL) ? (cont && (l.flags & KR_OPEN)) : !(l.flags & KR_RESET));
      f |= (r.flags & (KR_TAIL | (7u << 6))) | (open ? KR_OPEN : 0u);
      o.p = r.p; o.n = r.n+(cont ? l.n : 0);
    }
  else if (r.flags & KR_RESET) { o.p = 0; o.n = 0; }
  else
    { f |= l.flags & (KR_TAIL | (7u << 6) | KR_OPEN);
      o.p = l.p; o.n = l.n;
    }
  o.flags = f;
  return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// the walk

struct kr_rec { int64_t first, last, n; int32_t read, state; };          // cp_kmer_run

struct kr_walk
  { int xs;                                // the state of the run under way, -1: none
    int64_t xp, xn;                        // its last position in the batch and its n so far
    int64_t H;                             // records before the next head
    int r;                                 // the read the walk is in
    int64_t rs;                            // seq_off[r]
  };

// the largest r in [0, nreads) with seq_off[r] <= p (p >= 0 = seq_off[0])
CP_HDM int kr_read_of(const int64_t *seq_off, int nreads, int64_t p)
{ int lo_r = 0, hi_r = nreads;
  while (hi_r-lo_r > 1)
    { const int mid = (lo_r+hi_r) >> 1;
      if (seq_off[mid] <= p) lo_r = mid; else hi_r = mid;
    }
  return lo_r;
}

// a walk that begins at position p0, which the summary `in` (its left end a reset) reaches
CP_HDM kr_walk kr_walk_begin(const kr_sum &in, const int64_t *seq_off, int nreads, int64_t p0)
{ kr_walk x;
  x.xs = (in.flags & KR_TAIL) ? (int)kr_tail_s(in.flags) : -1;
  x.xp = in.p; x.xn = in.n; x.H = in.heads;
  x.r = kr_read_of(seq_off,nreads,p0);
  x.rs = seq_off[x.r];
  return x;
}

// the run under way ends: its last position and n are known; `start` is the first base of its read
CP_HDM void kr_walk_close(const kr_walk &x, int64_t start, unsigned int emit, int K, kr_rec *runs, int64_t capacity)
{ if (((emit >> x.xs) & 1u) && x.H >= 1 && x.H-1 < capacity)
    { kr_rec *o = runs+(x.H-1);
      o->last = x.xp-start-(K-1);
      o->n = x.xn;
    }
}

// run_off[q] = H for q and for the reads without a k-mer position just before it
CP_HDM void kr_walk_offsets(int q, int64_t H, const int64_t *seq_off, int K, int64_t *run_off)
{ for (; ; q--)
    { run_off[q] = H;
      if (q == 0 || seq_off[q]-seq_off[q-1] >= K) break;
    }
}

// the state byte b of position j
CP_HDM void kr_walk_step(kr_walk &x, unsigned int b, int64_t j, unsigned int skip, unsigned int emit, const int64_t *seq_off,
                         int nreads, int K, kr_rec *runs, int64_t capacity, int64_t *run_off)
{ const unsigned int s = b & 7u;
  if (b & KR_FIRST)                                        // a read begins: the one before is over
    { if (x.xs >= 0)
        { kr_walk_close(x,seq_off[kr_read_of(seq_off,nreads,x.xp)],emit,K,runs,capacity);
          x.xs = -1;
        }
      while (x.r+1 < nreads && seq_off[x.r+1] <= j) x.r++;
      x.rs = seq_off[x.r];
      kr_walk_offsets(x.r,x.H,seq_off,K,run_off);
    }
  if (s >= KR_NOKMER || ((skip >> s) & 1u)) return;
  if (x.xs == (int)s) { x.xp = j; x.xn++; return; }
  if (x.xs >= 0) kr_walk_close(x,x.rs,emit,K,runs,capacity);
  if ((emit >> s) & 1u)
    { if (x.H < capacity)
        { kr_rec *o = runs+x.H;
          o->first = j-x.rs-(K-1);
          o->read = x.r;
          o->state = (int32_t)s;
        }
      x.H++;
    }
  x.xs = (int)s; x.xp = j; x.xn = 1;
}

// the batch ends behind the walk's last position
CP_HDM void kr_walk_end(const kr_walk &x, unsigned int emit, const int64_t *seq_off, int nreads, int K, kr_rec *runs,
                        int64_t capacity, int64_t *run_off)
{ if (x.xs >= 0) kr_walk_close(x,seq_off[kr_read_of(seq_off,nreads,x.xp)],emit,K,runs,capacity);
  kr_walk_offsets(nreads,x.H,seq_off,K,run_off);
}

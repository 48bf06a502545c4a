// kmer_counts.hip -- k-mer count table on the device (kprof): how often each distinct canonical k-mer occurs in the
// batches added, then the per-read count profiles and the FASTK histogram of those counts.  Semantics:
// include/classpro_amd.h, "K-mer count table".  Included by capi.hip after kmer_table.hip (set_err, HIPCHK and the
// library's error contract are shared); keys, hash, claim protocol, lookup and walk come from kt_common.h, the table's
// life cycle (creation, growth, the add driver, destruction) from kt_store.h.  This file holds what is the count
// table's own: slot, counters, the add, profile, relative-label and histogram kernels and their entry points.
//
// One slot per key: hi, lo, a 64-bit count that cannot wrap (at most one add per base ever seen), and a pad word that
// keeps the slot at 32 bytes: a slot then never spans two 64-byte memory requests, and a probe costs what a probe of the
// label table costs (measured against a build without the pad word).
//   insert     find or claim the slot, one 64-bit atomic add; a probe run past KT_PROBE sets the position's bit in a
//              failure bitmap, the host grows the table and replays exactly those positions;
//   profile    a read-only lookup per position; a block stages its 16384 cells in LDS and stores them as 32-bit words;
//   rel labels a read-only lookup per position of a batch of another sequence set; labels staged in LDS (see there);
//   histogram  a slot sweep, counts below 256 binned in LDS per block, the tail by 64-bit global atomics.
// A FILTERED table (cp_kmer_counts_create_filtered) keeps the keys seen once out of the slots.  A bit
// array in device memory stands in front of the table; a key owns one 64-bit word of it and up to four bits in that word.
//   mark       one returning 64-bit atomic OR per position tests and sets the key's bits; only a key whose bits were all
//              set already is claimed in the table (no count yet).  Atomics on one word are totally ordered, so of two or
//              more occurrences of a key at most one finds a bit unset: every key that occurs twice is in the table.
//              Failed claims go through the same failure bitmap, growth and replay; a replay does not ask the filter again.
//   count      the keys are fixed now: a read-only lookup per position, a 64-bit atomic add on a key that is there, a
//              tally (n_single) of those that are not -- each of them occurs exactly once.
//   profile    the same kernel with "absent = 1".
// The per-lane tallies (claims, failures, skips, adds) are summed over the wave first: one atomic per wave and counter.
#include "kt_store.h"

#define KC_ERR_ABSENT 1u                   // a profile pass met a k-mer that was never added
#define KC_LOW_BINS   256                  // histogram bins kept in LDS per block
#define KC_CELLS      (KT_BLOCK*KT_CHUNK)  // k-mer positions (at most that many profile cells) per block

struct kc_slot { unsigned long long hi, lo, cnt, pad; };

struct kc_ctl                                                                 // device-side counters of one table
  { unsigned long long n_fail, n_occ, n_skip, n_rfail;                        // the store's: kt_store.h
    unsigned long long n_add;             // counted occurrences
    unsigned int err, pad;
    unsigned long long n_mark;            // filtered table: valid k-mer positions of the mark passes
    unsigned long long n_single;          // filtered table: positions of the count passes whose key is not in the table
    unsigned long long n_badkey;          // cp_kmer_counts_add_keys: keys of the last call that are no keys of K bases
  };

// adds the wave's sum of v to *dst (one atomic per wave; every lane of the wave must call)
__device__ static inline void kc_wave_add(unsigned long long *dst, unsigned long long v)
{ for (int w = warpSize/2; w > 0; w >>= 1) v += __shfl_down(v,w);
  if ((threadIdx.x & (warpSize-1)) == 0 && v) atomicAdd(dst,v);
}

// One add pass (REPLAY = false) or a replay of the positions whose bit is set in fail_in (REPLAY = true).
template <bool REPLAY>
__global__ void __launch_bounds__(KT_BLOCK) kc_add_kernel(kc_slot *tab, unsigned long long mask, const char *seq,
                                                          const int64_t *seq_off, int nreads, int64_t total, int K,
                                                          const unsigned int *fail_in, unsigned int *fail_out,
                                                          kc_ctl *ctl)
{ const int64_t p0 = ((int64_t)blockIdx.x*blockDim.x+threadIdx.x)*KT_CHUNK;
  unsigned long long nfail = 0, nocc = 0, nadd = 0, nskip = 0;
  if (p0 < total)
    nskip = kt_walk<true>(seq,seq_off,nreads,total,K,p0,
      [&](int64_t j, unsigned long long hi, unsigned long long lo)
      { if (REPLAY && !((fail_in[j >> 5] >> (j & 31)) & 1u)) return;
        bool claimed = false;
        kc_slot *e = kt_find_or_claim(tab,mask,hi,lo,&claimed);
        nocc += claimed;
        if (!e)
          { atomicOr(&fail_out[j >> 5],1u << (j & 31));
            nfail++;
            return;
          }
        atomicAdd(&e->cnt,1ull);
        nadd++;
      });
  kc_wave_add(&ctl->n_fail,nfail);
  kc_wave_add(&ctl->n_occ,nocc);
  kc_wave_add(&ctl->n_add,nadd);
  if (!REPLAY) kc_wave_add(&ctl->n_skip,nskip);
}

// The add pass over n EXPLICIT keys (cp_kmer_counts_add_keys), +1 each: the "positions" of the failure bitmap are the key
// indices, so failed inserts, growth and replay are those of kc_add_kernel.  A key that does not fit 2K bits or whose lo
// has bit 63 set is left out and counted; hi null: every hi is 0.
template <bool REPLAY>
__global__ void __launch_bounds__(KT_BLOCK) kc_add_keys_kernel(kc_slot *tab, unsigned long long mask,
                                                               const unsigned long long *khi, const unsigned long long *klo,
                                                               int64_t n, int K, const unsigned int *fail_in,
                                                               unsigned int *fail_out, kc_ctl *ctl)
{ unsigned long long nfail = 0, nocc = 0, nadd = 0, nbad = 0;
  for (int64_t j = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; j < n; j += (int64_t)gridDim.x*blockDim.x)
    { if (REPLAY && !((fail_in[j >> 5] >> (j & 31)) & 1u)) continue;
      const unsigned long long hi = khi ? khi[j] : 0, lo = klo[j];
      if (lo > KT_M63 || ((((kt_u128)hi) << 63) >> (2*K)) != 0 || (2*K < 63 && (lo >> (2*K)) != 0))
        { nbad++;
          continue;
        }
      bool claimed = false;
      kc_slot *e = kt_find_or_claim(tab,mask,hi,lo,&claimed);
      nocc += claimed;
      if (!e)
        { atomicOr(&fail_out[j >> 5],1u << (j & 31));
          nfail++;
          continue;
        }
      atomicAdd(&e->cnt,1ull);
      nadd++;
    }
  kc_wave_add(&ctl->n_fail,nfail);
  kc_wave_add(&ctl->n_occ,nocc);
  kc_wave_add(&ctl->n_add,nadd);
  if (!REPLAY) kc_wave_add(&ctl->n_badkey,nbad);
}

// The filter of a filtered table: `wmask`+1 64-bit words.  The word and the four bit positions of a key come from a hash
// of their own: the same mixer as kt_home with another constant, word index from bits 24.., bit positions from the four
// 6-bit fields below them (some of the four may coincide), so nothing is shared with the slot index (kt_home's low bits).
#define KF_SALT 0xd6e8feb86659fd93ull

__host__ __device__ static inline unsigned long long kf_hash(unsigned long long hi, unsigned long long lo)
{ return kt_mix(lo ^ kt_mix(hi ^ KF_SALT)); }

__host__ __device__ static inline unsigned long long kf_bits(unsigned long long h)
{ return (1ull << (h & 63)) | (1ull << ((h >> 6) & 63)) | (1ull << ((h >> 12) & 63)) | (1ull << ((h >> 18) & 63)); }

// sets the key's bits; true when all of them were set before (one device-scope atomic on one word: see the file comment)
__device__ static inline bool kf_test_and_set(unsigned long long *filter, unsigned long long wmask,
                                              unsigned long long hi, unsigned long long lo)
{ const unsigned long long h = kf_hash(hi,lo), m = kf_bits(h);
  const unsigned long long old = __hip_atomic_fetch_or(filter+((h >> 24) & wmask),m,__ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT);
  return (old & m) == m;
}

// One mark pass of a filtered table (REPLAY = false) or a replay of the claims that failed (REPLAY = true: those
// positions were judged "seen before" already, the filter is not asked again).
template <bool REPLAY>
__global__ void __launch_bounds__(KT_BLOCK) kc_mark_kernel(kc_slot *tab, unsigned long long mask,
                                                           unsigned long long *filter, unsigned long long wmask,
                                                           const char *seq, const int64_t *seq_off, int nreads,
                                                           int64_t total, int K, const unsigned int *fail_in,
                                                           unsigned int *fail_out, kc_ctl *ctl)
{ const int64_t p0 = ((int64_t)blockIdx.x*blockDim.x+threadIdx.x)*KT_CHUNK;
  unsigned long long nfail = 0, nocc = 0, nmark = 0;
  if (p0 < total)
    (void)kt_walk<true>(seq,seq_off,nreads,total,K,p0,
      [&](int64_t j, unsigned long long hi, unsigned long long lo)
      { if (REPLAY)
          { if (!((fail_in[j >> 5] >> (j & 31)) & 1u)) return; }
        else
          { nmark++;
            if (!kf_test_and_set(filter,wmask,hi,lo)) return;
          }
        bool claimed = false;
        kc_slot *e = kt_find_or_claim(tab,mask,hi,lo,&claimed);
        nocc += claimed;
        if (!e)
          { atomicOr(&fail_out[j >> 5],1u << (j & 31));
            nfail++;
          }
      });
  kc_wave_add(&ctl->n_fail,nfail);
  kc_wave_add(&ctl->n_occ,nocc);
  if (!REPLAY) kc_wave_add(&ctl->n_mark,nmark);
}

// The count pass of a filtered table: its keys are fixed, so nothing can fail and nothing grows.
__global__ void __launch_bounds__(KT_BLOCK) kc_count_kernel(kc_slot *tab, unsigned long long mask, const char *seq,
                                                            const int64_t *seq_off, int nreads, int64_t total, int K,
                                                            kc_ctl *ctl)
{ const int64_t p0 = ((int64_t)blockIdx.x*blockDim.x+threadIdx.x)*KT_CHUNK;
  unsigned long long nadd = 0, nsingle = 0, nskip = 0;
  if (p0 < total)
    nskip = kt_walk<true>(seq,seq_off,nreads,total,K,p0,
      [&](int64_t, unsigned long long hi, unsigned long long lo)
      { const kc_slot *e = kt_lookup((const kc_slot *)tab,mask,hi,lo);
        if (!e) { nsingle++; return; }
        atomicAdd(&const_cast<kc_slot *>(e)->cnt,1ull);
        nadd++;
      });
  kc_wave_add(&ctl->n_add,nadd);
  kc_wave_add(&ctl->n_single,nsingle);
  kc_wave_add(&ctl->n_skip,nskip);
}

// The prof cell of the k-mer position j of read r is prof_off[r] + j - seq_off[r] - (K-1).  Cells follow the k-mer
// positions in order, so the cells of a block's KC_CELLS positions are one contiguous run [q0, q0+n): staged in LDS,
// then stored by the whole block, two cells per lane and store.  The two halves are shared by the profile kernel and
// the relative-label kernel.

// threads 0 and 1: the first cell at or after position b0 / b1 into run[0] / run[1]
__device__ static inline void kc_cell_run(const int64_t *seq_off, const int64_t *prof_off, int nreads, int64_t total,
                                          int K, int64_t b0, int64_t b1, int64_t *run)
{ if (threadIdx.x < 2)
    { const int64_t p = threadIdx.x ? b1 : b0;
      int lo_r = 0, hi_r = nreads;
      while (hi_r-lo_r > 1)
        { const int mid = (lo_r+hi_r) >> 1;
          if (seq_off[mid] <= p) lo_r = mid; else hi_r = mid;
        }
      const int64_t in = p-seq_off[lo_r]-(K-1), len = prof_off[lo_r+1]-prof_off[lo_r];
      run[threadIdx.x] = p >= total ? prof_off[nreads] : prof_off[lo_r]+min(max(in,(int64_t)0),len);
    }
}

// the whole block: cell[0..n) to dst[0..n) as 32-bit words, the cell before the first 4-byte boundary and the last odd
// one on their own
__device__ static inline void kc_store_cells(const uint16_t *cell, uint16_t *dst, int64_t n)
{ const int head = (int)(((uintptr_t)dst >> 1) & 1);     // cells before the first 4-byte boundary
  const int64_t npair = (n-head) >> 1;
  if (threadIdx.x == 0)
    { if (head) dst[0] = cell[0];
      if ((n-head) & 1) dst[n-1] = cell[n-1];
    }
  for (int64_t i = threadIdx.x; i < npair; i += KT_BLOCK)
    *(unsigned int *)(dst+head+2*i) = (unsigned int)cell[head+2*i] | ((unsigned int)cell[head+2*i+1] << 16);
}

// ONCE: the table is a filtered one, where a valid k-mer that is absent occurs exactly once (cell 1, no error)
template <bool ONCE>
__global__ void __launch_bounds__(KT_BLOCK) kc_profile_kernel(const kc_slot *tab, unsigned long long mask,
                                                              const char *seq, const int64_t *seq_off,
                                                              const int64_t *prof_off, int nreads, int64_t total, int K,
                                                              uint16_t *prof, kc_ctl *ctl)
{ __shared__ uint16_t cell[KC_CELLS];
  __shared__ int64_t run[2];
  const int64_t b0 = (int64_t)blockIdx.x*KC_CELLS, b1 = min(b0+(int64_t)KC_CELLS,total);
  kc_cell_run(seq_off,prof_off,nreads,total,K,b0,b1,run);
  __syncthreads();
  const int64_t q0 = run[0];
  const int64_t n = min(max(run[1]-q0,(int64_t)0),min((int64_t)KC_CELLS,prof_off[nreads]-q0));
  const int64_t p0 = b0+(int64_t)threadIdx.x*KT_CHUNK;
  unsigned int err = 0;
  int cur = -1;                                          // the read whose cell base is held
  int64_t base = 0;
  if (p0 < total)
    kt_walk_all<true>(seq,seq_off,nreads,total,K,p0,
      [&](int r, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
      { if (r != cur) { cur = r; base = prof_off[r]-seq_off[r]-(K-1)-q0; }
        unsigned long long c = 0;
        if (ok)
          { const kc_slot *e = kt_lookup(tab,mask,hi,lo);
            if (e) c = min(e->cnt,(unsigned long long)CP_MAX_KMER_CNT);
            else if (ONCE) c = 1;
            else err |= KC_ERR_ABSENT;                   // a k-mer that was never added: the caller's error
          }
        const int64_t i = base+j;
        if ((unsigned long long)i < (unsigned long long)n) cell[i] = (uint16_t)c;
      });
  if (err) atomicOr(&ctl->err,err);
  __syncthreads();
  if (n <= 0) return;
  kc_store_cells(cell,prof+q0,n);
}

// ---------------------------------------------------------------------------------------------------------------------
// Relative labels (genome2class): every k-mer of a batch looked up in a table of ANOTHER sequence set, the count c
// turned into E (0, absent or a byte other than A C G T), H (1), D (2) or R (>= 3).  Semantics: include/classpro_amd.h,
// "Relative labels".  A block owns the KC_CELLS consecutive BASE positions [b0, b1), so its run of label characters is
// labels[b0..b1) and needs no search.  It fills an LDS stage with 'N', walks its positions (one lookup each) and
// overwrites the k-mer positions; then the whole block stores the stage.
//   characters  the stage is shifted by the destination's offset from a 16-byte boundary, so both the LDS reads and the
//               global stores of the middle are aligned 16-byte ones; head and tail go out byte by byte.
//   packed      four labels per byte counted from the start of each read (cp_pack_labels).  A byte belongs to the block
//               that holds its FIRST position (the rule of cp_threshold_labels: a group goes with its first position),
//               so every byte has one writer.  Such a byte may need up to three labels past b1: threads 0..2 look those
//               up themselves before the walk (they are tallied and profiled by the next block, not here).  Per read
//               of the block the bytes go out as 32-bit words between a byte-wise head and tail.
//   profile     the cell stage and store of kc_profile_kernel.
//   counts      tallied per lane, summed per wave, one atomic per wave and counter.
// The table is only read and ctl is not touched: an absent k-mer is the normal case here.

#define KC_STAGE (KC_CELLS+32)             // label stage: 15 bytes of shift, 3 positions past b1, rounded up

__device__ static inline unsigned kc_code(unsigned char c)                   // ctos: N, E -> 0, R -> 1, H -> 2, D -> 3
{ return c == 'R' ? 1u : c == 'H' ? 2u : c == 'D' ? 3u : 0u; }

template <bool PROF, bool LAB, bool PACK>
__global__ void __launch_bounds__(KT_BLOCK) kc_rel_kernel(const kc_slot *tab, unsigned long long mask, const char *seq,
                                                          const int64_t *seq_off, const int64_t *prof_off,
                                                          const int64_t *pack_off, int nreads, int64_t total, int K,
                                                          uint16_t *prof, char *labels, uint8_t *packed,
                                                          unsigned long long *counts)
{ constexpr bool STAGE = LAB || PACK;
  __shared__ uint16_t cell[PROF ? KC_CELLS : 1];
  __shared__ __attribute__((aligned(16))) unsigned char stage[STAGE ? KC_STAGE : 16];
  __shared__ int64_t run[2];
  const int64_t b0 = (int64_t)blockIdx.x*KC_CELLS, b1 = min(b0+(int64_t)KC_CELLS,total);
  const int shift = LAB ? (int)((uintptr_t)(labels+b0) & 15) : 0;
  if (PROF) kc_cell_run(seq_off,prof_off,nreads,total,K,b0,b1,run);
  if (STAGE)
    for (int i = threadIdx.x; i < KC_STAGE/4; i += KT_BLOCK) ((unsigned int *)stage)[i] = 0x4E4E4E4Eu;   // "NNNN"
  __syncthreads();
  int64_t q0 = 0, n = 0;
  if (PROF)
    { q0 = run[0];
      n = min(max(run[1]-q0,(int64_t)0),min((int64_t)KC_CELLS,prof_off[nreads]-q0));
    }
  auto label_of = [&](bool ok, unsigned long long hi, unsigned long long lo, unsigned long long *cnt) -> unsigned
    { unsigned long long c = 0;
      if (ok)
        { const kc_slot *e = kt_lookup(tab,mask,hi,lo);
          if (e) c = e->cnt;
        }
      *cnt = c;
      return (unsigned)min(c,3ull);                      // index in E, H, D, R
    };
  if (PACK && threadIdx.x < 3)                           // the labels past b1 that a byte begun before b1 holds
    { const int64_t j = b1+threadIdx.x;
      int lo_r = 0, hi_r = nreads;                       // the read holding b1-1
      while (hi_r-lo_r > 1)
        { const int mid = (lo_r+hi_r) >> 1;
          if (seq_off[mid] <= b1-1) lo_r = mid; else hi_r = mid;
        }
      const int64_t rs = seq_off[lo_r], re = seq_off[lo_r+1];
      if (j < re && j-rs >= K-1 && rs+((j-rs) & ~(int64_t)3) < b1)
        { const kt_u128 kmask = (((kt_u128)1) << (2*K))-1;
          kt_u128 fw = 0, rc = 0;
          bool ok = true;
          for (int64_t i = j-K+1; i <= j; i++)
            { const int b = kt_base((unsigned char)seq[i]);
              if (b < 0) { ok = false; break; }
              fw = ((fw << 2) | (kt_u128)b) & kmask;
              rc = (rc >> 2) | (((kt_u128)(3-b)) << (2*K-2));
            }
          const kt_u128 key = rc < fw ? rc : fw;
          unsigned long long c;
          const unsigned x = label_of(ok,(unsigned long long)(key >> 63),(unsigned long long)key & KT_M63,&c);
          stage[shift+(j-b0)] = (unsigned char)((0x52444845u >> (8*x)) & 0xffu);              // "EHDR"
        }
    }
  const int64_t p0 = b0+(int64_t)threadIdx.x*KT_CHUNK;
  unsigned int tally[4] = { 0, 0, 0, 0 };                // this lane's labels, order E, H, D, R
  int cur = -1;                                          // the read whose cell base is held
  int64_t base = 0;
  if (p0 < total)
    kt_walk_all<true>(seq,seq_off,nreads,total,K,p0,
      [&](int r, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
      { unsigned long long c;
        const unsigned x = label_of(ok,hi,lo,&c);
        tally[0] += x == 0; tally[1] += x == 1; tally[2] += x == 2; tally[3] += x == 3;
        if (STAGE) stage[shift+(j-b0)] = (unsigned char)((0x52444845u >> (8*x)) & 0xffu);
        if (PROF)
          { if (r != cur) { cur = r; base = prof_off[r]-seq_off[r]-(K-1)-q0; }
            const int64_t i = base+j;
            if ((unsigned long long)i < (unsigned long long)n)
              cell[i] = (uint16_t)min(c,(unsigned long long)CP_MAX_KMER_CNT);
          }
      });
  if (counts)
    for (int k = 0; k < 4; k++) kc_wave_add(counts+k,tally[k]);
  __syncthreads();
  if (PROF && n > 0) kc_store_cells(cell,prof+q0,n);
  if (LAB)
    { char *dst = labels+b0;
      const int64_t nb = b1-b0;
      const int64_t head = min(nb,(int64_t)((16-shift) & 15));
      const int64_t nvec = (nb-head) >> 4, tail = head+16*nvec;
      if ((int64_t)threadIdx.x < head) dst[threadIdx.x] = (char)stage[shift+threadIdx.x];
      for (int64_t i = threadIdx.x; i < nvec; i += KT_BLOCK)
        *(uint4 *)(dst+head+16*i) = *(const uint4 *)(stage+shift+head+16*i);
      if ((int64_t)threadIdx.x < nb-tail) dst[tail+threadIdx.x] = (char)stage[shift+tail+threadIdx.x];
    }
  if (PACK)
    { int r = 0, hi_r = nreads;                          // the read holding b0
      while (hi_r-r > 1)
        { const int mid = (r+hi_r) >> 1;
          if (seq_off[mid] <= b0) r = mid; else hi_r = mid;
        }
      for (; r < nreads; r++)
        { const int64_t rs = seq_off[r], re = seq_off[r+1];
          if (rs >= b1) break;
          const int64_t i0 = (max(rs,b0)-rs+3) >> 2, i1 = (min(re,b1)-rs+3) >> 2;   // bytes whose first position is ours
          if (i0 >= i1) continue;
          const int64_t s0 = shift+(rs-b0);              // label of read position l: stage[s0+l] (only l >= 4*i0 is read)
          const int64_t rlen = re-rs;
          auto byte_at = [&](int64_t i) -> unsigned
            { const int64_t l = 4*i;
              unsigned b = 0;
#pragma unroll
              for (int q = 0; q < 4; q++)
                if (l+q < rlen) b |= kc_code(stage[s0+l+q]) << (6-2*q);
              return b;
            };
          uint8_t *dst = packed+pack_off[r]+i0;
          const int64_t nb = i1-i0;
          const int64_t head = min(nb,(int64_t)((4-((uintptr_t)dst & 3)) & 3));
          const int64_t nw = (nb-head) >> 2, tail = head+4*nw;
          if ((int64_t)threadIdx.x < head) dst[threadIdx.x] = (uint8_t)byte_at(i0+threadIdx.x);
          for (int64_t w = threadIdx.x; w < nw; w += KT_BLOCK)
            { const int64_t i = i0+head+4*w;
              *(unsigned int *)(dst+head+4*w) = byte_at(i) | (byte_at(i+1) << 8) | (byte_at(i+2) << 16) | (byte_at(i+3) << 24);
            }
          if ((int64_t)threadIdx.x < nb-tail) dst[tail+threadIdx.x] = (uint8_t)byte_at(i0+tail+threadIdx.x);
        }
    }
}

// hist[c-1] += distinct keys with count c (c < 32767), hist[32766] += those with >= 32767, hist[32767] += the
// occurrences of the latter (ihighcnt)
__global__ void __launch_bounds__(KT_BLOCK) kc_hist_kernel(const kc_slot *tab, unsigned long long n,
                                                           unsigned long long *hist)
{ __shared__ unsigned int low[KC_LOW_BINS];
  for (int i = threadIdx.x; i < KC_LOW_BINS; i += KT_BLOCK) low[i] = 0;
  __syncthreads();
  for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < n;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const kc_slot e = tab[s];
      if (e.lo == KT_EMPTY || e.cnt == 0) continue;
      if (e.cnt <= KC_LOW_BINS) atomicAdd(&low[e.cnt-1],1u);
      else if (e.cnt < CP_MAX_KMER_CNT) atomicAdd(&hist[e.cnt-1],1ull);
      else
        { atomicAdd(&hist[CP_MAX_KMER_CNT-1],1ull);
          atomicAdd(&hist[CP_MAX_KMER_CNT],e.cnt);
        }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < KC_LOW_BINS; i += KT_BLOCK)
    if (low[i]) atomicAdd(&hist[i],(unsigned long long)low[i]);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct cp_kmer_counts : kt_store<kc_slot,kc_ctl>
  { bool unsized;                        // created with initial_slots = 0 and nothing added yet: the first add sizes it
    unsigned long long *filter;          // a filtered table's bit array (device); null: no filter
    unsigned long long filter_words;     // a power of two
    bool added;                          // a filtered table has seen its first add: its keys are fixed, no mark any more
  };

static int kc_create(const char *who, int K, int64_t initial_slots, int64_t filter_bits, cp_kmer_counts **out)
{ const std::string w(who);
  if (!out) return set_err(CP_EINVAL,w+": null out");
  *out = nullptr;
  if (K < 2 || K > 63)
    return set_err(CP_EINVAL,w+": K must lie in [2, 63] (a key holds 2K <= 126 bits)");
  if (initial_slots < 0 || initial_slots > ((int64_t)1 << 40))
    return set_err(CP_EINVAL,w+": bad initial_slots");
  cp_kmer_counts *t = new (std::nothrow) cp_kmer_counts();
  if (!t) return set_err(CP_ENOMEM,w+": out of memory");
  t->unsized = initial_slots == 0;
  int rc = kt_init(t,"cp_kmer_counts",K,initial_slots);
  if (rc == CP_OK && filter_bits > 0)
    { t->filter_words = kt_pow2_at_least((unsigned long long)filter_bits)/64;
      hipError_t e = hipMalloc(&t->filter,(size_t)t->filter_words*8);
      if (e == hipSuccess) e = hipMemset(t->filter,0,(size_t)t->filter_words*8);
      if (e == hipSuccess) e = hipStreamSynchronize(nullptr);          // the fill is on the null stream; the first mark need not be
      if (e != hipSuccess)
        { (void)hipGetLastError();
          char m[160];
          snprintf(m,sizeof(m),"%s: the filter of %llu bytes: %s",who,t->filter_words*8,hipGetErrorString(e));
          rc = set_err(CP_ENOMEM,m);
        }
    }
  if (rc != CP_OK)
    { cp_kmer_counts_destroy(t);
      return rc;
    }
  *out = t;
  return CP_OK;
}

extern "C" int cp_kmer_counts_create(int K, int64_t initial_slots, cp_kmer_counts **out)
{ return kc_create("cp_kmer_counts_create",K,initial_slots,0,out); }

extern "C" int cp_kmer_counts_create_filtered(int K, int64_t initial_slots, int64_t filter_bits, cp_kmer_counts **out)
{ if (out) *out = nullptr;
  if (filter_bits < 64 || filter_bits > ((int64_t)1 << 40))
    return set_err(CP_EINVAL,"cp_kmer_counts_create_filtered: filter_bits must lie in [64, 2^40]");
  return kc_create("cp_kmer_counts_create_filtered",K,initial_slots,filter_bits,out);
}

extern "C" void cp_kmer_counts_destroy(cp_kmer_counts *t)
{ if (!t) return;
  kt_free(t);
  if (t->filter) (void)hipFree(t->filter);
  delete t;
}

extern "C" int cp_kmer_counts_add(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                                  int64_t total_bases, void *stream)
{ if (!t || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_counts_add: bad argument");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off) return set_err(CP_EINVAL,"cp_kmer_counts_add: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = (int)((total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS);
  if (t->filter)                                           // the count pass: the keys are fixed, nothing to read back
    { t->stream = st;
      t->added = true;
      kc_count_kernel<<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,nreads,total_bases,t->K,t->ctl);
      HIPCHK(hipGetLastError());
      return CP_OK;
    }
  return kt_add(t,total_bases,st,&t->unsized,[&](bool replay, const unsigned int *fail_in, unsigned int *fail_out)
    { if (replay)
        kc_add_kernel<true><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,nreads,total_bases,t->K,fail_in,
                                                    fail_out,t->ctl);
      else
        kc_add_kernel<false><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,nreads,total_bases,t->K,fail_in,
                                                     fail_out,t->ctl);
    });
}

extern "C" int cp_kmer_counts_add_keys(cp_kmer_counts *t, const uint64_t *d_hi, const uint64_t *d_lo, int64_t n, void *stream)
{ const char *who = "cp_kmer_counts_add_keys";
  if (!t || n < 0) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (t->filter) return set_err(CP_EINVAL,std::string(who)+": a filtered table takes its keys from marked batches only");
  if (n == 0) return CP_OK;
  if (!d_lo) return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = kt_grid((unsigned long long)n);
  const unsigned long long *khi = (const unsigned long long *)d_hi, *klo = (const unsigned long long *)d_lo;
  HIPCHK(hipMemsetAsync(&t->ctl->n_badkey,0,sizeof(unsigned long long),st));
  const int rc = kt_add(t,n,st,&t->unsized,[&](bool replay, const unsigned int *fail_in, unsigned int *fail_out)
    { if (replay) kc_add_keys_kernel<true><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,khi,klo,n,t->K,fail_in,fail_out,t->ctl);
      else kc_add_keys_kernel<false><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,khi,klo,n,t->K,fail_in,fail_out,t->ctl);
    });
  if (rc != CP_OK) return rc;
  if (t->h_ctl->n_badkey)                                  // kt_add has read the control block back
    { char m[200];
      snprintf(m,sizeof(m),"%s: %llu of the %lld keys are no keys of %d bases (they were left out, the others added)",who,
               t->h_ctl->n_badkey,(long long)n,t->K);
      return set_err(CP_EINVAL,m);
    }
  return CP_OK;
}

extern "C" int cp_kmer_counts_mark(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                                   int64_t total_bases, void *stream)
{ if (!t || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_counts_mark: bad argument");
  if (!t->filter) return set_err(CP_EINVAL,"cp_kmer_counts_mark: the table has no filter");
  if (t->added)
    return set_err(CP_EINVAL,"cp_kmer_counts_mark: the table has been added to; every batch is marked before the first add");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off) return set_err(CP_EINVAL,"cp_kmer_counts_mark: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = (int)((total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS);
  if (t->unsized)                                          // the first-batch sizing of a filtered table: see the header
    { t->unsized = false;
      const int rc = kt_presize(t,kt_pow2_at_least((unsigned long long)total_bases/2),st);
      if (rc != CP_OK) return rc;
    }
  const unsigned long long wmask = t->filter_words-1;
  return kt_add(t,total_bases,st,(bool *)nullptr,[&](bool replay, const unsigned int *fail_in, unsigned int *fail_out)
    { if (replay)
        kc_mark_kernel<true><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,t->filter,wmask,d_seq,d_seq_off,nreads,total_bases,
                                                     t->K,fail_in,fail_out,t->ctl);
      else
        kc_mark_kernel<false><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,t->filter,wmask,d_seq,d_seq_off,nreads,total_bases,
                                                      t->K,fail_in,fail_out,t->ctl);
    },false);
}

extern "C" int cp_kmer_counts_profiles(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off,
                                       const int64_t *d_prof_off, int nreads, int64_t total_bases, uint16_t *d_prof,
                                       void *stream)
{ if (!t || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_counts_profiles: bad argument");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off || !d_prof_off || !d_prof)
    return set_err(CP_EINVAL,"cp_kmer_counts_profiles: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  t->stream = st;
  const int grid = (int)((total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS);
  if (t->filter)
    kc_profile_kernel<true><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,d_prof_off,nreads,total_bases,t->K,
                                                    d_prof,t->ctl);
  else
    kc_profile_kernel<false><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,d_prof_off,nreads,total_bases,t->K,
                                                     d_prof,t->ctl);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

extern "C" int cp_kmer_counts_rel_labels(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                                         int64_t total_bases, uint16_t *d_prof, const int64_t *d_prof_off,
                                         char *d_labels, uint8_t *d_packed, const int64_t *d_pack_off,
                                         int64_t *d_counts, void *stream)
{ if (!t || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_counts_rel_labels: bad argument");
  if (!d_prof != !d_prof_off) return set_err(CP_EINVAL,"cp_kmer_counts_rel_labels: d_prof and d_prof_off go together");
  if (!d_packed != !d_pack_off)
    return set_err(CP_EINVAL,"cp_kmer_counts_rel_labels: d_packed and d_pack_off go together");
  if (!d_prof && !d_labels && !d_packed && !d_counts)
    return set_err(CP_EINVAL,"cp_kmer_counts_rel_labels: no output wanted");
  if (t->filter)
    return set_err(CP_EINVAL,"cp_kmer_counts_rel_labels: a filtered table cannot tell a count of 0 from a count of 1");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off) return set_err(CP_EINVAL,"cp_kmer_counts_rel_labels: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  t->stream = st;
  const int grid = (int)((total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS);
  unsigned long long *cnt = (unsigned long long *)d_counts;
#define KC_REL(P,L,B) kc_rel_kernel<P,L,B><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,d_prof_off,d_pack_off, \
                                                                   nreads,total_bases,t->K,d_prof,d_labels,d_packed,cnt)
  switch ((d_prof ? 4 : 0) | (d_labels ? 2 : 0) | (d_packed ? 1 : 0))
    { case 0: KC_REL(false,false,false); break;
      case 1: KC_REL(false,false,true); break;
      case 2: KC_REL(false,true,false); break;
      case 3: KC_REL(false,true,true); break;
      case 4: KC_REL(true,false,false); break;
      case 5: KC_REL(true,false,true); break;
      case 6: KC_REL(true,true,false); break;
      default: KC_REL(true,true,true); break;
    }
#undef KC_REL
  HIPCHK(hipGetLastError());
  return CP_OK;
}

// reads the control block back; on a filtered table whose marked and added batches differ CP_EINVAL in the name of `who`
static int kc_sync_checked(cp_kmer_counts *t, const char *who)
{ const int rc = kt_sync_ctl(t,t->stream);
  if (rc != CP_OK) return rc;
  const unsigned long long marked = t->h_ctl->n_mark, counted = t->h_ctl->n_add+t->h_ctl->n_single;
  if (t->filter && marked != counted)
    { char m[200];
      snprintf(m,sizeof(m),"%s: %llu k-mers were marked and %llu added: the marked and the added batches differ",who,marked,
               counted);
      return set_err(CP_EINVAL,m);
    }
  return CP_OK;
}

// the slot sweep of the histogram into h[0..CP_MAX_KMER_CNT]; synchronises
static int kc_sweep(cp_kmer_counts *t, std::vector<unsigned long long> &h)
{ hipStream_t st = t->stream;
  const size_t bytes = sizeof(unsigned long long)*(CP_MAX_KMER_CNT+1);
  unsigned long long *d_hist = nullptr;
  if (hipMalloc(&d_hist,bytes) != hipSuccess)
    { (void)hipGetLastError();
      return set_err(CP_ENOMEM,"cp_kmer_counts_hist: cannot allocate the device histogram");
    }
  h.resize((size_t)CP_MAX_KMER_CNT+1);
  hipError_t e = hipMemsetAsync(d_hist,0,bytes,st);
  if (e == hipSuccess)
    { kc_hist_kernel<<<kt_grid(t->slots),KT_BLOCK,0,st>>>(t->tab,t->slots,d_hist);
      e = hipGetLastError();
    }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(),d_hist,bytes,hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_hist);
  if (e != hipSuccess) return set_err(CP_EHIP,std::string("cp_kmer_counts_hist: ")+hipGetErrorString(e));
  return CP_OK;
}

extern "C" int cp_kmer_counts_hist(cp_kmer_counts *t, int64_t *hist, int64_t *ilowcnt, int64_t *ihighcnt)
{ if (!t || !hist || !ilowcnt || !ihighcnt) return set_err(CP_EINVAL,"cp_kmer_counts_hist: bad argument");
  std::vector<unsigned long long> h;
  int rc;
  if (t->filter)
    { rc = kc_sync_checked(t,"cp_kmer_counts_hist");
      if (rc != CP_OK) return rc;
    }
  rc = kc_sweep(t,h);
  if (rc != CP_OK) return rc;
  if (t->filter) h[0] += t->h_ctl->n_single;               // the keys kept outside: each occurs once
  for (int c = 0; c < CP_MAX_KMER_CNT; c++) hist[c] = (int64_t)h[(size_t)c];
  *ilowcnt = (int64_t)h[0];
  *ihighcnt = (int64_t)h[(size_t)CP_MAX_KMER_CNT];
  return CP_OK;
}

extern "C" int cp_kmer_counts_stats(cp_kmer_counts *t, cp_kmer_count_stats *out)
{ if (!t || !out) return set_err(CP_EINVAL,"cp_kmer_counts_stats: bad argument");
  hipStream_t st = t->stream;
  int rc = kc_sync_checked(t,"cp_kmer_counts_stats");
  if (rc != CP_OK) return rc;
  if (t->h_ctl->err)                                       // deferred device errors: reported once, then cleared
    { HIPCHK(hipMemsetAsync(&t->ctl->err,0,sizeof(unsigned int),st));
      HIPCHK(hipStreamSynchronize(st));
      return set_err(CP_EINVAL,"cp_kmer_counts: a profile pass met a k-mer that was never added (its cell is 0)");
    }
  out->n_kmers = (int64_t)(t->h_ctl->n_add+t->h_ctl->n_single);          // n_single is 0 without a filter
  out->n_skipped = (int64_t)t->h_ctl->n_skip;
  out->n_distinct = (int64_t)(t->h_ctl->n_occ+t->h_ctl->n_single);
  out->slots = (int64_t)t->slots;
  out->bytes = (int64_t)(t->slots*sizeof(kc_slot)+2*t->fail_words*4+t->filter_words*8);
  out->growths = t->growths;
  return CP_OK;
}

extern "C" int cp_kmer_counts_filter_stats(cp_kmer_counts *t, cp_kmer_filter_stats *out)
{ if (!t || !out) return set_err(CP_EINVAL,"cp_kmer_counts_filter_stats: bad argument");
  int rc = kt_sync_ctl(t,t->stream);
  if (rc != CP_OK) return rc;
  std::vector<unsigned long long> h;
  rc = kc_sweep(t,h);
  if (rc != CP_OK) return rc;
  out->filter_bits = (int64_t)(t->filter_words*64);
  out->filter_bytes = (int64_t)(t->filter_words*8);
  out->n_marked = (int64_t)t->h_ctl->n_mark;
  out->n_counted = (int64_t)(t->h_ctl->n_add+t->h_ctl->n_single);
  out->n_table_keys = (int64_t)t->h_ctl->n_occ;
  out->n_outside = (int64_t)t->h_ctl->n_single;
  out->n_false = (int64_t)h[0];
  return CP_OK;
}

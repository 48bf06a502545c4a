// kmer_runs.hip -- the states of the k-mer positions of a batch, looked up in one or two sorted snapshots, reduced to RUNS
// on the device (tabtrack): only the runs come down, never a value per base.  Semantics: include/classpro_amd.h, "Runs of
// k-mer states along reads"; design: DESIGN.md 9.18; the summary algebra: kr_sum.h.  Included by capi.hip after
// kmer_hits.hip (the snapshot, kl_view, kl_find_group, kh_range, KC_CELLS, set_err and HIPCHK are in scope).  Both
// snapshots are only read.
//   states   kr_state_kernel has the lane and block shape of kh_hits_kernel: a lane rolls the keys of its KT_CHUNK positions
//            once (kt_walk_all) and looks each up once per table.  The state goes into one byte per base of the batch
//            (KR_NOKMER where no k-mer ends, KR_FIRST set on the first k-mer position of a read), staged in LDS and stored
//            as whole vectors, and into the lane's summary; the block joins its lanes' summaries into one.
//   scan     kr_scan_kernel, one block: the summaries of all blocks joined in order, each block's replaced by the join
//            of everything before it.  That one begins with a reset, so it holds the run under way at the block's first
//            position (state, last counting position, n so far) and the number of records before it: exact offsets.
//   write    kr_write_kernel reads only the state bytes.  A lane summarises its 64 bytes, the block scans the summaries,
//            and the lane walks its bytes again knowing the run under way and the record index.  A head stores
//            read/state/first of its own record and last/n of the run before it in its read; the first k-mer position of a
//            read closes the last run of the read before, the batch's last position closes the last run of all.  So work
//            is forward only.  The same lanes store d_run_off: the first k-mer position of read r knows the number of
//            records before it, and hands it down to the reads without a k-mer position that precede it.
//   split    a build with KR_SPLIT 1: kr_state_kernel leaves the summaries out and kr_sum_kernel makes them from the state
//            bytes.  Measured slower in every sample, so it is compiled out.
// Every record field is stored exactly once and nothing is added to in memory, so the records are a function of the read,
// the snapshots, the ranges and the masks alone.
#include "kr_sum.h"

#define KR_SPLIT 0                         // 1: the block summaries by a kernel of their own over the state bytes

__device__ static inline kr_sum kr_shfl_up(const kr_sum &a, int d)
{ kr_sum o;
  o.p = __shfl_up(a.p,d); o.n = __shfl_up(a.n,d); o.heads = __shfl_up(a.heads,d); o.flags = __shfl_up(a.flags,d);
  o.pad = 0;
  return o;
}

// inclusive scan over the lanes of a wave, in lane order
__device__ static inline kr_sum kr_wave_scan(kr_sum v, int lane, unsigned int emit)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    { const kr_sum u = kr_shfl_up(v,d);
      if (lane >= d) v = kr_join(u,v,emit);
    }
  return v;
}

template <bool CANON, bool LO_A, bool LO_B, bool HAS_B>
__global__ void __launch_bounds__(KT_BLOCK) kr_state_kernel(kl_view ta, kl_view tb, kh_range rg, unsigned int skip,
                                                            unsigned int emit, const char *seq, const int64_t *seq_off,
                                                            int nreads, int64_t total, int K, uint8_t *state, kr_sum *part)
{ constexpr bool SUM = KR_SPLIT == 0;                      // the block's summary is made here
  __shared__ __attribute__((aligned(16))) uint8_t cell[KC_CELLS];
  __shared__ kr_sum wave_v[KT_BLOCK/64];
  const int64_t b0 = (int64_t)blockIdx.x*KC_CELLS, b1 = min(b0+(int64_t)KC_CELLS,total);
  const int64_t p0 = b0+(int64_t)threadIdx.x*KT_CHUNK;
  for (int i = threadIdx.x; i < KC_CELLS/4; i += KT_BLOCK) ((unsigned int *)cell)[i] = KR_NOKMER*0x01010101u;
  __syncthreads();
  kr_sum sum{ 0, 0, 0, 0, 0 };
  int cur = -1;
  int64_t first_j = 0;                                     // the first k-mer position of the read under way
  if (p0 < total)
    kt_walk_all<CANON>(seq,seq_off,nreads,total,K,p0,
      [&](int r, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
      { if (r != cur) { cur = r; first_j = seq_off[r]+(K-1); }
        unsigned int s = CP_RUN_OTHER;
        if (ok)
          { const unsigned long long qh[1] = { hi }, ql[1] = { lo };
            int64_t pa[1], pb[1] = { -1 };
            kl_find_group<LO_A,KL_INTERP != 0,1>(ta,qh,ql,1,pa);
            if (HAS_B) kl_find_group<LO_B,KL_INTERP != 0,1>(tb,qh,ql,1,pb);
            const unsigned long long ca = pa[0] >= 0 ? ta.cnt[pa[0]] : 0;
            const unsigned long long cb = (HAS_B && pb[0] >= 0) ? tb.cnt[pb[0]] : 0;
            const bool in_a = pa[0] >= 0 && ca >= rg.amin && ca <= rg.amax;
            const bool in_b = HAS_B && pb[0] >= 0 && cb >= rg.bmin && cb <= rg.bmax;
            s = (in_a ? CP_RUN_A : 0u) | (in_b ? CP_RUN_B : 0u);
          }
        const bool first = j == first_j;
        const int64_t i = j-b0;
        if ((unsigned long long)i < (unsigned long long)KC_CELLS) cell[i] = (uint8_t)(s | (first ? KR_FIRST : 0u));
        if (SUM) kr_push(sum,first,s,j,skip,emit);
      });
  // ---- the block: its lanes' summaries joined in order ----
  if (SUM)
    { const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      const kr_sum inc = kr_wave_scan(sum,lane,emit);
      if (lane == 63) wave_v[wave] = inc;
    }
  __syncthreads();                                         // also: every cell is written
  if (SUM && threadIdx.x == 0)
    { kr_sum all = wave_v[0];
      for (int w = 1; w < KT_BLOCK/64; w++) all = kr_join(all,wave_v[w],emit);
      part[blockIdx.x] = all;
    }
  // ---- the state bytes of [b0, b1): whole 16-byte vectors, then the few bytes that are left ----
  const int nb = (int)(b1-b0), nvec = nb >> 4;
  uint8_t *out = state+b0;                                 // 16-byte aligned: the allocation is, and b0 is a multiple of 16
  for (int i = threadIdx.x; i < nvec; i += KT_BLOCK) ((uint4 *)out)[i] = ((const uint4 *)cell)[i];
  for (int i = 16*nvec+threadIdx.x; i < nb; i += KT_BLOCK) out[i] = cell[i];
}

// part[b] = the join of a reset and part[0 .. b-1]; part[nblk] = the join of all.  One block.
__global__ void __launch_bounds__(KT_BLOCK) kr_scan_kernel(kr_sum *part, int64_t nblk, unsigned int emit)
{ __shared__ kr_sum share[KT_BLOCK];
  const int64_t per = (nblk+KT_BLOCK-1)/KT_BLOCK;
  const int64_t i0 = min(nblk,(int64_t)threadIdx.x*per), i1 = min(nblk,i0+per);
  kr_sum acc{ 0, 0, 0, 0, 0 };
  for (int64_t i = i0; i < i1; i++) acc = kr_join(acc,part[i],emit);
  share[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    { kr_sum run{ 0, 0, 0, KR_RESET, 0 };
      for (int t = 0; t < KT_BLOCK; t++)
        { const kr_sum mine = share[t];
          share[t] = run;
          run = kr_join(run,mine,emit);
        }
      part[nblk] = run;
    }
  __syncthreads();
  acc = share[threadIdx.x];
  for (int64_t i = i0; i < i1; i++)
    { const kr_sum mine = part[i];
      part[i] = acc;
      acc = kr_join(acc,mine,emit);
    }
}

// the state bytes of the lane's np positions from p0 into w, eight to a word (KR_NOKMER past the batch's end), and their
// summary.  A word is taken apart by shifting, eight steps that are not unrolled: the walks stay small.
__device__ static inline kr_sum kr_lane_sum(const uint8_t *state, int64_t p0, int np, unsigned long long (&w)[KT_CHUNK/8],
                                            unsigned int skip, unsigned int emit)
{ if (np == KT_CHUNK)
    {
#pragma unroll
      for (int k = 0; k < KT_CHUNK/16; k++)
        { const uint4 v = ((const uint4 *)(state+p0))[k];
          w[2*k] = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
          w[2*k+1] = (unsigned long long)v.z | ((unsigned long long)v.w << 32);
        }
    }
  else
    {
#pragma unroll
      for (int k = 0; k < KT_CHUNK/8; k++)
        { unsigned long long v = 0;
          for (int c = 7; c >= 0; c--) v = (v << 8) | (unsigned long long)(8*k+c < np ? state[p0+8*k+c] : (uint8_t)KR_NOKMER);
          w[k] = v;
        }
    }
  kr_sum sum{ 0, 0, 0, 0, 0 };
#pragma unroll
  for (int k = 0; k < KT_CHUNK/8; k++)
    { unsigned long long v = w[k];
#pragma unroll 1
      for (int c = 0; c < 8; c++, v >>= 8)
        { const unsigned int b = (unsigned int)v & 0xffu;
          kr_push(sum,(b & KR_FIRST) != 0,b & 7u,p0+8*k+c,skip,emit);
        }
    }
  return sum;
}

#if KR_SPLIT
// the split form: the summary of block b from its state bytes, when kr_state_kernel has left it out
__global__ void __launch_bounds__(KT_BLOCK) kr_sum_kernel(const uint8_t *state, unsigned int skip, unsigned int emit,
                                                          int64_t total, kr_sum *part)
{ __shared__ kr_sum wave_v[KT_BLOCK/64];
  const int64_t p0 = (int64_t)blockIdx.x*KC_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  const int np = (int)min(max(total-p0,(int64_t)0),(int64_t)KT_CHUNK);
  unsigned long long w[KT_CHUNK/8];
  const kr_sum sum = kr_lane_sum(state,p0,np,w,skip,emit);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const kr_sum inc = kr_wave_scan(sum,lane,emit);
  if (lane == 63) wave_v[wave] = inc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  kr_sum all = wave_v[0];
  for (int v = 1; v < KT_BLOCK/64; v++) all = kr_join(all,wave_v[v],emit);
  part[blockIdx.x] = all;
}
#endif

__global__ void __launch_bounds__(KT_BLOCK) kr_write_kernel(const uint8_t *state, const kr_sum *part, unsigned int skip,
                                                            unsigned int emit, const int64_t *seq_off, int nreads,
                                                            int64_t total, int K, kr_rec *runs, int64_t capacity,
                                                            int64_t *run_off)
{ __shared__ kr_sum wave_v[KT_BLOCK/64];
  const int64_t p0 = (int64_t)blockIdx.x*KC_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  const int np = (int)min(max(total-p0,(int64_t)0),(int64_t)KT_CHUNK);
  unsigned long long w[KT_CHUNK/8];
  const kr_sum sum = kr_lane_sum(state,p0,np,w,skip,emit);
  // ---- the block: what reaches this lane = the block's carry, the waves before, the lanes before ----
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const kr_sum inc = kr_wave_scan(sum,lane,emit);
  kr_sum exc = kr_shfl_up(inc,1);
  if (lane == 0) exc = kr_sum{ 0, 0, 0, 0, 0 };
  if (lane == 63) wave_v[wave] = inc;
  __syncthreads();
  kr_sum in = part[blockIdx.x];
  for (int v = 0; v < wave; v++) in = kr_join(in,wave_v[v],emit);
  in = kr_join(in,exc,emit);
  if (np <= 0) return;
  // ---- the lane again, now with the run under way and the number of records so far (kr_sum.h) ----
  kr_walk x = kr_walk_begin(in,seq_off,nreads,p0);
#pragma unroll
  for (int k = 0; k < KT_CHUNK/8; k++)
    { unsigned long long v = w[k];
#pragma unroll 1
      for (int c = 0; c < 8; c++, v >>= 8)
        kr_walk_step(x,(unsigned int)v & 0xffu,p0+8*k+c,skip,emit,seq_off,nreads,K,runs,capacity,run_off);
    }
  if (p0+np == total) kr_walk_end(x,emit,seq_off,nreads,K,runs,capacity,run_off);      // the batch ends in this lane
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

extern "C" int cp_kmer_sorted_read_runs(const cp_kmer_sorted *a, const cp_kmer_sorted *b, int canonical,
                                        const int64_t *range, unsigned int skip, unsigned int emit, const char *d_seq,
                                        const int64_t *d_seq_off, int nreads, int64_t total_bases, cp_kmer_run *d_runs,
                                        int64_t capacity, int64_t *d_run_off, int64_t *total, void *stream)
{ const char *who = "cp_kmer_sorted_read_runs";
  static_assert(sizeof(cp_kmer_run) == sizeof(kr_rec) && sizeof(kr_rec) == 32,"a run is 32 bytes");
  if (!a || !total || nreads < 0 || total_bases < 0 || capacity < 0) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!a->ready || (b && !b->ready)) return set_err(CP_EINVAL,std::string(who)+": a snapshot is still being loaded");
  if (b && a->K != b->K)
    { char m[120];
      snprintf(m,sizeof(m),"%s: the snapshots hold %d-mers and %d-mers",who,a->K,b->K);
      return set_err(CP_EINVAL,m);
    }
  kh_range rg{ 1, (unsigned long long)INT64_MAX, 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0] || range[2] < 1 || range[3] < range[2])
        return set_err(CP_EINVAL,std::string(who)+": a count range needs 1 <= min <= max");
      rg.amin = (unsigned long long)range[0]; rg.amax = (unsigned long long)range[1];
      rg.bmin = (unsigned long long)range[2]; rg.bmax = (unsigned long long)range[3];
    }
  if (skip > 0x1fu || emit > 0x1fu || emit == 0 || (emit & skip) != 0)
    return set_err(CP_EINVAL,std::string(who)+": skip and emit are disjoint masks of the five states, emit not empty");
  if ((capacity > 0 && !d_runs) || (nreads > 0 && (!d_run_off || !d_seq_off)) || (total_bases > 0 && !d_seq))
    return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  const int64_t nblk = nreads > 0 ? (total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS : 0;
  if (nblk > 0x3fffffff) return set_err(CP_EINVAL,std::string(who)+": the batch is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  // one allocation, before anything is queued: the block summaries and the sum of all, then a state byte per base
  const size_t nsum = ((size_t)nblk+1)*sizeof(kr_sum), bytes = nsum+(size_t)total_bases;
  uint8_t *scratch = nullptr;
  if (nblk > 0 && (hipMallocAsync((void **)&scratch,bytes,st) != hipSuccess || !scratch))
    { (void)hipGetLastError();
      char m[160];
      snprintf(m,sizeof(m),"%s: cannot allocate %zu bytes for the states and the block summaries",who,bytes);
      return set_err(CP_ENOMEM,m);
    }
  *total = 0;
  if (d_run_off)
    { const hipError_t e0 = hipMemsetAsync(d_run_off,0,((size_t)nreads+1)*sizeof(int64_t),st);
      if (e0 != hipSuccess)
        { if (scratch) (void)hipFreeAsync(scratch,st);
          (void)hipStreamSynchronize(st);
          return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e0));
        }
    }
  if (nblk == 0)
    { HIPCHK(hipStreamSynchronize(st));
      return CP_OK;
    }
  kr_sum *part = (kr_sum *)scratch;
  uint8_t *state = scratch+nsum;                           // nsum is a multiple of 32
  const kl_view ta = kl_view_of(a), tb = b ? kl_view_of(b) : kl_view_of(a);
#define KR_RUN(C,LA,LB,HB) kr_state_kernel<C,LA,LB,HB><<<(unsigned)nblk,KT_BLOCK,0,st>>>(ta,tb,rg,skip,emit,d_seq,d_seq_off, \
                                                                                       nreads,total_bases,a->K,state,part)
#define KR_RUN_T(C) do { if (!b) { if (kl_lo_only(a)) KR_RUN(C,true,true,false); else KR_RUN(C,false,false,false); } \
                         else if (kl_lo_only(a)) { if (kl_lo_only(b)) KR_RUN(C,true,true,true); else KR_RUN(C,true,false,true); } \
                         else { if (kl_lo_only(b)) KR_RUN(C,false,true,true); else KR_RUN(C,false,false,true); } } while (0)
  if (canonical) KR_RUN_T(true); else KR_RUN_T(false);
#undef KR_RUN_T
#undef KR_RUN
  hipError_t e = hipGetLastError();
#if KR_SPLIT
  if (e == hipSuccess)
    { kr_sum_kernel<<<(unsigned)nblk,KT_BLOCK,0,st>>>(state,skip,emit,total_bases,part);
      e = hipGetLastError();
    }
#endif
  if (e == hipSuccess)
    { kr_scan_kernel<<<1,KT_BLOCK,0,st>>>(part,nblk,emit);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    { kr_write_kernel<<<(unsigned)nblk,KT_BLOCK,0,st>>>(state,part,skip,emit,d_seq_off,nreads,total_bases,a->K,(kr_rec *)d_runs,
                                                       capacity,d_run_off);
      e = hipGetLastError();
    }
  int64_t n = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&n,&part[nblk].heads,sizeof(int64_t),hipMemcpyDeviceToHost,st);
  const hipError_t ef = hipFreeAsync(scratch,st);
  if (e == hipSuccess) e = ef;
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  *total = n;
  if (n > capacity)
    { char m[160];
      snprintf(m,sizeof(m),"%s: %lld runs do not fit the %lld of d_runs",who,(long long)n,(long long)capacity);
      return set_err(CP_EOVERFLOW,m);
    }
  return CP_OK;
}

extern "C" int64_t cp_run_blocks(const cp_kmer_run *runs, int64_t nruns, int64_t min_n, cp_kmer_run *blocks, int64_t *dropped)
{ if (!runs || !blocks || !dropped || min_n < 1 || nruns < 0) return set_err(CP_EINVAL,"cp_run_blocks: bad argument");
  int64_t nb = 0, nd = 0;
  for (int64_t i = 0; i < nruns; i++)
    { const cp_kmer_run x = runs[i];                       // blocks may be runs: a block is written behind what was read
      if (x.n < min_n) { nd++; continue; }
      if (nb > 0 && blocks[nb-1].state == x.state)
        { blocks[nb-1].last = x.last;
          blocks[nb-1].n += x.n;
        }
      else blocks[nb++] = x;
    }
  *dropped = nd;
  return nb;
}

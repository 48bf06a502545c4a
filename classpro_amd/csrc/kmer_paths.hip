// kmer_paths.hip -- the k-mer positions of a batch threaded through the unitig graph of ONE sorted snapshot (tabpath): per
// position the oriented unitig and the place of its k-mer, reduced on the device to SEGMENTS, with the read coverage of
// every unitig and the read support of every arc.  Semantics: include/classpro_amd.h, "Reads through the unitig graph";
// design: DESIGN.md 9.21; the words, the summary algebra and the walk: kp_sum.h.  Included by capi.hip after
// kmer_unitig_graph.hip (the snapshot, kl_view, kl_find_group, cp_unitigs, cp_unitig_graph, KC_CELLS, kc_wave_add, set_err
// and HIPCHK are in scope).  Everything passed in is only read, but d_cov and d_support.
//   steps    kp_step_kernel has the lane and block shape of kr_state_kernel: a lane rolls the keys of its KT_CHUNK positions
//            once (kt_walk_strand, which also says which strand won), makes ONE bounded search per valid key and, when the key
//            is found, loads d_utg and d_at of the entry together.  One 64-bit word per base goes straight to memory
//            (kp_sum.h: x << 32 | raw place, three words for absent, other byte and no k-mer, bit 63 on the first k-mer
//            position of a read).  Continuity is decided on the raw place, so the length of a unitig is loaded at heads only.
//   count    kp_count_kernel: a lane summarises its KT_CHUNK words and the word before them, the block joins its lanes.
//   scan     kp_scan_kernel, one block: every block's summary replaced by the join of everything before it; the join of all.
//   write    kp_write_kernel summarises again, scans inside the block and walks its words once more knowing the record
//            index and the last head (kp_walk_step).  Coverage and support are 64-bit atomic adds, made only when all
//            records fit d_segs, so that the second call after CP_EOVERFLOW does not add twice.
// Every record field is stored exactly once; the two sums are integer atomics: nothing depends on grid, batching or
// scheduling.
#include "kp_sum.h"

enum { KP_C_PRESENT = 0, KP_C_ABSENT = 1, KP_C_OTHER = 2, KP_C_PAD = 3 };       // the counters behind the summaries

template <bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) kp_step_kernel(kl_view t, const int64_t *utg, const int64_t *at, int64_t ucount,
                                                           const char *seq, const int64_t *seq_off, int nreads,
                                                           int64_t total, int K, unsigned long long *word,
                                                           unsigned long long *ctl)
{ const int64_t p0 = (int64_t)blockIdx.x*KC_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  const int64_t p1 = min(p0+(int64_t)KT_CHUNK,total);
  unsigned long long npres = 0, nabs = 0, noth = 0;
  int64_t next = p0;                                       // the first position of the chunk without a word yet
  int cur = -1;
  int64_t first_j = 0;
  if (p0 < total)
    kt_walk_strand(seq,seq_off,nreads,total,K,p0,
      [&](int r, int64_t j, bool ok, unsigned long long hi, unsigned long long lo, bool won)
      { if (r != cur) { cur = r; first_j = seq_off[r]+(K-1); }
        unsigned long long w = KP_OTHER;
        if (ok)
          { const unsigned long long qh[1] = { hi }, ql[1] = { lo };
            int64_t pos[1];
            kl_find_group<LO_ONLY,KL_INTERP != 0,1>(t,qh,ql,1,pos);
            w = KP_ABSENT;
            if (pos[0] >= 0 && ucount > 0)
              { const int64_t e = min(pos[0],t.n-1);
                const int64_t u = utg[e], a = at[e];       // the two loads together
                if (u >= 0)
                  { const unsigned long long x = 2ull*(unsigned long long)min(u,ucount-1)+(unsigned long long)((won ? 1 : 0) ^ (int)(a & 1));
                    w = (x << 32) | (((unsigned long long)a >> 1) & KP_KMASK);
                  }
              }
            npres += w != KP_ABSENT;
            nabs += w == KP_ABSENT;
          }
        else noth++;
        if (j == first_j) w |= KP_FIRST;
        if (j < p0 || j >= p1) return;                     // never: the walk stays in the chunk
        for (; next < j; next++) word[next] = KP_NOKMER;
        word[j] = w;
        next = j+1;
      });
  for (; next < p1; next++) word[next] = KP_NOKMER;
  kc_wave_add(ctl+KP_C_PRESENT,npres);
  kc_wave_add(ctl+KP_C_ABSENT,nabs);
  kc_wave_add(ctl+KP_C_OTHER,noth);
}

__device__ static inline kp_sum kp_shfl_up(const kp_sum &a, int d)
{ kp_sum o;
  o.heads = __shfl_up(a.heads,d); o.joined = __shfl_up(a.joined,d); o.last = __shfl_up(a.last,d);
  o.pad = 0;
  return o;
}

// inclusive scan over the lanes of a wave, in lane order
__device__ static inline kp_sum kp_wave_scan(kp_sum v, int lane)
{
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    { const kp_sum u = kp_shfl_up(v,d);
      if (lane >= d) v = kp_join(u,v);
    }
  return v;
}

// the summary of the np words from p0 on
__device__ static inline kp_sum kp_lane_sum(const unsigned long long *word, int64_t p0, int np)
{ kp_sum sum{ 0, 0, 0, 0 };
  if (np <= 0) return sum;
  unsigned long long pw = p0 > 0 ? word[p0-1] : KP_NOKMER;
  if (np == KT_CHUNK)
    {
#pragma unroll 4
      for (int k = 0; k < KT_CHUNK/2; k++)
        { const ulonglong2 v = ((const ulonglong2 *)(word+p0))[k];          // p0 is a multiple of KT_CHUNK
          kp_push(sum,pw,v.x,p0+2*k);
          kp_push(sum,v.x,v.y,p0+2*k+1);
          pw = v.y;
        }
    }
  else
    for (int k = 0; k < np; k++)
      { const unsigned long long w = word[p0+k];
        kp_push(sum,pw,w,p0+k);
        pw = w;
      }
  return sum;
}

__global__ void __launch_bounds__(KT_BLOCK) kp_count_kernel(const unsigned long long *word, int64_t total, kp_sum *part)
{ __shared__ kp_sum wave_v[KT_BLOCK/64];
  const int64_t p0 = (int64_t)blockIdx.x*KC_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  const int np = (int)min(max(total-p0,(int64_t)0),(int64_t)KT_CHUNK);
  const kp_sum sum = kp_lane_sum(word,p0,np);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const kp_sum inc = kp_wave_scan(sum,lane);
  if (lane == 63) wave_v[wave] = inc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  kp_sum all = wave_v[0];
  for (int v = 1; v < KT_BLOCK/64; v++) all = kp_join(all,wave_v[v]);
  part[blockIdx.x] = all;
}

// part[b] = the join of part[0 .. b-1]; part[nblk] = the join of all.  One block.
__global__ void __launch_bounds__(KT_BLOCK) kp_scan_kernel(kp_sum *part, int64_t nblk)
{ __shared__ kp_sum share[KT_BLOCK];
  const int64_t per = (nblk+KT_BLOCK-1)/KT_BLOCK;
  const int64_t i0 = min(nblk,(int64_t)threadIdx.x*per), i1 = min(nblk,i0+per);
  kp_sum acc{ 0, 0, 0, 0 };
  for (int64_t i = i0; i < i1; i++) acc = kp_join(acc,part[i]);
  share[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    { kp_sum run{ 0, 0, 0, 0 };
      for (int t = 0; t < KT_BLOCK; t++)
        { const kp_sum mine = share[t];
          share[t] = run;
          run = kp_join(run,mine);
        }
      part[nblk] = run;
    }
  __syncthreads();
  acc = share[threadIdx.x];
  for (int64_t i = i0; i < i1; i++)
    { const kp_sum mine = part[i];
      part[i] = acc;
      acc = kp_join(acc,mine);
    }
}

__global__ void __launch_bounds__(KT_BLOCK) kp_write_kernel(const unsigned long long *word, const kp_sum *part, int64_t nblk,
                                                            int64_t total, kp_args a)
{ __shared__ kp_sum wave_v[KT_BLOCK/64];
  const int64_t p0 = (int64_t)blockIdx.x*KC_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  const int np = (int)min(max(total-p0,(int64_t)0),(int64_t)KT_CHUNK);
  const kp_sum sum = kp_lane_sum(word,p0,np);
  // ---- the block: what lies before this lane = the blocks before, the waves before, the lanes before ----
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const kp_sum inc = kp_wave_scan(sum,lane);
  kp_sum exc = kp_shfl_up(inc,1);
  if (lane == 0) exc = kp_sum{ 0, 0, 0, 0 };
  if (lane == 63) wave_v[wave] = inc;
  __syncthreads();
  kp_sum in = part[blockIdx.x];
  for (int v = 0; v < wave; v++) in = kp_join(in,wave_v[v]);
  in = kp_join(in,exc);
  if (np <= 0) return;
  if (part[nblk].heads > a.capacity) { a.cov = nullptr; a.support = nullptr; }     // the call will be made again
  // ---- the lane again, now with the record index and the last head ----
  kp_walk x = kp_walk_begin(in,a,p0);
  unsigned long long pw = p0 > 0 ? word[p0-1] : KP_NOKMER;
#pragma unroll 1
  for (int k = 0; k < np; k++)
    { const unsigned long long w = word[p0+k];
      kp_walk_step(x,pw,w,p0+k,a);
      pw = w;
    }
  if (p0+np == total) kp_walk_end(x,pw,total,a);            // the batch ends in this lane
}

// c[0..n) = 0, n <= 64: one wave.  A counter that a kernel adds to is zeroed by this store on the same stream, never by a
// fill of memory taken from the stream-ordered pool: kernel after kernel on one stream is the order
// everything else here rests on.
__global__ void __launch_bounds__(64) kp_zero_kernel(unsigned long long *c, int n)
{ if ((int)threadIdx.x < n) c[threadIdx.x] = 0;
}

// *out += the values of v[0..n) that are not zero
__global__ void __launch_bounds__(KT_BLOCK) kp_nonzero_kernel(const int64_t *v, int64_t n, unsigned long long *out)
{ unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < n; i += (int64_t)gridDim.x*blockDim.x) c += v[i] != 0;
  kc_wave_add(out,c);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

extern "C" int cp_kmer_sorted_read_paths(const cp_kmer_sorted *s, const cp_unitigs *u, const int64_t *d_utg, const int64_t *d_at,
                                         const cp_unitig_graph *g, const char *d_seq, const int64_t *d_seq_off, int nreads,
                                         int64_t total_bases, cp_path_seg *d_segs, int64_t capacity, int64_t *d_seg_off,
                                         int64_t *d_cov, int64_t *d_support, int64_t *tally, int64_t *total, void *stream)
{ const char *who = "cp_kmer_sorted_read_paths";
  static_assert(sizeof(cp_path_seg) == sizeof(kp_seg) && sizeof(kp_seg) == 32 && sizeof(kp_sum) == 32,"a segment is 32 bytes");
  if (!s || !u || !total || nreads < 0 || total_bases < 0 || capacity < 0) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!s->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (u->K != s->K)
    { char m[120];
      snprintf(m,sizeof(m),"%s: the snapshot holds %d-mers and the unitigs are of %d-mers",who,s->K,u->K);
      return set_err(CP_EINVAL,m);
    }
  if (u->count > 0 && (!d_utg || !d_at || !u->off || s->n <= 0))
    return set_err(CP_EINVAL,std::string(who)+": the where arrays are missing or the unitigs are not of this snapshot");
  if (d_support && !g) return set_err(CP_EINVAL,std::string(who)+": d_support needs the graph");
  if ((capacity > 0 && !d_segs) || (nreads > 0 && (!d_seg_off || !d_seq_off)) || (total_bases > 0 && !d_seq))
    return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  const int64_t nblk = nreads > 0 ? (total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS : 0;
  if (nblk > 0x3fffffff) return set_err(CP_EINVAL,std::string(who)+": the batch is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  // one allocation, before anything is queued: the block summaries, the sum of all and the counters, then a word per base
  const size_t nsum = ((size_t)nblk+2)*sizeof(kp_sum), bytes = nsum+(size_t)total_bases*8;
  uint8_t *scratch = nullptr;
  if (nblk > 0 && (hipMallocAsync((void **)&scratch,bytes,st) != hipSuccess || !scratch))
    { (void)hipGetLastError();
      char m[160];
      snprintf(m,sizeof(m),"%s: cannot allocate %zu bytes for the words and the block summaries",who,bytes);
      return set_err(CP_ENOMEM,m);
    }
  *total = 0;
  if (tally) memset(tally,0,CP_PATH_WIDTH*sizeof(int64_t));
  if (d_seg_off)
    { const hipError_t e0 = hipMemsetAsync(d_seg_off,0,((size_t)nreads+1)*sizeof(int64_t),st);
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
  kp_sum *part = (kp_sum *)scratch;
  unsigned long long *ctl = (unsigned long long *)(part+nblk+1);
  unsigned long long *word = (unsigned long long *)(scratch+nsum);          // nsum is a multiple of 32
  const kl_view t = kl_view_of(s);
  kp_args a;
  a.seq = d_seq; a.seq_off = d_seq_off; a.nreads = nreads; a.K = s->K;
  a.uoff = u->off; a.ucount = u->count;
  a.loff = g ? g->loff : nullptr; a.lbase = g ? g->base : nullptr;
  a.gcount = g ? g->count : 0; a.links = (g && g->loff && g->base) ? g->links : 0;
  a.segs = (kp_seg *)d_segs; a.capacity = capacity; a.seg_off = d_seg_off;
  a.cov = d_cov; a.support = d_support;
  kp_zero_kernel<<<1,64,0,st>>>(ctl,(int)(sizeof(kp_sum)/8));               // the counters: a store, not a fill (see there)
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    { if (kl_lo_only(s)) kp_step_kernel<true><<<(unsigned)nblk,KT_BLOCK,0,st>>>(t,d_utg,d_at,u->count,d_seq,d_seq_off,nreads,total_bases,s->K,word,ctl);
      else kp_step_kernel<false><<<(unsigned)nblk,KT_BLOCK,0,st>>>(t,d_utg,d_at,u->count,d_seq,d_seq_off,nreads,total_bases,s->K,word,ctl);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    { kp_count_kernel<<<(unsigned)nblk,KT_BLOCK,0,st>>>(word,total_bases,part);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    { kp_scan_kernel<<<1,KT_BLOCK,0,st>>>(part,nblk);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    { kp_write_kernel<<<(unsigned)nblk,KT_BLOCK,0,st>>>(word,part,nblk,total_bases,a);
      e = hipGetLastError();
    }
  int64_t h[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };               // the sum of all, then the counters
  if (e == hipSuccess) e = hipMemcpyAsync(h,part+nblk,2*sizeof(kp_sum),hipMemcpyDeviceToHost,st);
  const hipError_t ef = hipFreeAsync(scratch,st);
  if (e == hipSuccess) e = ef;
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  const int64_t n = h[0];
  *total = n;
  if (tally)
    { tally[CP_PATH_PRESENT] = h[4+KP_C_PRESENT]; tally[CP_PATH_ABSENT] = h[4+KP_C_ABSENT]; tally[CP_PATH_OTHER] = h[4+KP_C_OTHER];
      tally[CP_PATH_POSITIONS] = tally[CP_PATH_PRESENT]+tally[CP_PATH_ABSENT]+tally[CP_PATH_OTHER];
      tally[CP_PATH_SEGMENTS] = n; tally[CP_PATH_JOINED] = h[1]; tally[CP_PATH_WALKS] = n-h[1];
    }
  if (n > capacity)
    { char m[160];
      snprintf(m,sizeof(m),"%s: %lld segments do not fit the %lld of d_segs",who,(long long)n,(long long)capacity);
      return set_err(CP_EOVERFLOW,m);
    }
  return CP_OK;
}

extern "C" int cp_count_nonzero(const int64_t *d_v, int64_t n, int64_t *count, void *stream)
{ const char *who = "cp_count_nonzero";
  if (!count || n < 0 || (n > 0 && !d_v)) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  *count = 0;
  if (n == 0) return CP_OK;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *d_c = nullptr;
  if (hipMallocAsync((void **)&d_c,8,st) != hipSuccess || !d_c)
    { (void)hipGetLastError();
      return set_err(CP_ENOMEM,std::string(who)+": cannot allocate 8 bytes for the counter");
    }
  kp_zero_kernel<<<1,64,0,st>>>(d_c,1);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    { kp_nonzero_kernel<<<kt_grid((unsigned long long)n),KT_BLOCK,0,st>>>(d_v,n,d_c);
      e = hipGetLastError();
    }
  unsigned long long c = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&c,d_c,8,hipMemcpyDeviceToHost,st);
  const hipError_t ef = hipFreeAsync(d_c,st);
  if (e == hipSuccess) e = ef;
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  *count = (int64_t)c;
  return CP_OK;
}

// label_tools.hip -- two streaming kernels over label strings in HBM (ClassGS): labels from three global count
// thresholds (src/ClassGS.c:228-248) and the accuracy counting of class2acc (src/class2acc.c:141-316) for two label
// strings that are already on the device.  Semantics: include/classpro_amd.h, "Global-threshold labels" and "Label
// accuracy".  Included by capi.hip (set_err, HIPCHK and the library's error contract are shared).
//
// Both kernels are memory-bound element-wise passes with a reduction.  Work layout: the flat base range [0, total_bases)
// is cut into equal contiguous spans, one per WAVE of a capped grid (at most LT_MAX_BLOCKS blocks), so a read of any
// length is simply covered by as many waves as it spans and a batch of any number of reads by the same grid.  A wave
// finds the read holding the start of its span by one binary search and then walks the reads of its span in order;
// the read cursor is wave-uniform.  Inside a read the unit is a GROUP of consecutive label positions counted from
// the start of the read (8 for the thresholds: one 16-byte load of counts, one 8-byte store of labels, two packed
// bytes; 16 for the accuracy: one 16-byte load from either string); a group belongs to the wave whose span holds its
// first position, so every output byte has exactly one writer.  The addresses are only 2- / 1-byte aligned (gfx9
// global loads and stores take unaligned addresses).  All tallies stay in registers over the whole span, are reduced
// per wave by shuffles, per block through LDS, and reach memory as one set of 64-bit atomics per block.

#include <algorithm>

#define LT_BLOCK      256
#define LT_WAVES      (LT_BLOCK/WAVE)
#define LT_MAX_BLOCKS 2048

struct __attribute__((packed, aligned(1))) lt_u8x8 { uint32_t x, y; };
struct __attribute__((packed, aligned(1))) lt_u8x2 { uint16_t v; };

// the read holding flat position p (0 <= p < seq_off[nreads]): the last r with seq_off[r] <= p
__device__ static inline int lt_find_read(const int64_t *__restrict__ seq_off, int nreads, int64_t p)
{ int lo = 0, hi = nreads;
  while (hi-lo > 1)
    { const int mid = (int)(((unsigned)lo+(unsigned)hi) >> 1);
      if (seq_off[mid] <= p) lo = mid; else hi = mid;
    }
  return lo;
}

// v[0..N) summed over the block and added to dst[0..N): shuffles, LDS, one 64-bit atomic per value.  Every thread of
// the block calls it.
template <int N>
__device__ static inline void lt_block_add(unsigned long long (&v)[N], unsigned long long *__restrict__ dst)
{ __shared__ unsigned long long s[LT_WAVES][N];
  const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < N; k++)
    { unsigned long long x = v[k];
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x,o);
      if (lane == 0) s[wv][k] = x;
    }
  __syncthreads();
  if ((int)threadIdx.x < N)
    { unsigned long long x = 0;
      for (int w = 0; w < LT_WAVES; w++) x += s[w][threadIdx.x];
      if (x) atomicAdd(dst+threadIdx.x,x);
    }
}

// ---------------------------------------------------------------------------------------------
//  k_threshold_labels: ClassGS.c:228-248 for every read of a batch.  A count c is E if c < t0, else H if c < t1, else
//  D if c < t2, else R (the reference's chain; thresholds clamped to [0, 65536] by the host).  `sh` = 8 * (index in
//  E, H, D, R) selects the character, the 2-bit code of cp_pack_labels (E 0, H 2, D 3, R 1) and the tally field.
// ---------------------------------------------------------------------------------------------
template <bool LAB, bool PACK, bool CNT>
__global__ void __launch_bounds__(LT_BLOCK)
k_threshold_labels(const uint16_t *__restrict__ prof, const int64_t *__restrict__ prof_off, const int64_t *__restrict__ seq_off,
                   const int64_t *__restrict__ pack_off, int nreads, int64_t total, int64_t span, int Km1,
                   unsigned t0, unsigned t1, unsigned t2, char *__restrict__ labels, uint8_t *__restrict__ packed,
                   unsigned long long *__restrict__ counts)
{ const int lane = lane_id();
  const int wave = (int)blockIdx.x*LT_WAVES+__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = (int64_t)wave*span, w1 = min(w0+span,total);
  unsigned n[4] = { 0, 0, 0, 0 };                                  // this lane's labels, order E, H, D, R
  auto shift_of = [&](unsigned c) -> unsigned { return c < t0 ? 0u : c < t1 ? 8u : c < t2 ? 16u : 24u; };
  if (w0 < total)
    { int r = lt_find_read(seq_off,nreads,w0);
      int64_t rs = seq_off[r];
      while (r < nreads && rs < w1)
        { const int64_t re = seq_off[r+1], rlen = re-rs;
          const int64_t jlo = (max(rs,w0)-rs+7) >> 3, jhi = (min(re,w1)-rs+7) >> 3;   // groups whose start lies in the span
          if (jlo < jhi)
            { const int64_t po = prof_off[r]-Km1;                   // count of the k-mer ending at position l: prof[po+l]
              const int64_t pk = PACK ? pack_off[r] : 0;
              for (int64_t j = jlo+lane; j < jhi; j += WAVE)
                { const int64_t l0 = 8*j;
                  unsigned tally = 0, lo = 0, hi = 0, b0 = 0, b1 = 0;
                  if (l0 >= Km1 && l0+8 <= rlen)
                    { const cp_u16x8 x = *reinterpret_cast<const cp_u16x8 *>(prof+po+l0);
#pragma unroll
                      for (int q = 0; q < 8; q++)
                        { const unsigned sh = shift_of(x.v[q]);
                          if (CNT) tally += 1u << sh;
                          if (LAB)
                            { const unsigned ch = (0x52444845u >> sh) & 0xffu;                 // "EHDR"
                              if (q < 4) lo |= ch << (8*q); else hi |= ch << (8*(q-4));
                            }
                          if (PACK)
                            { const unsigned cd = (0x01030200u >> sh) & 3u;
                              if (q < 4) b0 |= cd << (6-2*q); else b1 |= cd << (6-2*(q-4));
                            }
                        }
                      if (LAB)
                        { lt_u8x8 o; o.x = lo; o.y = hi;
                          *reinterpret_cast<lt_u8x8 *>(labels+rs+l0) = o;
                        }
                      if (PACK)
                        { lt_u8x2 o; o.v = (uint16_t)(b0 | (b1 << 8));
                          *reinterpret_cast<lt_u8x2 *>(packed+pk+2*j) = o;
                        }
                    }
                  else                                              // the 'N' prefix or the end of the read: by position
                    { for (int q = 0; q < 8; q++)
                        { const int64_t l = l0+q;
                          if (l >= rlen) break;
                          unsigned ch = 'N', cd = 0;
                          if (l >= Km1)
                            { const unsigned sh = shift_of(prof[po+l]);
                              if (CNT) tally += 1u << sh;
                              ch = (0x52444845u >> sh) & 0xffu;
                              cd = (0x01030200u >> sh) & 3u;
                            }
                          if (LAB) labels[rs+l] = (char)ch;
                          if (q < 4) b0 |= cd << (6-2*q); else b1 |= cd << (6-2*(q-4));
                        }
                      if (PACK)
                        { if (l0 < rlen)   packed[pk+2*j]   = (uint8_t)b0;
                          if (l0+4 < rlen) packed[pk+2*j+1] = (uint8_t)b1;
                        }
                    }
                  if (CNT)
                    { n[0] += tally & 0xffu; n[1] += (tally >> 8) & 0xffu; n[2] += (tally >> 16) & 0xffu; n[3] += tally >> 24; }
                }
            }
          rs = re;
          r++;
        }
    }
  if (CNT)
    { unsigned long long v[4] = { n[0], n[1], n[2], n[3] };
      lt_block_add<4>(v,counts);
    }
}

extern "C" int cp_threshold_labels(int K, const int32_t *thres, const uint16_t *d_prof, const int64_t *d_prof_off,
                                   const int64_t *d_seq_off, int nreads, int64_t total_bases, char *d_labels,
                                   uint8_t *d_packed, const int64_t *d_pack_off, int64_t *d_counts, void *stream)
{ if (K < 1 || !thres || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_threshold_labels: bad argument");
  if (!d_labels && !d_packed && !d_counts) return set_err(CP_EINVAL,"cp_threshold_labels: no output wanted");
  if (d_packed && !d_pack_off) return set_err(CP_EINVAL,"cp_threshold_labels: d_packed needs d_pack_off");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_prof || !d_prof_off || !d_seq_off) return set_err(CP_EINVAL,"cp_threshold_labels: null device pointer");
  unsigned t[3];                                                  // counts are uint16: outside [0, 65536] nothing changes
  for (int i = 0; i < 3; i++) t[i] = (unsigned)std::min<int64_t>(std::max<int64_t>(thres[i],0),65536);
  // one span per wave, a whole number of 64 x 8 positions
  const int64_t unit = (int64_t)WAVE*8;
  const int64_t nwaves = std::min<int64_t>((int64_t)LT_MAX_BLOCKS*LT_WAVES,(total_bases+unit-1)/unit);
  const int64_t span = ((total_bases+nwaves-1)/nwaves+unit-1)/unit*unit;
  const int grid = (int)((nwaves+LT_WAVES-1)/LT_WAVES);
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *cnt = (unsigned long long *)d_counts;
#define LT_LAUNCH(L,P,C) hipLaunchKernelGGL((k_threshold_labels<L,P,C>),dim3(grid),dim3(LT_BLOCK),0,st,d_prof,d_prof_off,d_seq_off, \
                                            d_pack_off,nreads,total_bases,span,K-1,t[0],t[1],t[2],d_labels,d_packed,cnt)
  switch ((d_labels ? 4 : 0) | (d_packed ? 2 : 0) | (d_counts ? 1 : 0))
    { case 1: LT_LAUNCH(false,false,true); break;
      case 2: LT_LAUNCH(false,true,false); break;
      case 3: LT_LAUNCH(false,true,true); break;
      case 4: LT_LAUNCH(true,false,false); break;
      case 5: LT_LAUNCH(true,false,true); break;
      case 6: LT_LAUNCH(true,true,false); break;
      default: LT_LAUNCH(true,true,true); break;
    }
#undef LT_LAUNCH
  return launch_status();
}

// ---------------------------------------------------------------------------------------------
//  Label accuracy.  Device totals of one accumulator (all 64-bit):
//    [0,16) cfm[truth][estimate], order E R H D;  [16,19) ntot ncor nfne of all counted reads;  [19,22) normal;
//    [22,25) repeat;  [25] reads filtered out;  [26] invalid characters.
//  A read's decision needs its whole composition, so a wave finishes the reads that lie wholly inside its span itself
//  and adds its share of a read that crosses a span boundary (at most two per wave) to that read's four counters in
//  `part`; k_acc_finish then decides those reads, one thread per span boundary.
// ---------------------------------------------------------------------------------------------
#define LT_NTOT 27

struct lt_read_sums { unsigned long long comp_e, comp_r, cor, fne; };      // truth E, truth R, equal, truth E and estimate not E

// class2acc.c:243-262 for one read; t = the nine totals + filtered count, indices as in the device totals minus 16
__device__ static inline void lt_acc_decide(const lt_read_sums &q, int64_t rtot, double max_e_pct, double rep_pct,
                                            unsigned long long *t)
{ if (rtot <= 0) return;
  if ((double)q.comp_e/(double)rtot*100 > max_e_pct) { t[9]++; return; }
  const int o = ((double)q.comp_r/(double)rtot*100 > rep_pct) ? 6 : 3;
  t[0] += (unsigned long long)rtot; t[1] += q.cor; t[2] += q.fne;
  t[o] += (unsigned long long)rtot; t[o+1] += q.cor; t[o+2] += q.fne;
}

// E R H D -> 0 1 2 3 (stoc of class2acc), anything else 15: a table of nibbles indexed by c-'D'
__device__ static inline unsigned lt_state(unsigned c)
{ const unsigned d = c-0x44u;
  return d < 16u ? (unsigned)(0xF1FFFFFFFFF2FF03ull >> (4*d)) & 15u : 15u;
}

__global__ void __launch_bounds__(LT_BLOCK)
k_acc_add(const char *__restrict__ est, const char *__restrict__ truth, const int64_t *__restrict__ seq_off, int nreads,
          int64_t total, int64_t span, int Km1, double max_e_pct, double rep_pct, unsigned long long *__restrict__ part,
          unsigned long long *__restrict__ tot)
{ const int lane = lane_id();
  const int wave = (int)blockIdx.x*LT_WAVES+__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = (int64_t)wave*span, w1 = min(w0+span,total);
  unsigned gc[16], rc[16];                                         // cfm cells of this lane: whole span, current read
#pragma unroll
  for (int k = 0; k < 16; k++) gc[k] = rc[k] = 0;
  unsigned ninv = 0;
  unsigned long long wt[10] = { 0,0,0,0,0,0,0,0,0,0 };             // wave-uniform: nine totals, filtered reads
  if (w0 < total)
    { int r = lt_find_read(seq_off,nreads,w0);
      int64_t rs = seq_off[r];
      while (r < nreads && rs < w1)
        { const int64_t re = seq_off[r+1], rlen = re-rs;
          const int64_t jlo = (max(rs,w0)-rs+15) >> 4, jhi = (min(re,w1)-rs+15) >> 4;
          if (rlen > Km1)
            { const char *e = est+rs, *t = truth+rs;
              unsigned long long lo8 = 0, hi8 = 0;                 // cells 0,2,..,14 / 1,3,..,15 in 8-bit fields
              int nsp = 0;
              // one position: its cell truth x estimate as a 4-bit field increment; an invalid character counts apart
              auto cell = [&](unsigned ec, unsigned tc) -> unsigned long long
                { const unsigned ei = lt_state(ec), ti = lt_state(tc);
                  const unsigned ok = (ei | ti) < 4u ? 1u : 0u;
                  ninv += 1u-ok;
                  return (unsigned long long)ok << ((16*ti+4*ei) & 63u);
                };
              auto spill = [&]()
                {
#pragma unroll
                  for (int k = 0; k < 8; k++)
                    { rc[2*k] += (unsigned)(lo8 >> (8*k)) & 0xffu; rc[2*k+1] += (unsigned)(hi8 >> (8*k)) & 0xffu; }
                  lo8 = hi8 = 0; nsp = 0;
                };
              for (int64_t j = jlo+lane; j < jhi; j += WAVE)
                { const int64_t l0 = 16*j;
                  if (l0 >= Km1 && l0+16 <= rlen)
                    { const cp_u8x16 x = *reinterpret_cast<const cp_u8x16 *>(e+l0);
                      const cp_u8x16 y = *reinterpret_cast<const cp_u8x16 *>(t+l0);
#pragma unroll
                      for (int h = 0; h < 2; h++)
                        { unsigned long long a4 = 0;                 // 16 cells in 4-bit fields: at most 8 per half
#pragma unroll
                          for (int q = 0; q < 8; q++)
                            a4 += cell((x.v[2*h+(q >> 2)] >> (8*(q & 3))) & 0xffu,(y.v[2*h+(q >> 2)] >> (8*(q & 3))) & 0xffu);
                          lo8 += a4 & 0x0F0F0F0F0F0F0F0Full;
                          hi8 += (a4 >> 4) & 0x0F0F0F0F0F0F0F0Full;
                        }
                    }
                  else                                              // the 'N' prefix or the end of the read: by position
                    for (int h = 0; h < 2; h++)
                      { unsigned long long a4 = 0;
                        for (int q = 0; q < 8; q++)
                          { const int64_t l = l0+8*h+q;
                            if (l >= Km1 && l < rlen) a4 += cell((unsigned char)e[l],(unsigned char)t[l]);
                          }
                        lo8 += a4 & 0x0F0F0F0F0F0F0F0Full;
                        hi8 += (a4 >> 4) & 0x0F0F0F0F0F0F0F0Full;
                      }
                  if (++nsp == 15) spill();                         // 15 x 16 = 240 <= 255 per field
                }
              spill();
              lt_read_sums q;
              q.comp_e = rc[0]+rc[1]+rc[2]+rc[3];
              q.comp_r = rc[4]+rc[5]+rc[6]+rc[7];
              q.cor = rc[0]+rc[5]+rc[10]+rc[15];
              q.fne = rc[1]+rc[2]+rc[3];
#pragma unroll
              for (int k = 0; k < 16; k++) { gc[k] += rc[k]; rc[k] = 0; }
              for (int o = 32; o > 0; o >>= 1)
                { q.comp_e += __shfl_xor(q.comp_e,o); q.comp_r += __shfl_xor(q.comp_r,o);
                  q.cor += __shfl_xor(q.cor,o); q.fne += __shfl_xor(q.fne,o);
                }
              if (rs >= w0 && re <= w1) lt_acc_decide(q,rlen-Km1,max_e_pct,rep_pct,wt);
              else if (lane == 0)                                   // a read that crosses a span boundary
                { unsigned long long *p = part+4*(int64_t)r;
                  if (q.comp_e) atomicAdd(p,q.comp_e);
                  if (q.comp_r) atomicAdd(p+1,q.comp_r);
                  if (q.cor) atomicAdd(p+2,q.cor);
                  if (q.fne) atomicAdd(p+3,q.fne);
                }
            }
          rs = re;
          r++;
        }
    }
  unsigned long long v[LT_NTOT];
#pragma unroll
  for (int k = 0; k < 16; k++) v[k] = gc[k];
#pragma unroll
  for (int k = 0; k < 10; k++) v[16+k] = lane == 0 ? wt[k] : 0;
  v[26] = ninv;
  lt_block_add<LT_NTOT>(v,tot);
}

// the reads that cross a span boundary: the thread of span w decides the read that began before w0 and ends inside
// (w0, w1]; every wave's share of it is in `part` by now (stream order)
__global__ void __launch_bounds__(LT_BLOCK)
k_acc_finish(const int64_t *__restrict__ seq_off, int nreads, int64_t total, int64_t span, int64_t nwaves, int Km1,
             double max_e_pct, double rep_pct, const unsigned long long *__restrict__ part, unsigned long long *__restrict__ tot)
{ const int64_t w = (int64_t)blockIdx.x*LT_BLOCK+threadIdx.x;
  unsigned long long v[10] = { 0,0,0,0,0,0,0,0,0,0 };
  const int64_t w0 = w*span, w1 = min(w0+span,total);
  if (w > 0 && w < nwaves && w0 < total)
    { const int r = lt_find_read(seq_off,nreads,w0);
      const int64_t rs = seq_off[r], re = seq_off[r+1];
      if (rs < w0 && w0 < re && re <= w1)
        { lt_read_sums q;
          q.comp_e = part[4*(int64_t)r]; q.comp_r = part[4*(int64_t)r+1]; q.cor = part[4*(int64_t)r+2]; q.fne = part[4*(int64_t)r+3];
          lt_acc_decide(q,re-rs-Km1,max_e_pct,rep_pct,v);
        }
    }
  lt_block_add<10>(v,tot+16);
}

struct cp_acc
  { int K = 0, device = 0;
    double max_e_pct = 100, rep_pct = 0;
    unsigned long long *tot = nullptr;       // device totals, LT_NTOT
    unsigned long long *part = nullptr;      // device: four counters per read of the batch being added
    int64_t part_reads = 0;
    int64_t n_reads = 0;
    hipStream_t stream = nullptr;
  };

extern "C" void cp_acc_destroy(cp_acc *a)
{ if (!a) return;
  (void)hipDeviceSynchronize();
  if (a->tot) (void)hipFree(a->tot);
  if (a->part) (void)hipFree(a->part);
  delete a;
}

extern "C" int cp_acc_create(int K, double max_e_pct, double rep_pct, cp_acc **out)
{ if (!out) return set_err(CP_EINVAL,"cp_acc_create: null out");
  *out = nullptr;
  if (K < 1 || !(max_e_pct == max_e_pct) || !(rep_pct == rep_pct))
    return set_err(CP_EINVAL,"cp_acc_create: bad argument");
  cp_acc *a = new (std::nothrow) cp_acc();
  if (!a) return set_err(CP_ENOMEM,"cp_acc_create: out of memory");
  a->K = K; a->max_e_pct = max_e_pct; a->rep_pct = rep_pct;
  hipError_t e = hipGetDevice(&a->device);
  if (e == hipSuccess) e = hipMalloc(&a->tot,LT_NTOT*sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(a->tot,0,LT_NTOT*sizeof(unsigned long long));
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);              // the fill is on the null stream; the first add need not be
  if (e != hipSuccess)
    { const int rc = set_err(CP_EHIP,std::string("cp_acc_create: ")+hipGetErrorString(e));
      cp_acc_destroy(a);
      return rc;
    }
  *out = a;
  return CP_OK;
}

extern "C" int cp_acc_add(cp_acc *a, const char *d_est, const char *d_truth, const int64_t *d_seq_off, int nreads,
                          int64_t total_bases, void *stream)
{ if (!a || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_acc_add: bad argument");
  hipStream_t st = (hipStream_t)stream;
  a->stream = st;
  a->n_reads += nreads;
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_est || !d_truth || !d_seq_off) return set_err(CP_EINVAL,"cp_acc_add: null device pointer");
  if (nreads > a->part_reads)
    { HIPCHK(hipStreamSynchronize(st));
      if (a->part) { (void)hipFree(a->part); a->part = nullptr; a->part_reads = 0; }
      if (hipMalloc(&a->part,(size_t)nreads*4*sizeof(unsigned long long)) != hipSuccess)
        { (void)hipGetLastError();
          return set_err(CP_ENOMEM,"cp_acc_add: cannot allocate the per-read counters");
        }
      a->part_reads = nreads;
    }
  HIPCHK(hipMemsetAsync(a->part,0,(size_t)nreads*4*sizeof(unsigned long long),st));
  const int64_t unit = (int64_t)WAVE*16;
  const int64_t nwaves = std::min<int64_t>((int64_t)LT_MAX_BLOCKS*LT_WAVES,(total_bases+unit-1)/unit);
  const int64_t span = ((total_bases+nwaves-1)/nwaves+unit-1)/unit*unit;
  const int grid = (int)((nwaves+LT_WAVES-1)/LT_WAVES);
  hipLaunchKernelGGL(k_acc_add,dim3(grid),dim3(LT_BLOCK),0,st,d_est,d_truth,d_seq_off,nreads,total_bases,span,a->K-1,
                     a->max_e_pct,a->rep_pct,a->part,a->tot);
  hipLaunchKernelGGL(k_acc_finish,dim3((int)((nwaves+LT_BLOCK-1)/LT_BLOCK)),dim3(LT_BLOCK),0,st,d_seq_off,nreads,total_bases,
                     span,nwaves,a->K-1,a->max_e_pct,a->rep_pct,a->part,a->tot);
  return launch_status();
}

extern "C" int cp_acc_read(cp_acc *a, cp_acc_stats *out)
{ if (!a || !out) return set_err(CP_EINVAL,"cp_acc_read: bad argument");
  unsigned long long h[LT_NTOT];
  HIPCHK(hipMemcpyAsync(h,a->tot,sizeof(h),hipMemcpyDeviceToHost,a->stream));
  HIPCHK(hipStreamSynchronize(a->stream));
  memset(out,0,sizeof(*out));
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) out->cfm[i][j] = (int64_t)h[4*i+j];
  out->ntot = (int64_t)h[16]; out->ncor = (int64_t)h[17]; out->nfne = (int64_t)h[18];
  out->ntot_normal = (int64_t)h[19]; out->ncor_normal = (int64_t)h[20]; out->nfne_normal = (int64_t)h[21];
  out->ntot_repeat = (int64_t)h[22]; out->ncor_repeat = (int64_t)h[23]; out->nfne_repeat = (int64_t)h[24];
  out->n_reads = a->n_reads;
  out->n_reads_filtered = (int64_t)h[25];
  out->n_invalid = (int64_t)h[26];
  if (h[26])
    return set_err(CP_EINVAL,"cp_acc: "+std::to_string(h[26])+" label positions held a character other than E/H/D/R");
  return CP_OK;
}

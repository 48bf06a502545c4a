// kmer_sort.hip -- a sorted snapshot of a count table (kprof -t): every key with count >= min_count, ascending by key,
// and its FASTK .ktab payload (prefix index and fixed-width records) encoded on the device.  Semantics:
// include/classpro_amd.h, "Sorted k-mers"; design: DESIGN.md 9.11.  Included by capi.hip after kmer_counts.hip (the table,
// set_err, HIPCHK and the library's error contract are in scope).  The table is only read.
// The same snapshot of a LABEL table (class2ktab), one consensus class per call, and that table's per-class histogram:
// "Sorted k-mers of a label table" in the header, DESIGN.md 9.12.  The two sweeps over the slots are templates over the
// slot type and a selector (slot -> keep?, 64-bit payload); everything behind the scatter sees keys and payloads only.
//
// The file format names the partition: a bucket is the top pbits = 8*ibyte bits of the key (2K bits where K < 5 and
// there is no .ktab), and the prefix sum over the bucket sizes is the .ktab index.
//   count    a slot sweep, one 64-bit atomic per qualifying slot on its bucket's counter;
//   scan     three launches (sums of chunks, one block over the sums, the chunks again) leave the inclusive sums;
//   scatter  a second sweep; a slot takes the next place from its bucket's END (a returning atomic decrement), which
//            leaves the counters as the bucket STARTS: start[p+1] is index[p] of the .ktab;
//   tiles    the entries are grouped by bucket now and unordered inside one.  Block b owns the buckets that begin in
//            [B(b*KS_TILE), B((b+1)*KS_TILE)), B(x) the first bucket start at or after x; it cuts them greedily into
//            runs of whole buckets of at most KS_TILE entries and sorts each run by its full key in LDS.  All cuts are
//            binary searches over the bucket starts, so millions of empty buckets cost nothing;
//   oversize a bucket of more than KS_TILE entries is skipped by the tiles and sorted in place in device memory, all
//            such buckets at once, one launch per step of the network.
// Both sorts run the bitonic network in the form whose comparators all point the same way (a merge begins by comparing
// i with its mirror image in the block, the strides follow): imaginary +infinity entries behind the last one never move,
// so a run of any length is sorted by leaving out the comparators that reach past its end.
#define KS_TILE   2048                     // entries sorted by one block in LDS: 3 arrays of 8 bytes = 48 KiB of the CU's 160
#define KS_BLOCK  256
#define KS_CHUNK  4096                     // counters per block of the scan: 16 per lane
#define KS_ENC    256                      // records per block of the encode kernel
#define KS_MAXREC 18                       // a bound on a record's bytes: the 16 key bytes of K = 63 and the count

struct cp_kmer_sorted
  { int K, ibyte, pbits;
    int64_t n;                             // entries
    int64_t nb;                            // buckets = 1 << pbits
    unsigned long long *key;               // hi[n], lo[n], cnt[n] in one allocation (null when n = 0)
    int64_t *start;                        // nb+1 bucket starts; start[nb] = n
    bool ready;                            // sorted here, or loaded and checked (kmer_lookup.hip): the queries take it
    int64_t filled;                        // a snapshot being loaded: the entries appended so far
  };

__device__ static inline unsigned long long ks_bucket(unsigned long long hi, unsigned long long lo, int shift)
{ return (unsigned long long)(((((kt_u128)hi) << 63) | (kt_u128)lo) >> shift); }

// A selector says which slots a snapshot keeps and what it carries for them: keep(slot, &payload).
struct ks_sel_count                        // the count table: the keys seen at least min_count times, with their count
  { unsigned long long min_count;
    __device__ bool keep(const kc_slot &e, unsigned long long *pay) const
    { *pay = e.cnt;
      return e.cnt >= min_count;
    }
  };

struct ks_sel_class                        // the label table: the rule of "Sorted k-mers of a label table", with the total
  { int label;                             // -1: every class
    unsigned long long min_total, min_pct;
    __device__ bool keep(const kt_slot &e, unsigned long long *pay) const
    { unsigned long long tot = 0, mx = 0;
      for (int l = 0; l < 4; l++)
        { tot += e.cnt[l];
          mx = max(mx,(unsigned long long)e.cnt[l]);
        }
      *pay = tot;                          // tot < 2^34, so 100*mx and min_pct*tot stay far below 2^64
      return (label < 0 || kt_consensus(e.cnt) == label) && tot >= min_total && 100*mx >= min_pct*tot;
    }
  };

template <class Slot, class Sel>
__global__ void __launch_bounds__(KT_BLOCK) ks_count_kernel(const Slot *tab, unsigned long long nslots, Sel sel, int shift,
                                                            int64_t *start)
{ for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < nslots;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const Slot e = tab[s];
      unsigned long long pay;
      if (e.lo == KT_EMPTY || !sel.keep(e,&pay)) continue;
      atomicAdd((unsigned long long *)&start[ks_bucket(e.hi,e.lo,shift)],1ull);
    }
}

template <class Slot, class Sel>
__global__ void __launch_bounds__(KT_BLOCK) ks_scatter_kernel(const Slot *tab, unsigned long long nslots, Sel sel, int shift,
                                                              int64_t *start, unsigned long long *hi,
                                                              unsigned long long *lo, unsigned long long *cnt, int64_t n)
{ for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < nslots;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const Slot e = tab[s];
      unsigned long long pay;
      if (e.lo == KT_EMPTY || !sel.keep(e,&pay)) continue;
      const int64_t i = (int64_t)atomicAdd((unsigned long long *)&start[ks_bucket(e.hi,e.lo,shift)],~0ull)-1;
      if ((unsigned long long)i >= (unsigned long long)n) continue;        // cannot happen while the table is only read
      hi[i] = e.hi;
      lo[i] = e.lo;
      cnt[i] = pay;
    }
}

// The per-class histogram of a label table: hist[l*(CP_MAX_KMER_CNT+1) + ...] is the layout of kc_hist_kernel for the
// keys of consensus class l, the total of a key's four counts standing for the count.  4 x KC_LOW_BINS bins in LDS.
__global__ void __launch_bounds__(KT_BLOCK) ks_class_hist_kernel(const kt_slot *tab, unsigned long long n,
                                                                 unsigned long long *hist)
{ __shared__ unsigned int low[4*KC_LOW_BINS];
  for (int i = threadIdx.x; i < 4*KC_LOW_BINS; i += KT_BLOCK) low[i] = 0;
  __syncthreads();
  for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < n;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const kt_slot e = tab[s];
      if (e.lo == KT_EMPTY) continue;
      const unsigned long long tot = (unsigned long long)e.cnt[0]+e.cnt[1]+e.cnt[2]+e.cnt[3];
      if (tot == 0) continue;
      const int l = kt_consensus(e.cnt);
      unsigned long long *h = hist+(size_t)l*(CP_MAX_KMER_CNT+1);
      if (tot <= KC_LOW_BINS) atomicAdd(&low[l*KC_LOW_BINS+(int)tot-1],1u);
      else if (tot < CP_MAX_KMER_CNT) atomicAdd(&h[tot-1],1ull);
      else
        { atomicAdd(&h[CP_MAX_KMER_CNT-1],1ull);
          atomicAdd(&h[CP_MAX_KMER_CNT],tot);
        }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < 4*KC_LOW_BINS; i += KT_BLOCK)
    if (low[i]) atomicAdd(&hist[(size_t)(i/KC_LOW_BINS)*(CP_MAX_KMER_CNT+1)+(i%KC_LOW_BINS)],(unsigned long long)low[i]);
}

// the block's inclusive scan of one value per lane (KS_BLOCK lanes); `part` is KS_BLOCK words of LDS
__device__ static inline unsigned long long ks_block_scan(unsigned long long v, unsigned long long *part)
{ part[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < KS_BLOCK; d <<= 1)
    { const unsigned long long a = threadIdx.x >= (unsigned)d ? part[threadIdx.x-d] : 0;
      __syncthreads();
      part[threadIdx.x] += a;
      __syncthreads();
    }
  return part[threadIdx.x];
}

// sum[b] = the sum of chunk b of v[0..n)
__global__ void __launch_bounds__(KS_BLOCK) ks_chunk_sum_kernel(const int64_t *v, int64_t n, unsigned long long *sum)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x*KS_CHUNK+(int64_t)threadIdx.x*(KS_CHUNK/KS_BLOCK);
  unsigned long long a = 0;
  for (int k = 0; k < KS_CHUNK/KS_BLOCK; k++)
    if (i0+k < n) a += (unsigned long long)v[i0+k];
  a = ks_block_scan(a,part);
  if (threadIdx.x == KS_BLOCK-1) sum[blockIdx.x] = a;
}

// one block: sum[0..m) to its exclusive scan, m <= KS_CHUNK
__global__ void __launch_bounds__(KS_BLOCK) ks_sum_scan_kernel(unsigned long long *sum, int m)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int i0 = (int)threadIdx.x*(KS_CHUNK/KS_BLOCK);
  unsigned long long x[KS_CHUNK/KS_BLOCK], a = 0;
  for (int k = 0; k < KS_CHUNK/KS_BLOCK; k++)
    { x[k] = i0+k < m ? sum[i0+k] : 0;
      a += x[k];
    }
  unsigned long long run = ks_block_scan(a,part)-a;
  for (int k = 0; k < KS_CHUNK/KS_BLOCK; k++)
    { if (i0+k < m) sum[i0+k] = run;
      run += x[k];
    }
}

// v[0..n) to its inclusive scan, chunk b starting from sum[b]
__global__ void __launch_bounds__(KS_BLOCK) ks_chunk_scan_kernel(int64_t *v, int64_t n, const unsigned long long *sum)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x*KS_CHUNK+(int64_t)threadIdx.x*(KS_CHUNK/KS_BLOCK);
  unsigned long long x[KS_CHUNK/KS_BLOCK], a = 0;
  for (int k = 0; k < KS_CHUNK/KS_BLOCK; k++)
    { x[k] = i0+k < n ? (unsigned long long)v[i0+k] : 0;
      a += x[k];
    }
  unsigned long long run = sum[blockIdx.x]+ks_block_scan(a,part)-a;
  for (int k = 0; k < KS_CHUNK/KS_BLOCK; k++)
    { run += x[k];
      if (i0+k < n) v[i0+k] = (int64_t)run;
    }
}

// the first index p in [0, m] with start[p] >= x; start[0..m] is nondecreasing and start[m] >= x
__device__ static inline int64_t ks_lower(const int64_t *start, int64_t m, int64_t x)
{ int64_t a = 0, b = m;
  while (a < b)
    { const int64_t mid = (a+b) >> 1;
      if (start[mid] >= x) b = mid; else a = mid+1;
    }
  return a;
}

// Comparator q of a step of the network over a power of two of entries: the pair (i, l), i < l.  flip: the first step
// of the merge of blocks of k entries, i against its mirror image; otherwise the stride j.
__device__ static inline void ks_pair(int64_t q, int64_t k, int64_t j, bool flip, int64_t *i, int64_t *l)
{ const int64_t o = q & ((flip ? k >> 1 : j)-1), base = 2*(q-o);   // k and j are powers of two: no division
  *i = base+o;
  *l = flip ? base+k-1-o : base+o+j;
}

__device__ static inline void ks_cmpswap(unsigned long long *hi, unsigned long long *lo, unsigned long long *cnt,
                                         int64_t i, int64_t l)
{ const unsigned long long ah = hi[i], bh = hi[l], al = lo[i], bl = lo[l];
  if (ah > bh || (ah == bh && al > bl))
    { hi[i] = bh; hi[l] = ah;
      lo[i] = bl; lo[l] = al;
      const unsigned long long c = cnt[i];
      cnt[i] = cnt[l];
      cnt[l] = c;
    }
}

__global__ void __launch_bounds__(KS_BLOCK) ks_tile_kernel(unsigned long long *hi, unsigned long long *lo,
                                                           unsigned long long *cnt, const int64_t *start, int64_t nb,
                                                           int64_t n)
{ __shared__ unsigned long long shi[KS_TILE], slo[KS_TILE], scn[KS_TILE];
  const int64_t w0 = (int64_t)blockIdx.x*KS_TILE, w1 = min(w0+(int64_t)KS_TILE,n);
  int64_t s = start[ks_lower(start,nb,w0)];
  const int64_t end = start[ks_lower(start,nb,w1)];
  while (s < end)                                         // every lane of the block holds the same s, e and end
    { int64_t e = end;
      if (end-s > KS_TILE)
        { e = start[ks_lower(start,nb,s+KS_TILE+1)-1];    // the last bucket start <= s + KS_TILE; s is one, so e >= s
          if (e == s)                                     // a bucket of more than KS_TILE entries begins here: not ours
            { s = start[ks_lower(start,nb,s+1)];
              continue;
            }
        }
      const int m = (int)(e-s);
      if (m > 1)
        { for (int i = threadIdx.x; i < m; i += KS_BLOCK)
            { shi[i] = hi[s+i]; slo[i] = lo[s+i]; scn[i] = cnt[s+i]; }
          __syncthreads();
          int np = 2;
          while (np < m) np <<= 1;
          for (int k = 2; k <= np; k <<= 1)               // the merge of blocks of k: the flip, then the strides k/4 .. 1
            { for (int q = threadIdx.x; q < np/2; q += KS_BLOCK)
                { int64_t i, l;
                  ks_pair(q,k,0,true,&i,&l);
                  if (l < m) ks_cmpswap(shi,slo,scn,i,l);
                }
              __syncthreads();
              for (int j = k >> 2; j > 0; j >>= 1)
                { for (int q = threadIdx.x; q < np/2; q += KS_BLOCK)
                    { int64_t i, l;
                      ks_pair(q,k,j,false,&i,&l);
                      if (l < m) ks_cmpswap(shi,slo,scn,i,l);
                    }
                  __syncthreads();
                }
            }
          for (int i = threadIdx.x; i < m; i += KS_BLOCK)
            { hi[s+i] = shi[i]; lo[s+i] = slo[i]; cnt[s+i] = scn[i]; }
          __syncthreads();
        }
      s = e;
    }
}

struct ks_run { int64_t start, len; };

// the buckets of more than KS_TILE entries into list[0..ctl[0]), the longest into ctl[1]
__global__ void __launch_bounds__(KT_BLOCK) ks_oversize_kernel(const int64_t *start, int64_t nb, ks_run *list,
                                                               int64_t cap, unsigned long long *ctl)
{ for (int64_t p = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; p < nb; p += (int64_t)gridDim.x*blockDim.x)
    { const int64_t len = start[p+1]-start[p];
      if (len <= KS_TILE) continue;
      const unsigned long long at = atomicAdd(&ctl[0],1ull);
      if ((int64_t)at < cap)
        { list[at].start = start[p];
          list[at].len = len;
        }
      atomicMax(&ctl[1],(unsigned long long)len);
    }
}

// one step of the network over every oversize bucket, in device memory: blockIdx.y picks the bucket
__global__ void __launch_bounds__(KS_BLOCK) ks_step_kernel(unsigned long long *hi, unsigned long long *lo,
                                                           unsigned long long *cnt, const ks_run *list, int64_t k,
                                                           int64_t j, int flip)
{ const ks_run r = list[blockIdx.y];
  int64_t np = 2;
  while (np < r.len) np <<= 1;
  if (k > np) return;                                     // a shorter bucket than the longest: sorted already
  for (int64_t q = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; q < np/2; q += (int64_t)gridDim.x*blockDim.x)
    { int64_t i, l;
      ks_pair(q,k,j,flip != 0,&i,&l);
      if (l < r.len) ks_cmpswap(hi+r.start,lo+r.start,cnt+r.start,i,l);
    }
}

// The records of the entries [first, first+n): the key left-aligned in kbyte bytes, its last hbyte bytes, then the count
// clamped to CP_MAX_KMER_CNT as a little-endian uint16.  A block stages its KS_ENC records in LDS and stores them as
// 32-bit words between a byte-wise head and tail, the way kc_store_cells stores profile cells.
__global__ void __launch_bounds__(KS_ENC) ks_encode_kernel(const unsigned long long *hi, const unsigned long long *lo,
                                                           const unsigned long long *cnt, int64_t first, int64_t n,
                                                           int K, int ibyte, uint8_t *rec)
{ __shared__ uint8_t stage[KS_ENC*KS_MAXREC];
  const int kbyte = (K+3) >> 2, hbyte = kbyte-ibyte, pbyte = hbyte+2;
  const int64_t b0 = (int64_t)blockIdx.x*KS_ENC;
  const int m = (int)min((int64_t)KS_ENC,n-b0);
  if ((int)threadIdx.x < m)
    { const int64_t e = first+b0+threadIdx.x;
      const kt_u128 key = (((((kt_u128)hi[e]) << 63) | (kt_u128)lo[e])) << (8*kbyte-2*K);
      uint8_t *o = stage+(int)threadIdx.x*pbyte;
      for (int b = 0; b < hbyte; b++) o[b] = (uint8_t)(key >> (8*(hbyte-1-b)));
      const unsigned c = (unsigned)min(cnt[e],(unsigned long long)CP_MAX_KMER_CNT);
      o[hbyte] = (uint8_t)(c & 0xffu);
      o[hbyte+1] = (uint8_t)(c >> 8);
    }
  __syncthreads();
  if (m <= 0) return;
  uint8_t *dst = rec+b0*pbyte;
  const int nbytes = m*pbyte;
  const int head = min(nbytes,(int)((4-((uintptr_t)dst & 3)) & 3));
  const int nw = (nbytes-head) >> 2, tail = head+4*nw;
  if ((int)threadIdx.x < head) dst[threadIdx.x] = stage[threadIdx.x];
  for (int w = threadIdx.x; w < nw; w += KS_ENC)
    { const uint8_t *s = stage+head+4*w;
      *(unsigned int *)(dst+head+4*w) = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
  if ((int)threadIdx.x < nbytes-tail) dst[tail+threadIdx.x] = stage[tail+threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

extern "C" int cp_ktab_ibyte(int K)
{ return K >= 13 ? 3 : K >= 9 ? 2 : K >= 5 ? 1 : 0; }

extern "C" int cp_ktab_tile(void)
{ return KS_TILE; }

extern "C" void cp_kmer_sorted_destroy(cp_kmer_sorted *s)
{ if (!s) return;
  if (s->key) (void)hipFree(s->key);                       // hipFree waits for the work that may still read it
  if (s->start) (void)hipFree(s->start);
  delete s;
}

static int ks_alloc(const char *who, void **p, size_t bytes, const char *what)
{ const hipError_t e = hipMalloc(p,bytes);
  if (e == hipSuccess) return CP_OK;
  (void)hipGetLastError();
  *p = nullptr;
  char m[200];
  snprintf(m,sizeof(m),"%s: hipMalloc(%s, %llu bytes): %s",who,what,(unsigned long long)bytes,hipGetErrorString(e));
  return set_err(CP_ENOMEM,m);
}

// the sort of the buckets of more than KS_TILE entries (see the file comment); scratch is freed by the caller
static int ks_sort_oversize(const char *who, cp_kmer_sorted *s, hipStream_t st, void **scratch)
{ unsigned long long *hi = s->key, *lo = s->key+s->n, *cnt = s->key+2*s->n;
  const int64_t cap = s->n/(KS_TILE+1)+1;                  // no more buckets than that can be oversize
  int rc = ks_alloc(who,scratch,16+(size_t)cap*sizeof(ks_run),"the oversize list");
  if (rc != CP_OK) return rc;
  unsigned long long *ctl = (unsigned long long *)*scratch, h_ctl[2];
  ks_run *list = (ks_run *)(ctl+2);
  HIPCHK(hipMemsetAsync(ctl,0,16,st));
  ks_oversize_kernel<<<kt_grid((unsigned long long)s->nb),KT_BLOCK,0,st>>>(s->start,s->nb,list,cap,ctl);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_ctl,ctl,16,hipMemcpyDeviceToHost,st));
  HIPCHK(hipStreamSynchronize(st));
  const int64_t nover = (int64_t)h_ctl[0], longest = (int64_t)h_ctl[1];
  if (nover == 0) return CP_OK;
  if (nover > cap) return set_err(CP_EHIP,std::string(who)+": the oversize list overflowed");
  int64_t np = 2;
  while (np < longest) np <<= 1;
  const unsigned gx = (unsigned)std::min<int64_t>((np/2+KS_BLOCK-1)/KS_BLOCK,4096);
  auto step = [&](int64_t k, int64_t j)                    // j = 0: the flip step
    { for (int64_t y0 = 0; y0 < nover; y0 += 65535)        // the grid's second dimension holds 65535 blocks
        { const unsigned gy = (unsigned)std::min<int64_t>(nover-y0,65535);
          ks_step_kernel<<<dim3(gx,gy),KS_BLOCK,0,st>>>(hi,lo,cnt,list+y0,k,j,j == 0);
        }
    };
  for (int64_t k = 2; k <= np; k <<= 1)
    { step(k,0);
      for (int64_t j = k >> 2; j > 0; j >>= 1) step(k,j);
    }
  HIPCHK(hipGetLastError());
  return CP_OK;
}

// the snapshot of the slots that `sel` keeps, for either table; `who` names the entry point in the messages
template <class Tab, class Sel>
static int ks_build(const char *who, Tab *t, cp_kmer_sorted *s, Sel sel, hipStream_t st, void **scratch)
{ const int shift = 2*s->K-s->pbits;
  int rc = ks_alloc(who,(void **)&s->start,(size_t)(s->nb+1)*8,"the bucket counters");
  if (rc != CP_OK) return rc;
  HIPCHK(hipMemsetAsync(s->start,0,(size_t)(s->nb+1)*8,st));
  ks_count_kernel<<<kt_grid(t->slots),KT_BLOCK,0,st>>>(t->tab,t->slots,sel,shift,s->start);
  HIPCHK(hipGetLastError());
  const int nchunk = (int)((s->nb+KS_CHUNK-1)/KS_CHUNK);   // at most 2^24 / KS_CHUNK = KS_CHUNK
  rc = ks_alloc(who,scratch,(size_t)nchunk*8,"the scan's sums");
  if (rc != CP_OK) return rc;
  unsigned long long *sum = (unsigned long long *)*scratch;
  ks_chunk_sum_kernel<<<nchunk,KS_BLOCK,0,st>>>(s->start,s->nb,sum);
  ks_sum_scan_kernel<<<1,KS_BLOCK,0,st>>>(sum,nchunk);
  ks_chunk_scan_kernel<<<nchunk,KS_BLOCK,0,st>>>(s->start,s->nb,sum);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(s->start+s->nb,s->start+s->nb-1,8,hipMemcpyDeviceToDevice,st));
  HIPCHK(hipMemcpyAsync(&s->n,s->start+s->nb-1,8,hipMemcpyDeviceToHost,st));
  HIPCHK(hipStreamSynchronize(st));
  (void)hipFree(*scratch);
  *scratch = nullptr;
  if (s->n == 0) return CP_OK;                             // the starts are all 0 already
  rc = ks_alloc(who,(void **)&s->key,(size_t)s->n*24,"the sorted entries");
  if (rc != CP_OK) return rc;
  unsigned long long *hi = s->key, *lo = s->key+s->n, *cnt = s->key+2*s->n;
  ks_scatter_kernel<<<kt_grid(t->slots),KT_BLOCK,0,st>>>(t->tab,t->slots,sel,shift,s->start,hi,lo,cnt,s->n);
  HIPCHK(hipGetLastError());
  const int64_t ntile = (s->n+KS_TILE-1)/KS_TILE;
  if (ntile > 0x7fffffff) return set_err(CP_EINVAL,std::string(who)+": more than 2^31 tiles");
  ks_tile_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(hi,lo,cnt,s->start,s->nb,s->n);
  HIPCHK(hipGetLastError());
  rc = ks_sort_oversize(who,s,st,scratch);
  if (rc != CP_OK) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return CP_OK;
}

// what both sorts do once their arguments are checked and the table's stream is in order
template <class Tab, class Sel>
static int ks_snapshot(const char *who, Tab *t, Sel sel, hipStream_t st, cp_kmer_sorted **out)
{ cp_kmer_sorted *s = new (std::nothrow) cp_kmer_sorted();
  if (!s) return set_err(CP_ENOMEM,std::string(who)+": out of memory");
  s->K = t->K;
  s->ibyte = cp_ktab_ibyte(t->K);
  s->pbits = s->ibyte ? 8*s->ibyte : 2*t->K;
  s->nb = (int64_t)1 << s->pbits;
  void *scratch = nullptr;
  const int rc = ks_build(who,t,s,sel,st,&scratch);
  if (rc != CP_OK) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  if (rc != CP_OK)
    { cp_kmer_sorted_destroy(s);
      return rc;
    }
  s->ready = true;
  s->filled = s->n;
  *out = s;
  return CP_OK;
}

extern "C" int cp_kmer_counts_sort(cp_kmer_counts *t, int64_t min_count, void *stream, cp_kmer_sorted **out)
{ if (out) *out = nullptr;
  if (!t || !out) return set_err(CP_EINVAL,"cp_kmer_counts_sort: bad argument");
  if (min_count < 1 || min_count > CP_MAX_KMER_CNT)
    return set_err(CP_EINVAL,"cp_kmer_counts_sort: min_count must lie in [1, 32767]");
  if (t->filter && min_count < 2)
    return set_err(CP_EINVAL,"cp_kmer_counts_sort: a filtered table holds no k-mer seen once: min_count must be 2 or more");
  hipStream_t st = (hipStream_t)stream;
  if (t->filter)
    { const int rc = kc_sync_checked(t,"cp_kmer_counts_sort");
      if (rc != CP_OK) return rc;
    }
  else if (t->stream != st) HIPCHK(hipStreamSynchronize(t->stream));
  return ks_snapshot("cp_kmer_counts_sort",t,ks_sel_count{(unsigned long long)min_count},st,out);
}

extern "C" int cp_kmer_table_sort(cp_kmer_table *t, int label, int64_t min_total, int min_pct, void *stream,
                                  cp_kmer_sorted **out)
{ if (out) *out = nullptr;
  if (!t || !out) return set_err(CP_EINVAL,"cp_kmer_table_sort: bad argument");
  if (label < -1 || label > 3) return set_err(CP_EINVAL,"cp_kmer_table_sort: label must lie in [-1, 3]");
  if (min_total < 1 || min_total > CP_MAX_KMER_CNT)
    return set_err(CP_EINVAL,"cp_kmer_table_sort: min_total must lie in [1, 32767]");
  if (min_pct < 0 || min_pct > 100) return set_err(CP_EINVAL,"cp_kmer_table_sort: min_pct must lie in [0, 100]");
  hipStream_t st = (hipStream_t)stream;
  if (t->stream != st) HIPCHK(hipStreamSynchronize(t->stream));
  return ks_snapshot("cp_kmer_table_sort",t,
                     ks_sel_class{label,(unsigned long long)min_total,(unsigned long long)min_pct},st,out);
}

extern "C" int cp_kmer_table_class_hist(cp_kmer_table *t, int64_t *hist, int64_t *ilowcnt, int64_t *ihighcnt)
{ if (!t || !hist || !ilowcnt || !ihighcnt) return set_err(CP_EINVAL,"cp_kmer_table_class_hist: bad argument");
  hipStream_t st = t->stream;
  const size_t cells = 4*((size_t)CP_MAX_KMER_CNT+1), bytes = cells*sizeof(unsigned long long);
  unsigned long long *d_hist = nullptr;
  int rc = ks_alloc("cp_kmer_table_class_hist",(void **)&d_hist,bytes,"the device histogram");
  if (rc != CP_OK) return rc;
  std::vector<unsigned long long> h(cells);
  hipError_t e = hipMemsetAsync(d_hist,0,bytes,st);
  if (e == hipSuccess)
    { ks_class_hist_kernel<<<kt_grid(t->slots),KT_BLOCK,0,st>>>(t->tab,t->slots,d_hist);
      e = hipGetLastError();
    }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(),d_hist,bytes,hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_hist);
  if (e != hipSuccess) return set_err(CP_EHIP,std::string("cp_kmer_table_class_hist: ")+hipGetErrorString(e));
  for (int l = 0; l < 4; l++)
    { const unsigned long long *hl = h.data()+(size_t)l*(CP_MAX_KMER_CNT+1);
      for (int c = 0; c < CP_MAX_KMER_CNT; c++) hist[(size_t)l*CP_MAX_KMER_CNT+c] = (int64_t)hl[c];
      ilowcnt[l] = (int64_t)hl[0];
      ihighcnt[l] = (int64_t)hl[CP_MAX_KMER_CNT];
    }
  return CP_OK;
}

extern "C" int64_t cp_kmer_sorted_size(const cp_kmer_sorted *s)
{ if (!s) return set_err(CP_EINVAL,"cp_kmer_sorted_size: bad argument");
  return s->n;
}

extern "C" int64_t cp_kmer_sorted_bytes(const cp_kmer_sorted *s)
{ if (!s) return set_err(CP_EINVAL,"cp_kmer_sorted_bytes: bad argument");
  return s->n*24+(s->nb+1)*8;
}

extern "C" int cp_kmer_sorted_arrays(const cp_kmer_sorted *s, const uint64_t **d_hi, const uint64_t **d_lo,
                                     const uint64_t **d_cnt)
{ if (!s || !d_hi || !d_lo || !d_cnt) return set_err(CP_EINVAL,"cp_kmer_sorted_arrays: bad argument");
  if (!s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_arrays: the snapshot is still being loaded");
  *d_hi = s->n ? (const uint64_t *)s->key : nullptr;
  *d_lo = s->n ? (const uint64_t *)(s->key+s->n) : nullptr;
  *d_cnt = s->n ? (const uint64_t *)(s->key+2*s->n) : nullptr;
  return CP_OK;
}

extern "C" int cp_kmer_sorted_ktab(cp_kmer_sorted *s, int64_t first, int64_t n, uint8_t *d_records, int64_t *d_index,
                                   void *stream)
{ if (!s) return set_err(CP_EINVAL,"cp_kmer_sorted_ktab: bad argument");
  if (!s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_ktab: the snapshot is still being loaded");
  if (s->ibyte == 0) return set_err(CP_EINVAL,"cp_kmer_sorted_ktab: there is no .ktab for K < 5");
  if (first < 0 || n < 0 || first > s->n || n > s->n-first)
    return set_err(CP_EINVAL,"cp_kmer_sorted_ktab: the range does not lie in the snapshot");
  if (n > 0 && !d_records) return set_err(CP_EINVAL,"cp_kmer_sorted_ktab: null d_records");
  hipStream_t st = (hipStream_t)stream;
  if (d_index) HIPCHK(hipMemcpyAsync(d_index,s->start+1,(size_t)s->nb*8,hipMemcpyDeviceToDevice,st));
  if (n == 0) return CP_OK;
  const int64_t grid = (n+KS_ENC-1)/KS_ENC;
  if (grid > 0x7fffffff) return set_err(CP_EINVAL,"cp_kmer_sorted_ktab: the range is too long for one call");
  ks_encode_kernel<<<(unsigned)grid,KS_ENC,0,st>>>(s->key,s->key+s->n,s->key+2*s->n,first,n,s->K,s->ibyte,d_records);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

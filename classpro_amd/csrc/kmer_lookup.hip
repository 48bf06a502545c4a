// kmer_lookup.hip -- a sorted snapshot as INPUT (tab2prof): a cp_kmer_sorted loaded from the payload of a FASTK .ktab
// (the inverse of cp_kmer_sorted_ktab), and the two queries every ready snapshot answers: the ordinal of a key
// (libfastk.c's Find_Kmer) and the per-read profiles of a batch of reads looked up in it (FastK -p:<table>).  Semantics:
// include/classpro_amd.h, "Sorted k-mers as input"; design: DESIGN.md 9.13.  Included by capi.hip after kmer_sort.hip
// (the snapshot, ks_bucket, ks_alloc, the profile kernel's cell run and store, set_err and HIPCHK are in scope).
//   decode   a block stages its KS_ENC records in LDS as 32-bit words between a byte-wise head and tail (the stores of
//            ks_encode_kernel, turned round).  An entry's prefix is the bucket whose start range holds its ordinal:
//            threads 0 and 1 search the bucket starts for the block's first and last ordinal, the lanes then search
//            only between those two -- a handful of buckets where a bucket holds tens of entries.
//   check    key[i-1] < key[i] for every i; the first offender by a 64-bit atomic min.
//   lookup   bucket = the key's top pbits bits, then a binary search of the bucket's range.  Keys are distinct, so the
//            search ends at the first probe that is equal.  The range is clamped to [0, n] and the loop has a constant
//            bound, so no content of start[] can make a lane run on or read outside the arrays.  LO_ONLY: when
//            2K-63 <= pbits every bit of hi lies in the prefix, so the bucket fixes hi and hi[] is never loaded.
//   group    G searches of one lane advance in lock-step: each step issues its G probes back to back (every load
//            unconditional, an idle search probing entry 0) and only then compares, so a lane keeps G independent
//            misses in flight instead of one.  G = 1 is one search at a time, and the form the build uses: 2 and 4
//            were measured slower and stay for scripts/tabprof_bench.py alone.
//   interp   the first two probes of a search stand to either side of where the key would lie if the suffixes of its
//            bucket were spread evenly; any probe inside the range is a legal pivot, so the bisection simply goes on.
//   profile  the block and lane shape of kc_profile_kernel (KC_CELLS positions per block, kt_walk_all rolls the keys,
//            cells staged in LDS, kc_store_cells); a lane queues the keys of its chunk and searches them G at a time.
#define KL_STEPS 64                        // probes per search at most: enough for any range below 2^63 entries
#define KL_G      1                        // searches of a lane in lock-step (measured: DESIGN.md 9.13)
#define KL_INTERP 1                        // interpolated first probes (measured there too)
#define KL_NEAR   4                        // how far to either side of the interpolated place they stand

struct kl_view                             // what the lookups read of a snapshot
  { const unsigned long long *hi, *lo, *cnt;
    const int64_t *start;
    int64_t n, nb;
    int shift;                             // 2K - pbits
  };

// the largest p in [a, b] with start[p] <= e; start[a] <= e is the caller's
__device__ static inline int64_t kl_bucket_of(const int64_t *start, int64_t a, int64_t b, int64_t e)
{ for (int step = 0; step < 26 && a < b; step++)          // b - a < 2^24
    { const int64_t mid = (a+b+1) >> 1;
      if (start[mid] <= e) a = mid; else b = mid-1;
    }
  return a;
}

__global__ void __launch_bounds__(KS_ENC) kl_decode_kernel(const uint8_t *rec, int64_t first, int64_t n, int K, int ibyte,
                                                           const int64_t *start, int64_t nb, unsigned long long *hi,
                                                           unsigned long long *lo, unsigned long long *cnt)
{ __shared__ __attribute__((aligned(4))) uint8_t stage[KS_ENC*KS_MAXREC+4];
  __shared__ int64_t rng[2];
  const int kbyte = (K+3) >> 2, hbyte = kbyte-ibyte, pbyte = hbyte+2;
  const int64_t b0 = (int64_t)blockIdx.x*KS_ENC;
  const int m = (int)min((int64_t)KS_ENC,n-b0);
  if (m <= 0) return;
  const uint8_t *src = rec+b0*pbyte;
  const int nbytes = m*pbyte;
  const int shift = (int)((uintptr_t)src & 3);            // stage[shift+i] = src[i]: the words are aligned on both sides
  const int head = min(nbytes,(4-shift) & 3);
  const int nw = (nbytes-head) >> 2, tail = head+4*nw;
  if ((int)threadIdx.x < head) stage[shift+threadIdx.x] = src[threadIdx.x];
  for (int w = threadIdx.x; w < nw; w += KS_ENC)
    *(unsigned int *)(stage+shift+head+4*w) = *(const unsigned int *)(src+head+4*w);
  if ((int)threadIdx.x < nbytes-tail) stage[shift+tail+threadIdx.x] = src[tail+threadIdx.x];
  if (threadIdx.x < 2) rng[threadIdx.x] = kl_bucket_of(start,0,nb-1,first+b0+(threadIdx.x ? m-1 : 0));
  __syncthreads();
  if ((int)threadIdx.x >= m) return;
  const int64_t e = first+b0+threadIdx.x;
  const unsigned long long prefix = (unsigned long long)kl_bucket_of(start,rng[0],rng[1],e);
  const uint8_t *o = stage+shift+(int)threadIdx.x*pbyte;
  kt_u128 key = prefix;
  for (int b = 0; b < hbyte; b++) key = (key << 8) | (kt_u128)o[b];
  key >>= 8*kbyte-2*K;                                    // the pad bits of the last byte
  hi[e] = (unsigned long long)(key >> 63);
  lo[e] = (unsigned long long)key & KT_M63;
  cnt[e] = (unsigned long long)o[hbyte] | ((unsigned long long)o[hbyte+1] << 8);
}

__global__ void __launch_bounds__(KT_BLOCK) kl_check_kernel(const unsigned long long *hi, const unsigned long long *lo,
                                                            int64_t n, unsigned long long *bad)
{ for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x+1; i < n; i += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long ah = hi[i-1], bh = hi[i];
      if (!(ah < bh || (ah == bh && lo[i-1] < lo[i]))) atomicMin(bad,(unsigned long long)i);
    }
}

// pos[g] = the ordinal of the key (qh[g], ql[g]) for g < nq, or -1: G searches in lock-step (see the file comment).
// INTERP: the first two probes of a range of more than 2*KL_NEAR entries stand KL_NEAR entries to either side of where
// the key would lie if the suffixes of a bucket were spread evenly; the bisection goes on from whatever they leave.
template <bool LO_ONLY, bool INTERP, int G>
__device__ static inline void kl_find_group(const kl_view &t, const unsigned long long (&qh)[G],
                                            const unsigned long long (&ql)[G], int nq, int64_t (&pos)[G])
{ int64_t a[G], e[G], guess[G];
#pragma unroll
  for (int g = 0; g < G; g++)
    { const unsigned long long b = ks_bucket(qh[g],ql[g],t.shift);
      const bool in = g < nq && ql[g] <= KT_M63 && b < (unsigned long long)t.nb;
      const unsigned long long at = in ? b : 0;
      a[g] = min(max(t.start[at],(int64_t)0),t.n);
      e[g] = in ? min(max(t.start[at+1],(int64_t)0),t.n) : a[g];
      pos[g] = -1;
      guess[g] = -1;
      if (INTERP && e[g]-a[g] > 2*KL_NEAR && e[g]-a[g] < ((int64_t)1 << 31))
        { const kt_u128 suffix = ((((kt_u128)qh[g]) << 63) | (kt_u128)ql[g]) & ((((kt_u128)1) << t.shift)-1);
          const unsigned long long f = t.shift >= 32 ? (unsigned long long)(suffix >> (t.shift-32))
                                                     : (unsigned long long)suffix << (32-t.shift);      // below 2^32
          guess[g] = a[g]+(int64_t)((f*(unsigned long long)(e[g]-a[g])) >> 32);
        }
    }
  for (int step = 0; step < KL_STEPS; step++)
    { bool any = false;
#pragma unroll
      for (int g = 0; g < G; g++) any |= a[g] < e[g];
      if (!any) break;                                    // a live search has a < e <= n: entry 0 exists
      unsigned long long kh[G], kl[G];
      int64_t mid[G];
#pragma unroll
      for (int g = 0; g < G; g++)
        { mid[g] = (a[g]+e[g]) >> 1;
          if (INTERP && step < 2 && guess[g] >= 0)
            mid[g] = min(max(guess[g]+(step ? KL_NEAR : -KL_NEAR),a[g]),e[g]-1);
          const int64_t at = a[g] < e[g] ? mid[g] : 0;
          kl[g] = t.lo[at];
          kh[g] = LO_ONLY ? 0 : t.hi[at];
        }
#pragma unroll
      for (int g = 0; g < G; g++)
        { if (a[g] >= e[g]) continue;
          const bool eq = kl[g] == ql[g] && (LO_ONLY || kh[g] == qh[g]);
          const bool less = LO_ONLY ? kl[g] < ql[g] : (kh[g] < qh[g] || (kh[g] == qh[g] && kl[g] < ql[g]));
          if (eq) { pos[g] = mid[g]; e[g] = a[g]; }
          else if (less) a[g] = mid[g]+1;
          else e[g] = mid[g];
        }
    }
}

template <bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) kl_find_kernel(kl_view t, const unsigned long long *qhi,
                                                           const unsigned long long *qlo, int64_t m, int64_t *out)
{ for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < m; i += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long qh[1] = { qhi[i] }, ql[1] = { qlo[i] };
      int64_t pos[1];
      kl_find_group<LO_ONLY,KL_INTERP != 0,1>(t,qh,ql,1,pos);
      out[i] = pos[0];
    }
}

// tally: present, absent, other bytes -- per lane, summed per wave, one atomic per wave and counter
template <bool CANON, bool LO_ONLY, bool INTERP, int G>
__global__ void __launch_bounds__(KT_BLOCK) kl_profile_kernel(kl_view t, const char *seq, const int64_t *seq_off,
                                                              const int64_t *prof_off, int nreads, int64_t total, int K,
                                                              uint16_t *prof, unsigned long long *tally)
{ __shared__ uint16_t cell[KC_CELLS];
  __shared__ int64_t run[2];
  const int64_t b0 = (int64_t)blockIdx.x*KC_CELLS, b1 = min(b0+(int64_t)KC_CELLS,total);
  kc_cell_run(seq_off,prof_off,nreads,total,K,b0,b1,run);
  __syncthreads();
  const int64_t q0 = run[0];
  const int64_t n = min(max(run[1]-q0,(int64_t)0),min((int64_t)KC_CELLS,prof_off[nreads]-q0));
  const int64_t p0 = b0+(int64_t)threadIdx.x*KT_CHUNK;
  unsigned long long npres = 0, nabs = 0, noth = 0;
  unsigned long long qh[G], ql[G];
  int qi[G], nq = 0;                                     // a queued key's cell in the stage, -1: outside it
#pragma unroll
  for (int g = 0; g < G; g++) { qh[g] = 0; ql[g] = 0; qi[g] = -1; }
  auto flush = [&]()
    { int64_t pos[G];
      kl_find_group<LO_ONLY,INTERP,G>(t,qh,ql,nq,pos);
      unsigned long long c[G];
#pragma unroll
      for (int g = 0; g < G; g++) c[g] = t.n > 0 ? t.cnt[max(pos[g],(int64_t)0)] : 0;
#pragma unroll
      for (int g = 0; g < G; g++)
        { if (g >= nq) continue;
          npres += pos[g] >= 0;
          nabs += pos[g] < 0;
          if (qi[g] >= 0) cell[qi[g]] = pos[g] >= 0 ? (uint16_t)min(c[g],(unsigned long long)CP_MAX_KMER_CNT) : (uint16_t)0;
        }
      nq = 0;
    };
  int cur = -1;                                          // the read whose cell base is held
  int64_t base = 0;
  if (p0 < total)
    { kt_walk_all<CANON>(seq,seq_off,nreads,total,K,p0,
        [&](int r, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
        { if (r != cur) { cur = r; base = prof_off[r]-seq_off[r]-(K-1)-q0; }
          const int64_t i = base+j;
          const bool in = (unsigned long long)i < (unsigned long long)n;
          if (!ok)
            { noth++;
              if (in) cell[i] = 0;
              return;
            }
#pragma unroll
          for (int g = 0; g < G; g++)
            if (g == nq) { qh[g] = hi; ql[g] = lo; qi[g] = in ? (int)i : -1; }
          if (++nq == G) flush();
        });
      if (nq) flush();
    }
  if (tally)
    { kc_wave_add(tally,npres);
      kc_wave_add(tally+1,nabs);
      kc_wave_add(tally+2,noth);
    }
  __syncthreads();
  if (n <= 0) return;
  kc_store_cells(cell,prof+q0,n);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

static kl_view kl_view_of(const cp_kmer_sorted *s)
{ return kl_view{ s->key, s->key+s->n, s->key+2*s->n, s->start, s->n, s->nb, 2*s->K-s->pbits }; }

static bool kl_lo_only(const cp_kmer_sorted *s)
{ return 2*s->K-63 <= s->pbits; }

extern "C" int cp_kmer_sorted_load_begin(int K, const int64_t *index, cp_kmer_sorted **out)
{ if (out) *out = nullptr;
  if (!index || !out) return set_err(CP_EINVAL,"cp_kmer_sorted_load_begin: bad argument");
  if (K < 5 || K > 63)
    return set_err(CP_EINVAL,"cp_kmer_sorted_load_begin: K must lie in [5, 63] (a k-mer table has one to three prefix bytes)");
  cp_kmer_sorted *s = new (std::nothrow) cp_kmer_sorted();
  if (!s) return set_err(CP_ENOMEM,"cp_kmer_sorted_load_begin: out of memory");
  s->K = K;
  s->ibyte = cp_ktab_ibyte(K);
  s->pbits = 8*s->ibyte;
  s->nb = (int64_t)1 << s->pbits;
  std::vector<int64_t> start((size_t)s->nb+1);
  start[0] = 0;
  for (int64_t p = 0; p < s->nb; p++)
    { if (index[p] < start[(size_t)p])
        { delete s;
          char m[160];
          snprintf(m,sizeof(m),"cp_kmer_sorted_load_begin: the index is negative or decreases at prefix %lld",(long long)p);
          return set_err(CP_EINVAL,m);
        }
      start[(size_t)p+1] = index[p];
    }
  s->n = start[(size_t)s->nb];
  if (s->n > ((int64_t)1 << 56))
    { delete s;
      return set_err(CP_EINVAL,"cp_kmer_sorted_load_begin: the index ends past 2^56 entries");
    }
  int rc = ks_alloc("cp_kmer_sorted_load_begin",(void **)&s->start,(size_t)(s->nb+1)*8,"the bucket starts");
  if (rc == CP_OK && s->n > 0)
    rc = ks_alloc("cp_kmer_sorted_load_begin",(void **)&s->key,(size_t)s->n*24,"the sorted entries");
  if (rc == CP_OK)
    { const hipError_t e = hipMemcpy(s->start,start.data(),(size_t)(s->nb+1)*8,hipMemcpyHostToDevice);
      if (e != hipSuccess) rc = set_err(CP_EHIP,std::string("cp_kmer_sorted_load_begin: ")+hipGetErrorString(e));
    }
  if (rc != CP_OK)
    { cp_kmer_sorted_destroy(s);
      return rc;
    }
  *out = s;
  return CP_OK;
}

extern "C" int cp_kmer_sorted_load_records(cp_kmer_sorted *s, int64_t n, const uint8_t *d_records, void *stream)
{ if (!s || n < 0) return set_err(CP_EINVAL,"cp_kmer_sorted_load_records: bad argument");
  if (s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_load_records: the snapshot is not being loaded");
  if (n > s->n-s->filled)
    { char m[200];
      snprintf(m,sizeof(m),"cp_kmer_sorted_load_records: %lld entries after %lld run past the %lld of the index",(long long)n,
               (long long)s->filled,(long long)s->n);
      return set_err(CP_EINVAL,m);
    }
  if (n == 0) return CP_OK;
  if (!d_records) return set_err(CP_EINVAL,"cp_kmer_sorted_load_records: null d_records");
  const int64_t grid = (n+KS_ENC-1)/KS_ENC;
  if (grid > 0x7fffffff) return set_err(CP_EINVAL,"cp_kmer_sorted_load_records: the piece is too long for one call");
  kl_decode_kernel<<<(unsigned)grid,KS_ENC,0,(hipStream_t)stream>>>(d_records,s->filled,n,s->K,s->ibyte,s->start,s->nb,s->key,
                                                                    s->key+s->n,s->key+2*s->n);
  HIPCHK(hipGetLastError());
  s->filled += n;
  return CP_OK;
}

extern "C" int cp_kmer_sorted_load_end(cp_kmer_sorted *s, void *stream)
{ if (!s) return set_err(CP_EINVAL,"cp_kmer_sorted_load_end: bad argument");
  if (s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_load_end: the snapshot is not being loaded");
  if (s->filled != s->n)
    { char m[160];
      snprintf(m,sizeof(m),"cp_kmer_sorted_load_end: %lld of %lld entries were appended",(long long)s->filled,(long long)s->n);
      return set_err(CP_EINVAL,m);
    }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long bad = ~0ull, *d_bad = nullptr;
  if (s->n > 1)
    { const int rc = ks_alloc("cp_kmer_sorted_load_end",(void **)&d_bad,8,"the check's result");
      if (rc != CP_OK) return rc;
      hipError_t e = hipMemcpyAsync(d_bad,&bad,8,hipMemcpyHostToDevice,st);
      if (e == hipSuccess)
        { kl_check_kernel<<<kt_grid((unsigned long long)s->n),KT_BLOCK,0,st>>>(s->key,s->key+s->n,s->n,d_bad);
          e = hipGetLastError();
        }
      if (e == hipSuccess) e = hipMemcpyAsync(&bad,d_bad,8,hipMemcpyDeviceToHost,st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      (void)hipFree(d_bad);
      if (e != hipSuccess) return set_err(CP_EHIP,std::string("cp_kmer_sorted_load_end: ")+hipGetErrorString(e));
    }
  else HIPCHK(hipStreamSynchronize(st));
  if (bad != ~0ull)
    { char m[160];
      snprintf(m,sizeof(m),"cp_kmer_sorted_load_end: entry %llu is not above the entry before it",bad);
      return set_err(CP_EINVAL,m);
    }
  s->ready = true;
  return CP_OK;
}

extern "C" int cp_kmer_sorted_find(const cp_kmer_sorted *s, const uint64_t *d_hi, const uint64_t *d_lo, int64_t m,
                                   int64_t *d_pos, void *stream)
{ if (!s || m < 0) return set_err(CP_EINVAL,"cp_kmer_sorted_find: bad argument");
  if (!s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_find: the snapshot is still being loaded");
  if (m == 0) return CP_OK;
  if (!d_hi || !d_lo || !d_pos) return set_err(CP_EINVAL,"cp_kmer_sorted_find: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  const kl_view t = kl_view_of(s);
  const unsigned long long *qh = (const unsigned long long *)d_hi, *ql = (const unsigned long long *)d_lo;
  if (kl_lo_only(s)) kl_find_kernel<true><<<kt_grid((unsigned long long)m),KT_BLOCK,0,st>>>(t,qh,ql,m,d_pos);
  else kl_find_kernel<false><<<kt_grid((unsigned long long)m),KT_BLOCK,0,st>>>(t,qh,ql,m,d_pos);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

extern "C" int cp_kmer_sorted_profiles(const cp_kmer_sorted *s, int canonical, const char *d_seq, const int64_t *d_seq_off,
                                       const int64_t *d_prof_off, int nreads, int64_t total_bases, uint16_t *d_prof,
                                       int64_t *d_tally, void *stream)
{ if (!s || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_sorted_profiles: bad argument");
  if (!s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_profiles: the snapshot is still being loaded");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off || !d_prof_off || !d_prof)
    return set_err(CP_EINVAL,"cp_kmer_sorted_profiles: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = (int)((total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS);
  const kl_view t = kl_view_of(s);
  unsigned long long *tally = (unsigned long long *)d_tally;
  int g = KL_G, ip = KL_INTERP;                            // A/B knobs of scripts/tabprof_bench.py
  if (const char *e = getenv("CLASSPRO_TABPROF_LOCKSTEP")) g = atoi(e);
  if (const char *e = getenv("CLASSPRO_TABPROF_INTERP")) ip = atoi(e);
  if (g != 1 && g != 2 && g != 4) return set_err(CP_EINVAL,"cp_kmer_sorted_profiles: CLASSPRO_TABPROF_LOCKSTEP must be 1, 2 or 4");
  if (g != 1) ip = 0;                                      // the interpolated probes were tried on the form that was kept
#define KL_PROF(C,L,I,G) kl_profile_kernel<C,L,I,G><<<grid,KT_BLOCK,0,st>>>(t,d_seq,d_seq_off,d_prof_off,nreads,total_bases, \
                                                                          s->K,d_prof,tally)
#define KL_PROF_G(C,L) do { if (g == 4) KL_PROF(C,L,false,4); else if (g == 2) KL_PROF(C,L,false,2); \
                            else if (ip) KL_PROF(C,L,true,1); else KL_PROF(C,L,false,1); } while (0)
  if (canonical) { if (kl_lo_only(s)) KL_PROF_G(true,true); else KL_PROF_G(true,false); }
  else { if (kl_lo_only(s)) KL_PROF_G(false,true); else KL_PROF_G(false,false); }
#undef KL_PROF_G
#undef KL_PROF
  HIPCHK(hipGetLastError());
  return CP_OK;
}

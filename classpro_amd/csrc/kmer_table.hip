// kmer_table.hip -- per-k-mer label table on the device (class2cns): how often each distinct k-mer of a labelled batch
// got each of the labels E/H/D/R, the consensus label per k-mer and the consistency figure of the reference's
// scripts/agg2cons.py.  Semantics: include/classpro_amd.h, "Per-k-mer label table".  Included by capi.hip (set_err,
// HIPCHK and the library's error contract are shared).  This file holds what is the label table's own: slot, counters,
// the add, statistics, consensus and export kernels and their entry points.
//
// The table is open addressing with linear probing, one 32-byte slot per key: hi = key bits 125..63, lo = key bits
// 62..0, four u32 counts.  Keys, the hash, the claim protocol, the lookup and the walk over a batch's k-mers are shared
// with the count table (kmer_counts.hip): kt_common.h.  An insert finds or claims its key's slot and adds one count; one
// that runs past the probe bound (KT_PROBE) sets its position's bit in a failure bitmap and adds nothing.  The host then
// grows the table (rehash into at least twice the slots) and replays exactly the failed positions: kt_store.h, which
// holds the life cycle of both tables (creation, growth, the add driver, destruction).
#include "kt_store.h"

#define KT_ERR_LABEL    1u                 // a counted position held a label other than E/H/D/R
#define KT_ERR_OVERFLOW 2u                 // a count passed 2^32-1

struct kt_slot { unsigned long long hi, lo; unsigned int cnt[4]; };          // cnt in label order E, H, D, R

struct kt_ctl                                                                 // device-side counters of one table
  { unsigned long long n_fail, n_occ, n_skip, n_rfail;                        // the store's: kt_store.h
    unsigned long long n_out;             // export: entries written
    unsigned int err, pad;
  };

struct kt_part                                                                // one block's share of the statistics
  { unsigned long long n_distinct, n_unanimous, label_total[4], cns_total[4], s_hi, s_lo; };

__device__ static inline int kt_label(unsigned char c)                       // E H D R -> 0..3, anything else -1
{ return c == 'E' ? 0 : c == 'H' ? 1 : c == 'D' ? 2 : c == 'R' ? 3 : -1; }

// consensus label: the largest count; a tie goes to the larger copy number, R > D > H > E
__host__ __device__ static inline int kt_consensus(const unsigned int *c)
{ int best = 0;
  for (int l = 1; l < 4; l++)
    if (c[l] >= c[best]) best = l;
  return best;
}

// One add pass (REPLAY = false) or a replay of the positions whose bit is set in fail_in (REPLAY = true).
template <bool CANON, bool REPLAY>
__global__ void __launch_bounds__(KT_BLOCK) kt_add_kernel(kt_slot *tab, unsigned long long mask, const char *seq,
                                                          const int64_t *seq_off, const char *labels, int nreads,
                                                          int64_t total, int K, const unsigned int *fail_in,
                                                          unsigned int *fail_out, kt_ctl *ctl)
{ const int64_t p0 = ((int64_t)blockIdx.x*blockDim.x+threadIdx.x)*KT_CHUNK;
  if (p0 >= total) return;
  unsigned long long nfail = 0, nocc = 0;
  unsigned int err = 0;
  const unsigned long long nskip = kt_walk<CANON>(seq,seq_off,nreads,total,K,p0,
    [&](int64_t j, unsigned long long hi, unsigned long long lo)
    { if (REPLAY && !((fail_in[j >> 5] >> (j & 31)) & 1u)) return;
      const int l = kt_label((unsigned char)labels[j]);
      if (l < 0) { err |= KT_ERR_LABEL; return; }
      bool claimed = false;
      kt_slot *e = kt_find_or_claim(tab,mask,hi,lo,&claimed);
      nocc += claimed;
      if (!e)
        { atomicOr(&fail_out[j >> 5],1u << (j & 31));
          nfail++;
          return;
        }
      if (atomicAdd(&e->cnt[l],1u) == 0xFFFFFFFFu) err |= KT_ERR_OVERFLOW;
    });
  if (nfail) atomicAdd(&ctl->n_fail,nfail);
  if (nocc) atomicAdd(&ctl->n_occ,nocc);
  if (!REPLAY && nskip) atomicAdd(&ctl->n_skip,nskip);
  if (err) atomicOr(&ctl->err,err);
}

// per-block partial statistics over the occupied slots (integer sums only: the result does not depend on the order)
__global__ void __launch_bounds__(KT_BLOCK) kt_stats_kernel(const kt_slot *tab, unsigned long long n, kt_part *parts)
{ kt_part a = {};
  for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < n;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const kt_slot e = tab[s];
      if (e.lo == KT_EMPTY) continue;
      unsigned long long tot = 0, mx = 0;
      for (int l = 0; l < 4; l++)
        { tot += e.cnt[l];
          mx = max(mx,(unsigned long long)e.cnt[l]);
          a.label_total[l] += e.cnt[l];
        }
      a.n_distinct++;
      a.n_unanimous += (tot == mx);
      a.cns_total[kt_consensus(e.cnt)] += tot;
      // floor(tot * 2^64 / mx) = q * 2^64 + floor(r * 2^64 / mx), the fraction by two 32-bit long-division steps
      // (mx < 2^32, r < mx)
      const unsigned long long q = tot/mx, r = tot%mx;
      const unsigned long long a1 = r << 32, q1 = a1/mx, r1 = a1%mx, q2 = (r1 << 32)/mx;
      const unsigned long long frac = (q1 << 32) | q2;
      a.s_lo += frac;
      a.s_hi += q+(a.s_lo < frac);
    }
  __shared__ kt_part sh[KT_BLOCK];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = KT_BLOCK/2; w > 0; w >>= 1)
    { if ((int)threadIdx.x < w)
        { kt_part &x = sh[threadIdx.x];
          const kt_part &y = sh[threadIdx.x+w];
          x.n_distinct += y.n_distinct;
          x.n_unanimous += y.n_unanimous;
          for (int l = 0; l < 4; l++) { x.label_total[l] += y.label_total[l]; x.cns_total[l] += y.cns_total[l]; }
          x.s_lo += y.s_lo;
          x.s_hi += y.s_hi+(x.s_lo < y.s_lo);
        }
      __syncthreads();
    }
  if (threadIdx.x == 0) parts[blockIdx.x] = sh[0];
}

// consensus labels: out[j] = the consensus label of the k-mer ending at j; skipped k-mers keep what out holds
template <bool CANON>
__global__ void __launch_bounds__(KT_BLOCK) kt_consensus_kernel(const kt_slot *tab, unsigned long long mask,
                                                                const char *seq, const int64_t *seq_off, int nreads,
                                                                int64_t total, int K, char *out, kt_ctl *ctl)
{ const int64_t p0 = ((int64_t)blockIdx.x*blockDim.x+threadIdx.x)*KT_CHUNK;
  if (p0 >= total) return;
  unsigned int err = 0;
  kt_walk<CANON>(seq,seq_off,nreads,total,K,p0,
    [&](int64_t j, unsigned long long hi, unsigned long long lo)
    { const kt_slot *e = kt_lookup(tab,mask,hi,lo);
      if (!e) { err |= KT_ERR_LABEL; return; }           // a k-mer that was never added: the caller's error
      out[j] = "EHDR"[kt_consensus(e->cnt)];
    });
  if (err) atomicOr(&ctl->err,err);
}

__global__ void __launch_bounds__(KT_BLOCK) kt_export_kernel(const kt_slot *tab, unsigned long long n, kt_slot *out,
                                                             unsigned long long cap, kt_ctl *ctl)
{ for (unsigned long long s = (unsigned long long)blockIdx.x*blockDim.x+threadIdx.x; s < n;
       s += (unsigned long long)gridDim.x*blockDim.x)
    { const kt_slot e = tab[s];
      if (e.lo == KT_EMPTY) continue;
      const unsigned long long i = atomicAdd(&ctl->n_out,1ull);
      if (i < cap) out[i] = e;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

struct cp_kmer_table : kt_store<kt_slot,kt_ctl>
  { int canonical;
    bool overflowed;                     // sticky: a count passed 2^32-1
  };

extern "C" int cp_kmer_table_create(int K, int canonical, int64_t initial_slots, cp_kmer_table **out)
{ if (!out) return set_err(CP_EINVAL,"cp_kmer_table_create: null out");
  *out = nullptr;
  if (K < 2 || K > 63)
    return set_err(CP_EINVAL,"cp_kmer_table_create: K must lie in [2, 63] (a key holds 2K <= 126 bits)");
  if (initial_slots < 0 || initial_slots > ((int64_t)1 << 40))
    return set_err(CP_EINVAL,"cp_kmer_table_create: bad initial_slots");
  cp_kmer_table *t = new (std::nothrow) cp_kmer_table();
  if (!t) return set_err(CP_ENOMEM,"cp_kmer_table_create: out of memory");
  t->canonical = canonical ? 1 : 0;
  const int rc = kt_init(t,"cp_kmer_table",K,initial_slots);
  if (rc != CP_OK)
    { cp_kmer_table_destroy(t);
      return rc;
    }
  *out = t;
  return CP_OK;
}

extern "C" void cp_kmer_table_destroy(cp_kmer_table *t)
{ if (!t) return;
  kt_free(t);
  delete t;
}

extern "C" int cp_kmer_table_add(cp_kmer_table *t, const char *d_seq, const int64_t *d_seq_off, const char *d_labels,
                                 int nreads, int64_t total_bases, void *stream)
{ if (!t || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_table_add: bad argument");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off || !d_labels) return set_err(CP_EINVAL,"cp_kmer_table_add: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  const int grid = (int)((total_bases+(int64_t)KT_BLOCK*KT_CHUNK-1)/((int64_t)KT_BLOCK*KT_CHUNK));
  return kt_add(t,total_bases,st,nullptr,[&](bool replay, const unsigned int *fail_in, unsigned int *fail_out)
    {
#define KT_ADD(C,R) kt_add_kernel<C,R><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,d_labels,nreads,total_bases, \
                                                               t->K,fail_in,fail_out,t->ctl)
      if (t->canonical) { if (replay) KT_ADD(true,true); else KT_ADD(true,false); }
      else { if (replay) KT_ADD(false,true); else KT_ADD(false,false); }
#undef KT_ADD
    });
}

// n_distinct * 2^64 / S, correctly rounded (S >= n_distinct * 2^64 > 0): 64 significant quotient bits by restoring
// division, then round half to even on the dropped bits and the remainder
static double kt_ratio(unsigned long long n, unsigned long long s_hi, unsigned long long s_lo)
{ const kt_u128 S = ((kt_u128)s_hi << 64) | s_lo;
  kt_u128 r = (kt_u128)n << 64;
  unsigned long long m = 0;
  int e = 0, nbits = 0;
  // the quotient lies in [1/4, 1]: its leading bit is at 2^0, 2^-1 or 2^-2
  if (r >= S) { m = 1; r -= S; nbits = 1; }
  while (nbits < 64)
    { r <<= 1;
      e--;
      const unsigned long long bit = r >= S;
      if (bit) r -= S;
      if (nbits > 0 || bit) { m = (m << 1) | bit; nbits++; }
    }
  // value = m * 2^e, m has 64 significant bits; keep 53
  const unsigned long long drop = m & 0x7ff;
  m >>= 11;
  e += 11;
  if (drop > 0x400 || (drop == 0x400 && (r != 0 || (m & 1)))) m++;
  if (m == (1ull << 53)) { m >>= 1; e++; }
  return ldexp((double)m,e);
}

extern "C" int cp_kmer_table_stats(cp_kmer_table *t, cp_kmer_stats *out)
{ if (!t || !out) return set_err(CP_EINVAL,"cp_kmer_table_stats: bad argument");
  hipStream_t st = t->stream;
  const int grid = kt_grid(t->slots);
  std::vector<kt_part> parts((size_t)grid);
  kt_part *d_parts = nullptr;
  HIPCHK(hipMalloc(&d_parts,sizeof(kt_part)*grid));
  kt_stats_kernel<<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots,d_parts);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(parts.data(),d_parts,sizeof(kt_part)*grid,hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipMemcpyAsync(t->h_ctl,t->ctl,sizeof(kt_ctl),hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_parts);
  if (e != hipSuccess) return set_err(CP_EHIP,std::string("cp_kmer_table_stats: ")+hipGetErrorString(e));
  const unsigned int err = t->h_ctl->err;
  if (err)                                                  // deferred device errors: reported once, then cleared
    { HIPCHK(hipMemsetAsync(&t->ctl->err,0,sizeof(unsigned int),st));
      HIPCHK(hipStreamSynchronize(st));
    }
  if (err & KT_ERR_OVERFLOW) t->overflowed = true;
  if (t->overflowed)
    return set_err(CP_EOVERFLOW,"cp_kmer_table: a k-mer's count of one label passed 2^32-1; the table is no longer exact");
  if (err & KT_ERR_LABEL)
    return set_err(CP_EINVAL,"cp_kmer_table: a counted k-mer position held a label other than E/H/D/R, or a consensus "
                             "pass met a k-mer that was never added");
  kt_part a = {};
  for (const kt_part &p : parts)
    { a.n_distinct += p.n_distinct;
      a.n_unanimous += p.n_unanimous;
      for (int l = 0; l < 4; l++) { a.label_total[l] += p.label_total[l]; a.cns_total[l] += p.cns_total[l]; }
      a.s_lo += p.s_lo;
      a.s_hi += p.s_hi+(a.s_lo < p.s_lo);
    }
  memset(out,0,sizeof(*out));
  out->n_skipped = (int64_t)t->h_ctl->n_skip;
  out->n_distinct = (int64_t)a.n_distinct;
  out->n_unanimous = (int64_t)a.n_unanimous;
  for (int l = 0; l < 4; l++)
    { out->label_total[l] = (int64_t)a.label_total[l];
      out->cns_total[l] = (int64_t)a.cns_total[l];
      out->n_kmers += out->label_total[l];
    }
  out->s_fixed_hi = a.s_hi;
  out->s_fixed_lo = a.s_lo;
  out->consistency = a.n_distinct ? kt_ratio(a.n_distinct,a.s_hi,a.s_lo) : NAN;
  out->slots = (int64_t)t->slots;
  out->bytes = (int64_t)(t->slots*sizeof(kt_slot)+2*t->fail_words*4);
  out->growths = t->growths;
  return CP_OK;
}

extern "C" int cp_kmer_table_consensus(cp_kmer_table *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                                       int64_t total_bases, char *d_labels, void *stream)
{ if (!t || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,"cp_kmer_table_consensus: bad argument");
  if (nreads == 0 || total_bases == 0) return CP_OK;
  if (!d_seq || !d_seq_off || !d_labels) return set_err(CP_EINVAL,"cp_kmer_table_consensus: null device pointer");
  hipStream_t st = (hipStream_t)stream;
  t->stream = st;
  const int grid = (int)((total_bases+(int64_t)KT_BLOCK*KT_CHUNK-1)/((int64_t)KT_BLOCK*KT_CHUNK));
  if (t->canonical)
    kt_consensus_kernel<true><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,nreads,total_bases,t->K,
                                                      d_labels,t->ctl);
  else
    kt_consensus_kernel<false><<<grid,KT_BLOCK,0,st>>>(t->tab,t->slots-1,d_seq,d_seq_off,nreads,total_bases,t->K,
                                                       d_labels,t->ctl);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

extern "C" int64_t cp_kmer_table_export(cp_kmer_table *t, uint64_t *hi, uint64_t *lo, uint32_t *counts4,
                                        int64_t capacity)
{ if (!t || capacity < 0) return set_err(CP_EINVAL,"cp_kmer_table_export: bad argument");
  hipStream_t st = t->stream;
  int rc = kt_sync_ctl(t,st);
  if (rc != CP_OK) return rc;
  const unsigned long long n = t->h_ctl->n_occ;
  if ((unsigned long long)capacity < n || !hi || !lo || !counts4) return (int64_t)n;
  if (n == 0) return 0;
  kt_slot *d_out = nullptr;
  if (hipMalloc(&d_out,(size_t)n*sizeof(kt_slot)) != hipSuccess)
    { (void)hipGetLastError();
      return set_err(CP_ENOMEM,"cp_kmer_table_export: cannot allocate the export buffer");
    }
  std::vector<kt_slot> h((size_t)n);
  hipError_t e = hipMemsetAsync(&t->ctl->n_out,0,sizeof(unsigned long long),st);
  if (e == hipSuccess)
    { kt_export_kernel<<<kt_grid(t->slots),KT_BLOCK,0,st>>>(t->tab,t->slots,d_out,n,t->ctl);
      e = hipGetLastError();
    }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(),d_out,(size_t)n*sizeof(kt_slot),hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_out);
  if (e != hipSuccess) return set_err(CP_EHIP,std::string("cp_kmer_table_export: ")+hipGetErrorString(e));
  std::sort(h.begin(),h.end(),[](const kt_slot &a, const kt_slot &b)
            { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; });
  for (size_t i = 0; i < (size_t)n; i++)
    { hi[i] = h[i].hi;
      lo[i] = h[i].lo;
      for (int l = 0; l < 4; l++) counts4[4*i+l] = h[i].cnt[l];
    }
  return (int64_t)n;
}

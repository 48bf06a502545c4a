// kmer_fixes.hip -- the gaps of a batch of reads in one sorted snapshot, the one edit that closes a gap where there is one,
// and the pass that applies such edits (tabfix).  Semantics: include/classpro_amd.h, "Fixing reads from a k-mer table";
// design: DESIGN.md 9.23; the rule: fx_rule.h.  Included by capi.hip after kmer_runs.hip (the snapshot, kl_view,
// kl_find_group, kr_state_kernel, kr_scan_kernel, kr_write_kernel, the ks_* scan kernels, kc_wave_add, KC_CELLS, set_err
// and HIPCHK are in scope).  The snapshot and the batch are only read.
//   gaps     the state bytes, block summaries, scan and write pass of kmer_runs.hip with one table, skip = 0 and
//            emit = 1 << CP_RUN_NONE: a NONE run is a gap, and its kr_rec (32 bytes) is written where its cp_kmer_fix
//            (32 bytes) will stand.
//   fix      fx_fix_kernel, one wave per gap, four gaps per block.  The wave stages the codes of the bases
//            s[i, i+2K+2) once in LDS -- every edited window lies in them -- and decides open or closed from the two
//            bytes s[i-1] and s[j+K] and the read's bounds.  Per candidate, lane l packs the K bases of the k-mer at
//            checked position i+l of the edited window (the edit spliced in by index, nothing is rolled), takes the smaller
//            of it and its reverse complement, and makes one kl_find_group<.,.,1> search with the range test; a __ballot
//            over the lanes decides.  A window of more than 64 k-mers (K = 63 with an insertion) takes a second round; a
//            candidate stops at the first round with an absent k-mer.  Lane 0 replaces the record.
//   clash    two passes of one lane per record: fx_clash_kernel reads first, read, status and del of its record and of the
//            two beside it and leaves its decision in a spare byte of its own record; fx_status_kernel turns the decisions
//            into statuses and sums the tally per wave before any atomic.  No lane reads what a lane of its pass stores.
//   apply    fx_delta_kernel turns every record into its signed length change (0 for whatever is no edit), the
//            three-kernel scan of kmer_sort.hip makes it inclusive over all records, fx_offsets_kernel makes it relative
//            per read and adds the read's start.  fx_copy_kernel has the lane and block shape of the state kernel: a lane
//            owns 64 consecutive bases of the batch, finds their read, begins an fx_walk there (a binary search in the
//            read's records) and takes its bases one by one.  A base that an edit inserts before is written by the lane
//            that owns that base.  No lane is serial over more than its 64 bases and the records of FX_BACK gaps.
// Every record field and every output base is stored exactly once and nothing but the tally is added to in memory.
#include "fx_rule.h"

#define FX_WAVES (KT_BLOCK/64)             // gaps per block of the fix kernel
#define FX_MAXREC ((int64_t)KS_CHUNK*KS_CHUNK)          // records per call: what one level of the scan of apply_fixes holds
#define FX_STAGE 192                       // staged bases per gap: K-1 + FX_MAXD + K-1 <= 128 are used, three rounds are staged

static_assert(sizeof(fx_fix) == 32 && sizeof(kr_rec) == 32,"a gap is written as a run and replaced by its fix in place");
static_assert(2*63+2 <= FX_STAGE && FX_STAGE == 3*64,"the stage holds every edited window");

template <bool CANON, bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) fx_fix_kernel(kl_view t, unsigned long long amin, unsigned long long amax, int D,
                                                          const char *seq, const int64_t *seq_off, int nreads, int K,
                                                          fx_fix *fix, int64_t nfix)
{ __shared__ uint8_t code_of[FX_WAVES][FX_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t k = (int64_t)blockIdx.x*FX_WAVES+wave;
  const bool live = k < nfix;
  uint8_t *code = code_of[wave];
  int64_t i = 0, j = 0, rs = 0, n = 0;
  int r = 0;
  if (live)
    { const kr_rec in = ((const kr_rec *)fix)[k];
      i = in.first; j = in.last;
      r = min(max(in.read,0),nreads-1);
      rs = seq_off[r];
      n = seq_off[r+1]-rs;
#pragma unroll
      for (int x = lane; x < FX_STAGE; x += 64)
        { const int64_t p = i+x;
          const int b = (p >= 0 && p < n) ? kt_base((unsigned char)seq[rs+p]) : -1;
          code[x] = (uint8_t)(b < 0 ? 4 : b);
        }
    }
  __syncthreads();                                         // the one barrier: the stage of every wave is written
  if (!live) return;
  const int64_t e = fx_e(i,K);
  const bool closed = i >= 1 && j+K <= n-1 && i+K <= n && kt_base((unsigned char)seq[rs+i-1]) >= 0
                      && kt_base((unsigned char)seq[rs+j+K]) >= 0;
  fx_fix out;
  out.first = i; out.last = j; out.read = r;
  out.status = FX_OPEN; out.del = 0; out.nins = 0; out.nacc = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) out.ins[c] = 0;
  if (closed)
    { const int64_t g = fx_g(i,j,K);
      const int nc = fx_ncand(g,D);
      char near[5];
#pragma unroll
      for (int c = 0; c < 5; c++) near[c] = "ACGTN"[code[K-1-4+c]];
      const kt_u128 kmask = (((kt_u128)1) << (2*K))-1;
      const int rshift = 2*K-2;
      int nexist = 0, nacc = 0;
      fx_edit won;
      won.del = 0; won.nins = 0;
      for (int c = 0; c < FX_MAXD; c++) won.ins[c] = 0;
      for (int c = 0; c < nc; c++)
        { const fx_edit ed = fx_cand(c,g,D,near);
          if (!fx_exists(e,ed.del,n)) continue;
          nexist++;
          int64_t q0, q1;
          fx_window(i,K,ed.del,ed.nins,n,&q0,&q1);
          const int W = (int)min(q1-q0+1,(int64_t)(K-1+FX_MAXD));      // q0 == i: the gap is closed
          bool good = W > 0;
          for (int base = 0; base < W && good; base += 64)
            { const int l = base+lane;
              const bool active = l < W;
              kt_u128 fw = 0, rc = 0;
              bool ok = active;
              if (active)
                for (int b = 0; b < K; b++)                // base l+b of the edited window, which begins at base i of the read
                  { const int x = l+b;
                    int v;
                    if (x < K-1) v = code[x];
                    else if (x < K-1+ed.nins) v = kt_base((unsigned char)ed.ins[x-(K-1)]);
                    else v = code[min(x-ed.nins+ed.del,FX_STAGE-1)];
                    if (v < 0 || v > 3) { ok = false; v = 0; }
                    fw = ((fw << 2) | (kt_u128)v) & kmask;
                    rc = (rc >> 2) | (((kt_u128)(3-v)) << rshift);
                  }
              const kt_u128 key = (CANON && rc < fw) ? rc : fw;
              const unsigned long long qh[1] = { (unsigned long long)(key >> 63) }, ql[1] = { (unsigned long long)key & KT_M63 };
              int64_t pos[1];
              kl_find_group<LO_ONLY,KL_INTERP != 0,1>(t,qh,ql,ok ? 1 : 0,pos);
              bool present = false;
              if (ok && pos[0] >= 0)
                { const unsigned long long cnt = t.cnt[pos[0]];
                  present = cnt >= amin && cnt <= amax;
                }
              if (__ballot(active && !present) != 0) good = false;
            }
          if (good)
            { if (nacc == 0) won = ed;
              nacc++;
            }
        }
      out.nacc = (uint8_t)nacc;
      out.status = (uint8_t)(nexist == 0 ? FX_NOCAND : nacc == 0 ? FX_NONE : nacc == 1 ? FX_ONE : FX_MANY);
      if (nacc == 1)
        { out.del = (uint8_t)won.del; out.nins = (uint8_t)won.nins;
          for (int c = 0; c < FX_MAXD; c++) out.ins[c] = won.ins[c];
        }
    }
  if (lane == 0) fix[k] = out;
}

// The clash rule in two passes, so that no lane reads what another lane of the same pass stores.  fx_clash_kernel reads of its
// own record and of the two beside it only first, read, status and del, none of which it stores, and leaves its decision in
// the record's last ins byte, which holds no base (nins <= FX_MAXD < 8) and which no lane of this pass reads.
__global__ void __launch_bounds__(KT_BLOCK) fx_clash_kernel(fx_fix *fix, int64_t nfix, int K)
{ const int64_t k = (int64_t)blockIdx.x*KT_BLOCK+threadIdx.x;
  if (k >= nfix || fix[k].status != FX_ONE) return;
  const int64_t e = fx_e(fix[k].first,K);
  const int32_t read = fix[k].read;
  bool clash = false;
  if (k > 0 && fix[k-1].read == read && fix[k-1].status == FX_ONE) clash |= fx_clash(fx_e(fix[k-1].first,K),fix[k-1].del,e);
  if (k+1 < nfix && fix[k+1].read == read && fix[k+1].status == FX_ONE) clash |= fx_clash(e,fix[k].del,fx_e(fix[k+1].first,K));
  if (clash) fix[k].ins[7] = 1;
}

// the decisions become statuses; the tally by final status, summed per wave before any atomic
__global__ void __launch_bounds__(KT_BLOCK) fx_status_kernel(fx_fix *fix, int64_t nfix, unsigned long long *tally)
{ const int64_t k = (int64_t)blockIdx.x*KT_BLOCK+threadIdx.x;
  int status = -1;
  if (k < nfix)
    { status = fix[k].status;
      if (fix[k].ins[7])
        { status = FX_CLASH;
          fix[k].status = (uint8_t)FX_CLASH;
          fix[k].ins[7] = 0;
        }
    }
  if (tally)
    for (int s = 0; s < 6; s++) kc_wave_add(tally+s,status == s ? 1ull : 0ull);
}

// ---- applying ----

// the records [lo, hi) of read r, whatever fix_off holds
__device__ static inline void fx_records_of(const int64_t *fix_off, int r, int64_t nfix, int64_t *lo, int64_t *hi)
{ *lo = min(max(fix_off[r],(int64_t)0),nfix);
  *hi = max(*lo,min(max(fix_off[r+1],(int64_t)0),nfix));
}

__global__ void __launch_bounds__(KT_BLOCK) fx_delta_kernel(const fx_fix *fix, const int64_t *fix_off, const int64_t *seq_off,
                                                            int nreads, int K, int64_t nfix, int64_t *cum)
{ const int64_t k = (int64_t)blockIdx.x*KT_BLOCK+threadIdx.x;
  if (k >= nfix) return;
  const fx_fix x = fix[k];
  const int r = min(max(x.read,0),nreads-1);
  int64_t lo, hi;
  fx_records_of(fix_off,r,nfix,&lo,&hi);
  const int64_t n = seq_off[r+1]-seq_off[r];
  cum[k] = (k >= lo && k < hi) ? fx_delta(x,r,n,K) : 0;
}

// out_off[r] = seq_off[r] + the length changes of the records before those of read r; out_off[nreads] the new total
__global__ void __launch_bounds__(KT_BLOCK) fx_offsets_kernel(const int64_t *cum, const int64_t *fix_off, const int64_t *seq_off,
                                                              int nreads, int64_t nfix, int64_t *out_off)
{ const int64_t r = (int64_t)blockIdx.x*KT_BLOCK+threadIdx.x;
  if (r > nreads) return;
  const int64_t lo = r < nreads ? min(max(fix_off[r],(int64_t)0),nfix) : nfix;
  out_off[r] = seq_off[r]+fx_excl(cum,lo);
}

__global__ void __launch_bounds__(KT_BLOCK) fx_copy_kernel(const char *seq, const int64_t *seq_off, int nreads, int64_t total,
                                                           int K, const fx_fix *fix, const int64_t *fix_off, int64_t nfix,
                                                           const int64_t *cum, const int64_t *out_off, char *out,
                                                           int64_t out_capacity)
{ const int64_t p0 = (int64_t)blockIdx.x*KC_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  if (p0 >= total) return;
  const int64_t p1 = min(p0+(int64_t)KT_CHUNK,total);
  int r = kr_read_of(seq_off,nreads,p0);
  for (int64_t p = p0; p < p1 && r < nreads; r++)
    { const int64_t rs = seq_off[r], re = seq_off[r+1];
      if (re <= p) continue;                               // empty reads
      const int64_t q1 = min(p1,re), n = re-rs;
      int64_t lo, hi;
      fx_records_of(fix_off,r,nfix,&lo,&hi);
      const int64_t o0 = out_off[r], olen = out_off[r+1]-o0;
      fx_walk w = fx_walk_begin(fix,cum,lo,hi,r,n,K,p-rs);
      for (int64_t q = p; q < q1; q++)
        fx_walk_step(w,fix,q-rs,seq[q],[&](int64_t o, char ch)
          { const int64_t at = o0+o;
            if (o >= 0 && o < olen && at >= 0 && at < out_capacity) out[at] = ch;
          });
      p = q1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

extern "C" int cp_kmer_sorted_read_fixes(const cp_kmer_sorted *s, int canonical, const int64_t *range, int max_indel,
                                         const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases,
                                         cp_kmer_fix *d_fixes, int64_t capacity, int64_t *d_fix_off, int64_t *total,
                                         int64_t *d_tally, void *stream)
{ const char *who = "cp_kmer_sorted_read_fixes";
  static_assert(sizeof(cp_kmer_fix) == sizeof(fx_fix) && sizeof(fx_fix) == 32,"a fix is 32 bytes");
  static_assert(CP_FIX_NONE == FX_NONE && CP_FIX_ONE == FX_ONE && CP_FIX_MANY == FX_MANY && CP_FIX_OPEN == FX_OPEN
                && CP_FIX_NOCAND == FX_NOCAND && CP_FIX_CLASH == FX_CLASH,"the statuses of the header are those of fx_rule.h");
  if (!s || !total || nreads < 0 || total_bases < 0 || capacity < 0) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!s->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (s->K < 5 || s->K > 63) return set_err(CP_EINVAL,std::string(who)+": K must lie in [5, 63]");      // near[] of fx_cand: s[e-4 .. e]
  if (max_indel < 0 || max_indel > FX_MAXD) return set_err(CP_EINVAL,std::string(who)+": max_indel must lie in [0, 4]");
  kh_range rg{ 1, (unsigned long long)INT64_MAX, 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0]) return set_err(CP_EINVAL,std::string(who)+": a count range needs 1 <= min <= max");
      rg.amin = (unsigned long long)range[0]; rg.amax = (unsigned long long)range[1];
    }
  if ((capacity > 0 && !d_fixes) || (nreads > 0 && (!d_fix_off || !d_seq_off)) || (total_bases > 0 && !d_seq))
    return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  const int64_t nblk = nreads > 0 ? (total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS : 0;
  if (nblk > 0x3fffffff) return set_err(CP_EINVAL,std::string(who)+": the batch is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  const unsigned int skip = 0, emit = 1u << CP_RUN_NONE;
  // one allocation, before anything is queued: the block summaries and the sum of all, then a state byte per base
  const size_t nsum = ((size_t)nblk+1)*sizeof(kr_sum), bytes = nsum+(size_t)total_bases;
  uint8_t *scratch = nullptr;
  if (nblk > 0 && (hipMalloc((void **)&scratch,bytes) != hipSuccess || !scratch))
    { (void)hipGetLastError();
      char m[160];
      snprintf(m,sizeof(m),"%s: cannot allocate %zu bytes for the states and the block summaries",who,bytes);
      return set_err(CP_ENOMEM,m);
    }
  *total = 0;
  if (d_fix_off)
    { const hipError_t e0 = hipMemsetAsync(d_fix_off,0,((size_t)nreads+1)*sizeof(int64_t),st);
      if (e0 != hipSuccess)
        { (void)hipStreamSynchronize(st);
          if (scratch) (void)hipFree(scratch);
          return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e0));
        }
    }
  if (nblk == 0)
    { HIPCHK(hipStreamSynchronize(st));
      return CP_OK;
    }
  kr_sum *part = (kr_sum *)scratch;
  uint8_t *state = scratch+nsum;                           // nsum is a multiple of 32
  const kl_view ta = kl_view_of(s);
  const int K = s->K;
  const bool lo_only = kl_lo_only(s);
#define FX_STATE(C,L) kr_state_kernel<C,L,L,false><<<(unsigned)nblk,KT_BLOCK,0,st>>>(ta,ta,rg,skip,emit,d_seq,d_seq_off,nreads, \
                                                                                  total_bases,K,state,part)
  if (canonical) { if (lo_only) FX_STATE(true,true); else FX_STATE(true,false); }
  else { if (lo_only) FX_STATE(false,true); else FX_STATE(false,false); }
#undef FX_STATE
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    { kr_scan_kernel<<<1,KT_BLOCK,0,st>>>(part,nblk,emit);
      e = hipGetLastError();
    }
  int64_t n = 0;                                           // the gaps: known before the records are written, so that a call
  if (e == hipSuccess) e = hipMemcpyAsync(&n,&part[nblk].heads,sizeof(int64_t),hipMemcpyDeviceToHost,st);   // that overflows
  if (e == hipSuccess) e = hipStreamSynchronize(st);                                                        // writes none
  if (e == hipSuccess && n > FX_MAXREC)                    // what cp_apply_fixes takes in one call: refused here, not there
    { (void)hipFree(scratch);
      *total = n;
      char m[200];
      snprintf(m,sizeof(m),"%s: %lld gaps in one call, more than %lld: pass fewer bases per call",who,(long long)n,(long long)FX_MAXREC);
      return set_err(CP_EINVAL,m);
    }
  const bool fits = n <= capacity;
  if (e == hipSuccess)
    { kr_write_kernel<<<(unsigned)nblk,KT_BLOCK,0,st>>>(state,part,skip,emit,d_seq_off,nreads,total_bases,K,(kr_rec *)d_fixes,
                                                       fits ? capacity : 0,d_fix_off);
      e = hipGetLastError();
    }
  if (e == hipSuccess && fits && n > 0)
    { const int64_t grid = (n+FX_WAVES-1)/FX_WAVES;
      if (grid > 0x7fffffff) e = hipErrorInvalidValue;
      else
        {
#define FX_FIX(C,L) fx_fix_kernel<C,L><<<(unsigned)grid,KT_BLOCK,0,st>>>(ta,rg.amin,rg.amax,max_indel,d_seq,d_seq_off,nreads,K, \
                                                                        (fx_fix *)d_fixes,n)
          if (canonical) { if (lo_only) FX_FIX(true,true); else FX_FIX(true,false); }
          else { if (lo_only) FX_FIX(false,true); else FX_FIX(false,false); }
#undef FX_FIX
          e = hipGetLastError();
        }
      if (e == hipSuccess)
        { fx_clash_kernel<<<(unsigned)((n+KT_BLOCK-1)/KT_BLOCK),KT_BLOCK,0,st>>>((fx_fix *)d_fixes,n,K);
          fx_status_kernel<<<(unsigned)((n+KT_BLOCK-1)/KT_BLOCK),KT_BLOCK,0,st>>>((fx_fix *)d_fixes,n,(unsigned long long *)d_tally);
          e = hipGetLastError();
        }
    }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  const hipError_t ef = hipFree(scratch);
  if (e == hipSuccess) e = ef;
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  *total = n;
  if (!fits)
    { char m[160];
      snprintf(m,sizeof(m),"%s: %lld fixes do not fit the %lld of d_fixes",who,(long long)n,(long long)capacity);
      return set_err(CP_EOVERFLOW,m);
    }
  return CP_OK;
}

extern "C" int cp_apply_fixes(const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases, int K,
                              const cp_kmer_fix *d_fixes, const int64_t *d_fix_off, char *d_out, int64_t out_capacity,
                              int64_t *d_out_off, int64_t *out_total, void *stream)
{ const char *who = "cp_apply_fixes";
  if (!out_total || nreads < 0 || total_bases < 0 || out_capacity < 0 || K < 5 || K > 63)
    return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if ((nreads > 0 && (!d_seq_off || !d_fix_off || !d_out_off)) || (total_bases > 0 && !d_seq) || (out_capacity > 0 && !d_out))
    return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  hipStream_t st = (hipStream_t)stream;
  *out_total = 0;
  if (nreads == 0)
    { if (d_out_off) HIPCHK(hipMemsetAsync(d_out_off,0,sizeof(int64_t),st));
      HIPCHK(hipStreamSynchronize(st));
      return CP_OK;
    }
  int64_t nfix = 0;
  HIPCHK(hipMemcpyAsync(&nfix,d_fix_off+nreads,sizeof(int64_t),hipMemcpyDeviceToHost,st));
  HIPCHK(hipStreamSynchronize(st));
  if (nfix < 0 || nfix > ((int64_t)1 << 40)) return set_err(CP_EINVAL,std::string(who)+": d_fix_off does not end in a number of records");
  if (nfix > 0 && !d_fixes) return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  const int64_t nblk = (total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS;
  if (nblk > 0x3fffffff) return set_err(CP_EINVAL,std::string(who)+": the batch is too long for one call");
  // one allocation: the scanned length changes, one per record, and the chunk sums of the scan
  const int64_t nchunk = (nfix+KS_CHUNK-1)/KS_CHUNK;
  if (nfix > FX_MAXREC) return set_err(CP_EINVAL,std::string(who)+": more than 2^24 records in one call");
  const size_t bytes = ((size_t)nfix+(size_t)nchunk+1)*sizeof(int64_t);
  int64_t *cum = nullptr;
  if (hipMalloc((void **)&cum,bytes) != hipSuccess || !cum)
    { (void)hipGetLastError();
      char m[160];
      snprintf(m,sizeof(m),"%s: cannot allocate %zu bytes for the scan of the length changes",who,bytes);
      return set_err(CP_ENOMEM,m);
    }
  unsigned long long *sum = (unsigned long long *)(cum+nfix);
  const fx_fix *fix = (const fx_fix *)d_fixes;
  hipError_t e = hipSuccess;
  if (nfix > 0)
    { fx_delta_kernel<<<(unsigned)((nfix+KT_BLOCK-1)/KT_BLOCK),KT_BLOCK,0,st>>>(fix,d_fix_off,d_seq_off,nreads,K,nfix,cum);
      ks_chunk_sum_kernel<<<(unsigned)nchunk,KS_BLOCK,0,st>>>(cum,nfix,sum);
      ks_sum_scan_kernel<<<1,KS_BLOCK,0,st>>>(sum,(int)nchunk);
      ks_chunk_scan_kernel<<<(unsigned)nchunk,KS_BLOCK,0,st>>>(cum,nfix,sum);
      e = hipGetLastError();
    }
  if (e == hipSuccess)
    { fx_offsets_kernel<<<(unsigned)(((int64_t)nreads+1+KT_BLOCK-1)/KT_BLOCK),KT_BLOCK,0,st>>>(cum,d_fix_off,d_seq_off,nreads,nfix,
                                                                                               d_out_off);
      e = hipGetLastError();
    }
  int64_t n_out = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&n_out,d_out_off+nreads,sizeof(int64_t),hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const bool fits = n_out <= out_capacity;
  if (e == hipSuccess && fits && nblk > 0)
    { fx_copy_kernel<<<(unsigned)nblk,KT_BLOCK,0,st>>>(d_seq,d_seq_off,nreads,total_bases,K,fix,d_fix_off,nfix,cum,d_out_off,d_out,
                                                      out_capacity);
      e = hipGetLastError();
    }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  const hipError_t ef = hipFree(cum);
  if (e == hipSuccess) e = ef;
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  *out_total = n_out;
  if (!fits)
    { char m[160];
      snprintf(m,sizeof(m),"%s: %lld bases do not fit the %lld of d_out",who,(long long)n_out,(long long)out_capacity);
      return set_err(CP_EOVERFLOW,m);
    }
  return CP_OK;
}

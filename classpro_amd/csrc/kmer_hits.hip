// kmer_hits.hip -- two sorted snapshots looked at together (tabbin): per read, how many k-mer positions carry a key only in
// A, only in B, in both, or hold another byte, and how often the A/B markers switch sides along the read.  Semantics:
// include/classpro_amd.h, "Read hits in two sorted k-mer sets"; design: DESIGN.md 9.15.  Included by capi.hip after
// kmer_lookup.hip (the snapshot, kl_view, kl_find_group, ks_bucket, KC_CELLS, set_err and HIPCHK are in scope).  Both
// snapshots are only read.
//   summary  of a run of positions of ONE read: (first marker, last marker, switches, nA, nB, nBoth, nOther).  Two
//            summaries join by adding the counts, plus one switch when the left's last and the right's first marker are
//            both set and differ; an empty side passes the other's first or last marker through.  The operator is
//            associative and not commutative, and the empty summary is its identity.  Packed: the four counts in 16 bits
//            each (a block holds KC_CELLS = 2^14 positions) and first | last << 2 | switches << 4 in a 32-bit word.
//   lane     rolls the keys of its KT_CHUNK positions once (kt_walk_all), looks each key up in both tables and keeps the
//            summary of the read it is in, in registers.  A read that begins AND ends inside the chunk is finished there:
//            its row is stored at once.  What is left is at most a HEAD (the read that was already under way at the
//            chunk's first position) and a TAIL (the read still under way at its last); a lane that lies inside one read
//            has one summary that is both (a SPAN lane).
//   block    a segmented scan over the lanes in order: a SPAN lane joins its summary to the carry, every other lane
//            resets the carry to its tail (empty when no read is under way at its end).  The carry that reaches a lane
//            joined with its head is the whole of that read inside the block: the row itself when the read's first k-mer
//            position lies in the block, otherwise the block's ENTER partial.  The carry that leaves the last lane is the
//            block's LEAVE partial, or -- all lanes SPAN, one read covering the block -- an ENTER partial marked COVER.
//            So a block leaves two partials at most, and a block or lane without an A or B marker passes the last marker
//            through because the empty summary does.  The scan is six shuffle steps per wave and a word per wave in LDS.
//   stitch   a second kernel, one wave per block: where a block's ENTER partial ends a read, the wave joins the LEAVE
//            partial of the read's first block, the COVER partials between and that ENTER partial in block order (a
//            contiguous share per lane, then the 64 shares in lane order) and stores the row.  A read of n blocks costs n
//            16-byte loads there, never a walk over its positions.
//   lookup   kl_find_group per table, one after the other, or kh_find_pair: the two searches of one key in lock-step,
//            their probes issued back to back before either is compared (kl_find_group's idea with a view per search).
//            Clamped ranges, the constant probe bound, LO_ONLY per table and the interpolated first probes as there.
// Rows are first set to zero (reads without a k-mer position get nothing else), then every other row is stored exactly
// once: nothing is added to, so a row does not depend on the batch, the read order or the block and chunk sizes.
#define KH_LOCKSTEP 0                      // the two searches of a key in lock-step (measured: DESIGN.md 9.15)
#define KH_A        1u                     // markers; 0 is none
#define KH_B        2u
#define KH_COVER    0x80000000u            // in the meta word of an ENTER partial: the read also leaves the block

struct kh_sum { unsigned long long cnt; unsigned int meta; };

struct kh_part                             // a block's partial summary of a read that crosses a block edge
  { int read;                              // -1: none
    unsigned int meta;
    unsigned long long cnt;
  };

struct kh_range { unsigned long long amin, amax, bmin, bmax; };

__device__ static inline kh_sum kh_join(kh_sum l, kh_sum r)
{ const unsigned int lf = l.meta & 3, ll = (l.meta >> 2) & 3, rf = r.meta & 3, rl = (r.meta >> 2) & 3;
  const unsigned int sw = (l.meta >> 4)+(r.meta >> 4)+((ll && rf && ll != rf) ? 1u : 0u);
  return kh_sum{ l.cnt+r.cnt, (lf ? lf : rf) | ((rl ? rl : ll) << 2) | (sw << 4) };
}

__device__ static inline void kh_store_row(int64_t *hits, int nreads, int r, kh_sum s)
{ if ((unsigned int)r >= (unsigned int)nreads) return;
  int64_t *o = hits+(int64_t)r*CP_HIT_WIDTH;
  o[CP_HIT_A] = (int64_t)(s.cnt & 0xffff);
  o[CP_HIT_B] = (int64_t)((s.cnt >> 16) & 0xffff);
  o[CP_HIT_BOTH] = (int64_t)((s.cnt >> 32) & 0xffff);
  o[CP_HIT_OTHER] = (int64_t)(s.cnt >> 48);
  o[CP_HIT_SWITCHES] = (int64_t)((s.meta & ~KH_COVER) >> 4);
}

// pos[0], pos[1] = the ordinal of the key (qh, ql) in ta and in tb, or -1: the two searches in lock-step
template <bool LO_A, bool LO_B, bool INTERP>
__device__ static inline void kh_find_pair(const kl_view &ta, const kl_view &tb, unsigned long long qh,
                                           unsigned long long ql, int64_t (&pos)[2])
{ int64_t a[2], e[2], guess[2];
#pragma unroll
  for (int g = 0; g < 2; g++)
    { const kl_view &t = g ? tb : ta;
      const unsigned long long b = ks_bucket(qh,ql,t.shift);
      const bool in = ql <= KT_M63 && b < (unsigned long long)t.nb;
      const unsigned long long at = in ? b : 0;
      a[g] = min(max(t.start[at],(int64_t)0),t.n);
      e[g] = in ? min(max(t.start[at+1],(int64_t)0),t.n) : a[g];
      pos[g] = -1;
      guess[g] = -1;
      if (INTERP && e[g]-a[g] > 2*KL_NEAR && e[g]-a[g] < ((int64_t)1 << 31))
        { const kt_u128 suffix = ((((kt_u128)qh) << 63) | (kt_u128)ql) & ((((kt_u128)1) << t.shift)-1);
          const unsigned long long f = t.shift >= 32 ? (unsigned long long)(suffix >> (t.shift-32))
                                                     : (unsigned long long)suffix << (32-t.shift);      // below 2^32
          guess[g] = a[g]+(int64_t)((f*(unsigned long long)(e[g]-a[g])) >> 32);
        }
    }
  for (int step = 0; step < KL_STEPS; step++)
    { if (a[0] >= e[0] && a[1] >= e[1]) break;             // a live search has a < e <= n: entry 0 exists
      unsigned long long kh[2], kl[2];
      int64_t mid[2];
#pragma unroll
      for (int g = 0; g < 2; g++)
        { const kl_view &t = g ? tb : ta;
          mid[g] = (a[g]+e[g]) >> 1;
          if (INTERP && step < 2 && guess[g] >= 0)
            mid[g] = min(max(guess[g]+(step ? KL_NEAR : -KL_NEAR),a[g]),e[g]-1);
          const bool live = a[g] < e[g];
          const int64_t at = live ? mid[g] : 0;
          kl[g] = live ? t.lo[at] : 0;
          kh[g] = ((g ? LO_B : LO_A) || !live) ? 0 : t.hi[at];
        }
#pragma unroll
      for (int g = 0; g < 2; g++)
        { if (a[g] >= e[g]) continue;
          const bool lo_only = g ? LO_B : LO_A;
          const bool eq = kl[g] == ql && (lo_only || kh[g] == qh);
          const bool less = lo_only ? kl[g] < ql : (kh[g] < qh || (kh[g] == qh && kl[g] < ql));
          if (eq) { pos[g] = mid[g]; e[g] = a[g]; }
          else if (less) a[g] = mid[g]+1;
          else e[g] = mid[g];
        }
    }
}

template <bool CANON, bool LO_A, bool LO_B, bool LOCK>
__global__ void __launch_bounds__(KT_BLOCK) kh_hits_kernel(kl_view ta, kl_view tb, kh_range rg, const char *seq,
                                                           const int64_t *seq_off, int nreads, int64_t total, int K,
                                                           int64_t *hits, kh_part *part)
{ __shared__ kh_sum wave_v[KT_BLOCK/64];
  __shared__ unsigned int wave_f[KT_BLOCK/64];
  const int64_t b0 = (int64_t)blockIdx.x*KC_CELLS;
  const int64_t p0 = b0+(int64_t)threadIdx.x*KT_CHUNK;
  if (threadIdx.x == 0)
    { part[2*(int64_t)blockIdx.x] = kh_part{ -1, 0, 0 };
      part[2*(int64_t)blockIdx.x+1] = kh_part{ -1, 0, 0 };
    }
  // ---- the lane: one summary in registers, closed whenever the read changes ----
  int cur = -1, head_r = -1;                               // the read under way; the read of the head, once it is closed
  bool cur_open = false;                                   // the read under way began before this chunk
  unsigned long long cnt = 0;
  unsigned int first = 0, last = 0, sw = 0;
  kh_sum head{ 0, 0 };
  int64_t last_j = -1;
  auto packed = [&]() { return kh_sum{ cnt, first | (last << 2) | (sw << 4) }; };
  if (p0 < total)
    kt_walk_all<CANON>(seq,seq_off,nreads,total,K,p0,
      [&](int r, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
      { if (r != cur)
          { if (cur >= 0)
              { if (cur_open) { head = packed(); head_r = cur; }
                else kh_store_row(hits,nreads,cur,packed());
              }
            cur = r;
            cur_open = j > seq_off[r]+(K-1);
            cnt = 0; first = 0; last = 0; sw = 0;
          }
        last_j = j;
        if (!ok) { cnt += 1ull << 48; return; }
        int64_t pos[2];
        if (LOCK) kh_find_pair<LO_A,LO_B,KL_INTERP != 0>(ta,tb,hi,lo,pos);
        else
          { const unsigned long long qh[1] = { hi }, ql[1] = { lo };
            int64_t pa[1], pb[1];
            kl_find_group<LO_A,KL_INTERP != 0,1>(ta,qh,ql,1,pa);
            kl_find_group<LO_B,KL_INTERP != 0,1>(tb,qh,ql,1,pb);
            pos[0] = pa[0]; pos[1] = pb[0];
          }
        const unsigned long long ca = pos[0] >= 0 ? ta.cnt[pos[0]] : 0, cb = pos[1] >= 0 ? tb.cnt[pos[1]] : 0;
        const bool in_a = pos[0] >= 0 && ca >= rg.amin && ca <= rg.amax;
        const bool in_b = pos[1] >= 0 && cb >= rg.bmin && cb <= rg.bmax;
        if (in_a && in_b) cnt += 1ull << 32;
        else if (in_a || in_b)
          { const unsigned int m = in_a ? KH_A : KH_B;
            cnt += in_a ? 1ull : 1ull << 16;
            sw += last && last != m;
            if (!first) first = m;
            last = m;
          }
      });
  const bool leaves = cur >= 0 && last_j+1 < min(seq_off[cur+1],total);    // the read under way goes on past this chunk
  const bool span = leaves && cur_open;
  kh_sum v{ 0, 0 };                                        // what the lane hands on: its tail, or its all when it spans
  if (leaves) v = packed();
  else if (cur_open) { head = packed(); head_r = cur; }
  else if (cur >= 0) kh_store_row(hits,nreads,cur,packed());
  const bool have_head = head_r >= 0;
  // ---- the block: inclusive segmented scan of (reset, v) over the lanes ----
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int f = span ? 0u : 1u;
  kh_sum inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
    { const unsigned long long uc = __shfl_up(inc.cnt,d);
      const unsigned int um = __shfl_up(inc.meta,d), uf = __shfl_up(f,d);
      if (lane >= d)
        { if (!f) inc = kh_join(kh_sum{ uc, um },inc);
          f |= uf;
        }
    }
  unsigned long long ec = __shfl_up(inc.cnt,1);            // the same, exclusive
  unsigned int em = __shfl_up(inc.meta,1), ef = __shfl_up(f,1);
  if (lane == 0) { ec = 0; em = 0; ef = 0; }
  if (lane == 63) { wave_v[wave] = inc; wave_f[wave] = f; }
  __syncthreads();                                         // also orders thread 0's empty partials before the real ones
  kh_sum before{ 0, 0 };                                   // the carry that reaches this wave
  for (int w = 0; w < wave; w++) before = wave_f[w] ? wave_v[w] : kh_join(before,wave_v[w]);
  const kh_sum carry = ef ? kh_sum{ ec, em } : kh_join(before,kh_sum{ ec, em });
  if (have_head)                                           // the read of the head ends in this lane
    { const kh_sum whole = kh_join(carry,head);
      if (seq_off[head_r]+(K-1) >= b0) kh_store_row(hits,nreads,head_r,whole);
      else part[2*(int64_t)blockIdx.x] = kh_part{ head_r, whole.meta, whole.cnt };
    }
  if (threadIdx.x == KT_BLOCK-1 && leaves)                 // the read under way at the block's last position
    { const kh_sum out = f ? inc : kh_join(before,inc);
      if (seq_off[cur]+(K-1) >= b0) part[2*(int64_t)blockIdx.x+1] = kh_part{ cur, out.meta, out.cnt };
      else part[2*(int64_t)blockIdx.x] = kh_part{ cur, out.meta | KH_COVER, out.cnt };
    }
}

struct kh_wide { long long c[4], sw; unsigned int first, last; };

__device__ static inline void kh_wide_add(kh_wide &l, const kh_wide &r)
{ for (int k = 0; k < 4; k++) l.c[k] += r.c[k];
  l.sw += r.sw+((l.last && r.first && l.last != r.first) ? 1 : 0);
  if (!l.first) l.first = r.first;
  if (r.last) l.last = r.last;
}

// block b: when its ENTER partial ends a read, the row of that read from the partials of its blocks, in block order
__global__ void __launch_bounds__(64) kh_stitch_kernel(const kh_part *part, const int64_t *seq_off, int nreads, int K,
                                                       int64_t *hits)
{ __shared__ kh_wide share[64];
  const int64_t b = blockIdx.x;
  const kh_part end = part[2*b];
  if (end.read < 0 || end.read >= nreads || (end.meta & KH_COVER)) return;
  const int r = end.read;
  const int64_t bs = min(max((seq_off[r]+(K-1))/(int64_t)KC_CELLS,(int64_t)0),b);    // the block of r's first k-mer position
  const int64_t n = b-bs+1, per = (n+63)/64;
  kh_wide acc{ { 0, 0, 0, 0 }, 0, 0, 0 };
  const int64_t i1 = min(n,((int64_t)threadIdx.x+1)*per);
  for (int64_t i = (int64_t)threadIdx.x*per; i < i1; i++)
    { const int64_t blk = bs+i;
      const kh_part p = part[2*blk+((i == 0 && blk < b) ? 1 : 0)];
      if (p.read != r) continue;                           // cannot happen while the batch is only read
      const kh_wide w{ { (long long)(p.cnt & 0xffff), (long long)((p.cnt >> 16) & 0xffff), (long long)((p.cnt >> 32) & 0xffff),
                         (long long)(p.cnt >> 48) }, (long long)((p.meta & ~KH_COVER) >> 4), p.meta & 3, (p.meta >> 2) & 3 };
      kh_wide_add(acc,w);
    }
  share[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int l = 1; l < 64; l++) kh_wide_add(acc,share[l]);
  int64_t *o = hits+(int64_t)r*CP_HIT_WIDTH;
  o[CP_HIT_A] = acc.c[0]; o[CP_HIT_B] = acc.c[1]; o[CP_HIT_BOTH] = acc.c[2]; o[CP_HIT_OTHER] = acc.c[3];
  o[CP_HIT_SWITCHES] = acc.sw;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

extern "C" int cp_kmer_sorted_read_hits(const cp_kmer_sorted *a, const cp_kmer_sorted *b, int canonical,
                                        const int64_t *range, const char *d_seq, const int64_t *d_seq_off, int nreads,
                                        int64_t total_bases, int64_t *d_hits, void *stream)
{ const char *who = "cp_kmer_sorted_read_hits";
  if (!a || !b || nreads < 0 || total_bases < 0) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!a->ready || !b->ready) return set_err(CP_EINVAL,std::string(who)+": a snapshot is still being loaded");
  if (a->K != b->K)
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
  int lock = KH_LOCKSTEP;                                  // A/B knob of scripts/readhits_bench.py
  if (const char *e = getenv("CLASSPRO_READHITS_LOCKSTEP")) lock = atoi(e);
  if (lock != 0 && lock != 1) return set_err(CP_EINVAL,std::string(who)+": CLASSPRO_READHITS_LOCKSTEP must be 0 or 1");
  if (nreads == 0) return CP_OK;
  if (!d_hits || !d_seq_off || (total_bases > 0 && !d_seq)) return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  const int64_t nblk = (total_bases+(int64_t)KC_CELLS-1)/(int64_t)KC_CELLS;
  if (nblk > 0x3fffffff) return set_err(CP_EINVAL,std::string(who)+": the batch is too long for one call");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(d_hits,0,(size_t)nreads*CP_HIT_WIDTH*sizeof(int64_t),st));
  if (nblk == 0) return CP_OK;
  kh_part *part = nullptr;                                 // two partials per block, in stream order like the kernels
  if (hipMallocAsync((void **)&part,(size_t)nblk*2*sizeof(kh_part),st) != hipSuccess || !part)
    { (void)hipGetLastError();
      char m[160];
      snprintf(m,sizeof(m),"%s: cannot allocate %zu bytes for the block partials",who,(size_t)nblk*2*sizeof(kh_part));
      return set_err(CP_ENOMEM,m);
    }
  const kl_view ta = kl_view_of(a), tb = kl_view_of(b);
#define KH_RUN(C,LA,LB,LK) kh_hits_kernel<C,LA,LB,LK><<<(unsigned)nblk,KT_BLOCK,0,st>>>(ta,tb,rg,d_seq,d_seq_off,nreads, \
                                                                                      total_bases,a->K,d_hits,part)
#define KH_RUN_L(C,LA,LB) do { if (lock) KH_RUN(C,LA,LB,true); else KH_RUN(C,LA,LB,false); } while (0)
#define KH_RUN_T(C) do { if (kl_lo_only(a)) { if (kl_lo_only(b)) KH_RUN_L(C,true,true); else KH_RUN_L(C,true,false); } \
                         else { if (kl_lo_only(b)) KH_RUN_L(C,false,true); else KH_RUN_L(C,false,false); } } while (0)
  if (canonical) KH_RUN_T(true); else KH_RUN_T(false);
#undef KH_RUN_T
#undef KH_RUN_L
#undef KH_RUN
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    { kh_stitch_kernel<<<(unsigned)nblk,64,0,st>>>(part,d_seq_off,nreads,a->K,d_hits);
      e = hipGetLastError();
    }
  const hipError_t ef = hipFreeAsync(part,st);
  if (e == hipSuccess) e = ef;
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  return CP_OK;
}

extern "C" int cp_bin_call(const int64_t *hit, int64_t only_a, int64_t only_b, int64_t min_markers, int normalise)
{ if (!hit) return set_err(CP_EINVAL,"cp_bin_call: bad argument");
  const __int128 na = hit[CP_HIT_A], nb = hit[CP_HIT_B];
  if (na+nb < (__int128)min_markers) return 'U';
  const bool norm = normalise && only_a > 0 && only_b > 0;
  const __int128 wa = norm ? only_a : 1, wb = norm ? only_b : 1;
  if (na*wb > nb*wa) return 'A';
  if (nb*wa > na*wb) return 'B';
  return 'U';
}

// kmer_setops.hip -- set algebra on sorted snapshots (tabop): the AND, OR, SUB or XOR of two cp_kmer_sorted as a third,
// with a count rule and a count range per operand, and the FASTK histogram of a snapshot's counts.  Semantics:
// include/classpro_amd.h, "Set algebra on sorted k-mers"; design: DESIGN.md 9.14.  Included by capi.hip after
// kmer_lookup.hip (the snapshot, ks_bucket, ks_alloc, the three scan kernels, kc_wave_add, set_err and HIPCHK are in
// scope).  Both operands are only read.
//   cut      the merged sequence of all n+m entries (an A entry before the B entry of the same key) is cut into tiles
//            of KS_TILE entries: one lane per cut searches the two global arrays for the (i, j) of diagonal t*KS_TILE.
//            A cut that falls between an A entry and the B entry of the same key moves behind that B entry, so a pair
//            is never split and a tile holds KS_TILE-1, KS_TILE or KS_TILE+1 entries.
//   tile     a block loads its A range and its B range into LDS (8-byte loads from the three arrays; hi[] is neither
//            loaded nor compared where 2K <= 63 and it is zero).  Each entry searches the other side's range in LDS:
//            an A entry finds its partner and decides for the pair; a B entry without a partner decides for itself; a
//            B entry with one leaves it to its partner.  The search also gives the entry's rank in the merged tile.
//   count    the first pass leaves the kept entries of every tile and the tally; the three scan launches of
//            kmer_sort.hip turn the tile counts into the tiles' places in the result, which is then allocated at its
//            exact size.
//   write    the second pass repeats the decisions, marks the kept entries at their ranks, compacts them by a block scan
//            and stores them with coalesced 8-byte stores.  A run of one bucket inside a tile adds its length to the
//            bucket's counter by at most two 64-bit atomics (minus its first place, plus one past its last), and the
//            same scan over the counters leaves the bucket starts.  No lane walks over empty buckets.
//   derived  what every stage that makes a snapshot out of the kept entries of another shares, here once: the host steps
//            (so_derived_*: the fresh result, the tile and scan sizes, the scan of the tile counts, the exact allocation,
//            the scan of the bucket counters, the unwinding) and, for a per-entry predicate over ONE snapshot, the two
//            kernels (ks_keep_count_kernel, ks_keep_write_kernel).  Used by kmer_hetpairs.hip, kmer_unitigs.hip (the
//            count kernel) and kmer_prune.hip.
// Every search has a constant bound and every index is clamped to its array.
#define SO_CAP   (KS_TILE+1)                               // entries of a tile at most
#define SO_PER   ((SO_CAP+KS_BLOCK-1)/KS_BLOCK)            // ranks per lane in the compaction
#define SO_NONE  0xffffu
#define HP_PER_LANE (KS_TILE/KS_BLOCK)                     // consecutive entries of a lane in the compaction by a predicate

struct so_view { const unsigned long long *hi, *lo, *cnt; int64_t n; };

struct so_rule
  { int set_op, cnt_op;
    unsigned long long amin, amax, bmin, bmax;
  };

template <bool HI>
__device__ static inline bool so_less(unsigned long long ah, unsigned long long al, unsigned long long bh,
                                      unsigned long long bl)
{ return HI ? (ah < bh || (ah == bh && al < bl)) : al < bl; }

// cut t = the (i, j) where tile t begins, t in [0, ntile]; see the file comment
template <bool HI>
__global__ void __launch_bounds__(KT_BLOCK) so_cut_kernel(so_view a, so_view b, int64_t ntile, int64_t *ci, int64_t *cj)
{ const int64_t n = a.n, m = b.n;
  for (int64_t t = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; t <= ntile; t += (int64_t)gridDim.x*blockDim.x)
    { const int64_t d = min(t*(int64_t)KS_TILE,n+m);
      int64_t lo = max((int64_t)0,d-m), hi = min(d,n);     // i = the entries of A among the first d of the merge
      for (int step = 0; step < 64 && lo < hi; step++)
        { const int64_t mid = (lo+hi) >> 1;
          const int64_t ia = min(max(mid,(int64_t)0),n-1), ib = min(max(d-1-mid,(int64_t)0),m-1);
          if (!so_less<HI>(HI ? b.hi[ib] : 0,b.lo[ib],HI ? a.hi[ia] : 0,a.lo[ia])) lo = mid+1;    // A[mid] <= B[d-1-mid]
          else hi = mid;
        }
      const int64_t i = lo;
      int64_t j = d-i;
      if (i > 0 && j < m && a.lo[i-1] == b.lo[j] && (!HI || a.hi[i-1] == b.hi[j])) j++;             // never split a pair
      ci[t] = i;
      cj[t] = j;
    }
}

// The kept entries of a tile from LDS to their places base.. of the result by coalesced 8-byte stores: entry i of the nk
// is slot at(i) of (shi, slo, scn).  A run of one bucket adds its length to cnt_of[bucket] by at most two 64-bit atomics
// (minus its first place, plus one past its last; per_entry: one atomic per entry instead).
template <bool HI, class AT>
__device__ static inline void so_store_kept(const unsigned long long *shi, const unsigned long long *slo,
                                            const unsigned long long *scn, AT at, int nk, int64_t base,
                                            unsigned long long *ohi, unsigned long long *olo, unsigned long long *ocn,
                                            int64_t on, unsigned long long *cnt_of, int64_t nb, int shift, bool per_entry)
{ for (int i = threadIdx.x; i < nk; i += KS_BLOCK)
    { const int s = at(i);
      const int64_t g = base+i;
      if ((unsigned long long)g >= (unsigned long long)on) continue;    // cannot happen while the operands are only read
      const unsigned long long kh = HI ? shi[s] : 0, kl = slo[s];
      if (HI) ohi[g] = kh; else ohi[g] = 0;
      olo[g] = kl;
      ocn[g] = scn[s];
      const unsigned long long bk = ks_bucket(kh,kl,shift);
      if (bk >= (unsigned long long)nb) continue;
      bool head = per_entry || i == 0, tail = per_entry || i == nk-1;
      if (!head)
        { const int p = at(i-1);
          head = ks_bucket(HI ? shi[p] : 0,slo[p],shift) != bk;
        }
      if (!tail)
        { const int p = at(i+1);
          tail = ks_bucket(HI ? shi[p] : 0,slo[p],shift) != bk;
        }
      if (head && tail) atomicAdd(&cnt_of[bk],1ull);
      else if (head) atomicAdd(&cnt_of[bk],0ull-(unsigned long long)g);      // the sums wrap to the run's length
      else if (tail) atomicAdd(&cnt_of[bk],(unsigned long long)g+1);
    }
}

// The compaction of ONE snapshot by a predicate (kmer_hetpairs.hip, kmer_unitigs.hip, kmer_prune.hip): KEEP is a small
// struct passed by value whose operator()(int64_t i) says whether entry i is kept.
// tile_n[t] = the kept entries among [t*KS_TILE, (t+1)*KS_TILE)
template <class KEEP>
__global__ void __launch_bounds__(KS_BLOCK) ks_keep_count_kernel(KEEP keep, int64_t n, int64_t *tile_n)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x*KS_TILE;
  unsigned long long mine = 0;
  for (int s = threadIdx.x; s < KS_TILE; s += KS_BLOCK)
    if (i0+s < n) mine += keep(i0+s);
  const unsigned long long tot = ks_block_scan(mine,part);
  if (threadIdx.x == KS_BLOCK-1) tile_n[blockIdx.x] = (int64_t)tot;
}

// tile_n holds the inclusive sums: the kept entries of a tile go to their places in order.  keep is asked once per entry.
template <bool HI, class KEEP>
__global__ void __launch_bounds__(KS_BLOCK) ks_keep_write_kernel(so_view a, KEEP keep, const int64_t *tile_n,
                                                                 unsigned long long *ohi, unsigned long long *olo,
                                                                 unsigned long long *ocn, int64_t on, unsigned long long *cnt_of,
                                                                 int64_t nb, int shift)
{ __shared__ unsigned long long shi[HI ? KS_TILE : 1], slo[KS_TILE], scn[KS_TILE];
  __shared__ unsigned long long part[KS_BLOCK];
  const int64_t t = blockIdx.x, i0 = t*KS_TILE+(int64_t)threadIdx.x*HP_PER_LANE;
  unsigned int bits = 0, mine = 0;
  for (int k = 0; k < HP_PER_LANE; k++)
    { if (i0+k >= a.n) break;
      if (keep(i0+k)) { bits |= 1u << k; mine++; }
    }
  int at = (int)(ks_block_scan((unsigned long long)mine,part)-(unsigned long long)mine);
  for (int k = 0; k < HP_PER_LANE; k++)
    { if (!((bits >> k) & 1u) || at >= KS_TILE) continue;
      if (HI) shi[at] = a.hi[i0+k];
      slo[at] = a.lo[i0+k];
      scn[at] = a.cnt[i0+k];
      at++;
    }
  __syncthreads();
  const int nk = (int)min(part[KS_BLOCK-1],(unsigned long long)KS_TILE);
  so_store_kept<HI>(shi,slo,scn,[](int i) { return i; },nk,t ? tile_n[t-1] : 0,ohi,olo,ocn,on,cnt_of,nb,shift,false);
}

// WRITE = false: tile_n[t] = the kept entries of tile t, tally += only in A, only in B, in both.
// WRITE = true: tile_n holds the inclusive sums of those; the kept entries go to their places in (ohi, olo, ocn) and
// the bucket counters cnt_of[bucket] take the run lengths.
template <bool HI, bool WRITE>
__global__ void __launch_bounds__(KS_BLOCK) so_tile_kernel(so_view a, so_view b, so_rule r, const int64_t *ci,
                                                           const int64_t *cj, int64_t *tile_n, unsigned long long *tally,
                                                           unsigned long long *ohi, unsigned long long *olo,
                                                           unsigned long long *ocn, int64_t on, unsigned long long *cnt_of,
                                                           int64_t nb, int shift, bool per_entry)
{ __shared__ unsigned long long shi[HI ? SO_CAP : 1], slo[SO_CAP], scn[SO_CAP];
  __shared__ unsigned long long part[KS_BLOCK], blk[3];
  __shared__ unsigned short ord[WRITE ? SO_PER*KS_BLOCK : 1], pack[WRITE ? SO_CAP : 1];
  const int64_t t = blockIdx.x;
  const int64_t i0 = min(max(ci[t],(int64_t)0),a.n), j0 = min(max(cj[t],(int64_t)0),b.n);
  const int na = (int)min(max(ci[t+1]-i0,(int64_t)0),min((int64_t)SO_CAP,a.n-i0));
  const int nbt = (int)min(max(cj[t+1]-j0,(int64_t)0),min((int64_t)(SO_CAP-na),b.n-j0));
  const int nt = na+nbt;
  for (int s = threadIdx.x; s < na; s += KS_BLOCK)
    { if (HI) shi[s] = a.hi[i0+s];
      slo[s] = a.lo[i0+s];
      scn[s] = a.cnt[i0+s];
    }
  for (int s = threadIdx.x; s < nbt; s += KS_BLOCK)
    { if (HI) shi[na+s] = b.hi[j0+s];
      slo[na+s] = b.lo[j0+s];
      scn[na+s] = b.cnt[j0+s];
    }
  if (WRITE)
    for (int s = threadIdx.x; s < SO_PER*KS_BLOCK; s += KS_BLOCK) ord[s] = SO_NONE;
  else if (threadIdx.x < 3) blk[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long only_a = 0, only_b = 0, both = 0, kept = 0;
  for (int s = threadIdx.x; s < nt; s += KS_BLOCK)
    { const bool is_a = s < na;
      const unsigned long long kh = HI ? shi[s] : 0, kl = slo[s];
      int x = is_a ? na : 0, x1 = is_a ? nt : na;          // the first entry of the other side that is not below the key
      const int xe = x1;
      for (int step = 0; step < 16 && x < x1; step++)
        { const int mid = (x+x1) >> 1;
          if (so_less<HI>(HI ? shi[mid] : 0,slo[mid],kh,kl)) x = mid+1; else x1 = mid;
        }
      const bool found = x < xe && slo[x] == kl && (!HI || shi[x] == kh);
      const int rank = is_a ? s+(x-na) : (s-na)+x+(found ? 1 : 0);
      const unsigned long long ca = is_a ? scn[s] : 0, cb = is_a ? (found ? scn[x] : 0) : scn[s];
      const bool decides = is_a || !found;                 // a B entry with a partner leaves the pair to it
      const bool in_a = decides && is_a && ca >= r.amin && ca <= r.amax;
      const bool in_b = decides && (!is_a || found) && cb >= r.bmin && cb <= r.bmax;
      only_a += in_a && !in_b;
      only_b += in_b && !in_a;
      both += in_a && in_b;
      const bool keep = r.set_op == CP_SET_AND ? in_a && in_b : r.set_op == CP_SET_OR ? in_a || in_b
                        : r.set_op == CP_SET_SUB ? in_a && !in_b : in_a != in_b;
      kept += keep;
      if (WRITE)
        { const unsigned long long va = in_a ? ca : 0, vb = in_b ? cb : 0;
          unsigned long long c;
          if (!in_a || !in_b) c = va+vb;                    // one side only: its count under every rule
          else c = r.cnt_op == CP_CNT_LEFT ? va : r.cnt_op == CP_CNT_SUM ? va+vb : r.cnt_op == CP_CNT_MIN ? min(va,vb)
                                                                                                             : max(va,vb);
          if (keep)
            { scn[s] = c;                                   // read by no other entry: a partner's count is B's, and kept B entries have none
              ord[min(rank,SO_PER*KS_BLOCK-1)] = (unsigned short)s;
            }
        }
    }
  if (!WRITE)
    { kc_wave_add(blk,only_a);                            // the waves into LDS, then one atomic per block and counter
      kc_wave_add(blk+1,only_b);
      kc_wave_add(blk+2,both);
      const unsigned long long tot = ks_block_scan(kept,part);     // its barriers order the LDS sums before the reads below
      if (threadIdx.x == KS_BLOCK-1) tile_n[t] = (int64_t)tot;
      if (threadIdx.x < 3 && blk[threadIdx.x]) atomicAdd(&tally[threadIdx.x],blk[threadIdx.x]);
      return;
    }
  __syncthreads();
  int mine = 0;
  for (int k = 0; k < SO_PER; k++) mine += ord[threadIdx.x*SO_PER+k] != SO_NONE;
  int at = (int)(ks_block_scan((unsigned long long)mine,part)-(unsigned long long)mine);
  for (int k = 0; k < SO_PER; k++)
    { const unsigned short s = ord[threadIdx.x*SO_PER+k];
      if (s != SO_NONE && at < SO_CAP) pack[at++] = s;
    }
  __syncthreads();
  const int nk = (int)min(part[KS_BLOCK-1],(unsigned long long)SO_CAP);
  so_store_kept<HI>(shi,slo,scn,[&](int i) { return min((int)pack[i],SO_CAP-1); },nk,t ? tile_n[t-1] : 0,ohi,olo,ocn,on,cnt_of,
                    nb,shift,per_entry);
}

// the layout of kc_hist_kernel over the counts of a snapshot
__global__ void __launch_bounds__(KT_BLOCK) so_hist_kernel(const unsigned long long *cnt, int64_t n, unsigned long long *hist)
{ __shared__ unsigned int low[KC_LOW_BINS];
  for (int i = threadIdx.x; i < KC_LOW_BINS; i += KT_BLOCK) low[i] = 0;
  __syncthreads();
  for (int64_t s = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; s < n; s += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long c = cnt[s];
      if (c == 0) continue;
      if (c <= KC_LOW_BINS) atomicAdd(&low[c-1],1u);
      else if (c < CP_MAX_KMER_CNT) atomicAdd(&hist[c-1],1ull);
      else
        { atomicAdd(&hist[CP_MAX_KMER_CNT-1],1ull);
          atomicAdd(&hist[CP_MAX_KMER_CNT],c);
        }
    }
  __syncthreads();
  for (int i = threadIdx.x; i < KC_LOW_BINS; i += KT_BLOCK)
    if (low[i]) atomicAdd(&hist[i],(unsigned long long)low[i]);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

static so_view so_view_of(const cp_kmer_sorted *s)
{ return so_view{ s->key, s->key+s->n, s->key+2*s->n, s->n }; }

// v[0..n) to its inclusive scan; sum is room for (n + KS_CHUNK - 1) / KS_CHUNK words
static void so_scan(int64_t *v, int64_t n, unsigned long long *sum, hipStream_t st)
{ const int nchunk = (int)((n+KS_CHUNK-1)/KS_CHUNK);
  ks_chunk_sum_kernel<<<nchunk,KS_BLOCK,0,st>>>(v,n,sum);
  ks_sum_scan_kernel<<<1,KS_BLOCK,0,st>>>(sum,nchunk);
  ks_chunk_scan_kernel<<<nchunk,KS_BLOCK,0,st>>>(v,n,sum);
}

// the memory of a result of n_out entries: its bucket counters, zeroed, and its entries (none for an empty result)
static int so_result_alloc(const char *who, cp_kmer_sorted *s, int64_t n_out, hipStream_t st)
{ int rc = ks_alloc(who,(void **)&s->start,(size_t)(s->nb+1)*8,"the bucket starts");
  if (rc != CP_OK) return rc;
  HIPCHK(hipMemsetAsync(s->start,0,(size_t)(s->nb+1)*8,st));
  s->n = n_out;
  if (n_out > 0) rc = ks_alloc(who,(void **)&s->key,(size_t)n_out*24,"the result's entries");
  return rc;
}

// ---- a snapshot derived from one that exists: what cp_kmer_sorted_combine, cp_kmer_sorted_het_pairs and
// cp_kmer_sorted_unitig_prune share on the host.  A caller counts the kept entries per tile into tile_n, calls
// so_derived_counted, waits for the stream, calls so_derived_alloc, launches its write kernel and calls so_derived_starts.

// where a write kernel puts the result: its three arrays, its entries, the bucket counters and the shift of ks_bucket
struct so_dest { unsigned long long *hi, *lo, *cnt, *cnt_of; int64_t n, nb; int shift; };

// a fresh result with the shape of the operand
static int so_derived_new(const char *who, const cp_kmer_sorted *a, cp_kmer_sorted **res)
{ cp_kmer_sorted *s = new (std::nothrow) cp_kmer_sorted();
  if (!s) return set_err(CP_ENOMEM,std::string(who)+": out of memory");
  s->K = a->K; s->ibyte = a->ibyte; s->pbits = a->pbits; s->nb = a->nb;
  *res = s;
  return CP_OK;
}

// the tiles of n entries and the words so_scan needs over them or over nb buckets: tile_n and sum are ntile+nsum words of
// the caller's scratch, in that order.  bound: more tiles than the scan takes are refused.
static int so_derived_tiles(const char *who, int64_t n, int64_t nb, bool bound, int64_t *ntile, int64_t *nsum)
{ *ntile = (n+KS_TILE-1)/KS_TILE;
  if (bound && *ntile > (int64_t)KS_CHUNK*KS_CHUNK) return set_err(CP_EINVAL,std::string(who)+": more than 2^24 tiles");
  *nsum = std::max((*ntile+KS_CHUNK-1)/KS_CHUNK,(nb+KS_CHUNK-1)/KS_CHUNK);
  return CP_OK;
}

// the tile counts to their inclusive sums; n_out is the last of them once the stream has been waited for
static int so_derived_counted(int64_t *tile_n, int64_t ntile, unsigned long long *sum, hipStream_t st, int64_t &n_out)
{ so_scan(tile_n,ntile,sum,st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&n_out,tile_n+ntile-1,8,hipMemcpyDeviceToHost,st));
  return CP_OK;
}

// the result's memory at its exact size, and where its entries go
static int so_derived_alloc(const char *who, cp_kmer_sorted *s, int64_t n_out, hipStream_t st, so_dest *o)
{ const int rc = so_result_alloc(who,s,n_out,st);
  if (rc != CP_OK) return rc;
  *o = so_dest{ s->key, s->key+n_out, s->key+2*n_out, (unsigned long long *)s->start+1,  // start[p+1] counts bucket p, then ends it
                n_out, s->nb, 2*s->K-s->pbits };
  return CP_OK;
}

// the kept entries of every tile of a to their places, by a predicate
template <class KEEP>
static int so_derived_write(const cp_kmer_sorted *a, KEEP keep, bool with_hi, int64_t ntile, const int64_t *tile_n,
                            const so_dest &o, hipStream_t st)
{ const so_view va = so_view_of(a);
  if (with_hi) ks_keep_write_kernel<true><<<(unsigned)ntile,KS_BLOCK,0,st>>>(va,keep,tile_n,o.hi,o.lo,o.cnt,o.n,o.cnt_of,o.nb,o.shift);
  else ks_keep_write_kernel<false><<<(unsigned)ntile,KS_BLOCK,0,st>>>(va,keep,tile_n,o.hi,o.lo,o.cnt,o.n,o.cnt_of,o.nb,o.shift);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

// the bucket counters that the write kernel left to the bucket starts
static int so_derived_starts(cp_kmer_sorted *s, unsigned long long *sum, hipStream_t st)
{ so_scan(s->start+1,s->nb,sum,st);
  HIPCHK(hipGetLastError());
  return CP_OK;
}

// the end of the three calls: rc is what the passes returned.  The scratch goes; the result goes too when they failed,
// otherwise it is ready and the caller's.
static int so_derived_finish(int rc, hipStream_t st, void *scratch, cp_kmer_sorted *s, cp_kmer_sorted **out)
{ if (rc != CP_OK) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  if (rc != CP_OK)
    { cp_kmer_sorted_destroy(s);
      return rc;
    }
  if (s)
    { s->ready = true;
      s->filled = s->n;
      *out = s;
    }
  return CP_OK;
}

// the two passes; scratch and the result's memory are freed by the caller when this fails
static int so_combine(const cp_kmer_sorted *a, const cp_kmer_sorted *b, const so_rule &r, bool with_hi, bool per_entry,
                      int64_t *tally,
                      hipStream_t st, cp_kmer_sorted *s, void **scratch)
{ const char *who = "cp_kmer_sorted_combine";
  const so_view va = so_view_of(a), vb = so_view_of(b);
  int64_t ntile, nsum;
  int rc = so_derived_tiles(who,a->n+b->n,a->nb,true,&ntile,&nsum);
  if (rc != CP_OK) return rc;
  rc = ks_alloc(who,scratch,(size_t)(4+3*ntile+2+nsum)*8,"the cuts and the tile counts");
  if (rc != CP_OK) return rc;
  unsigned long long *d_tally = (unsigned long long *)*scratch, *sum = d_tally+4+3*ntile+2, h_tally[4] = { 0, 0, 0, 0 };
  int64_t *ci = (int64_t *)d_tally+4, *cj = ci+ntile+1, *tile_n = cj+ntile+1, n_out = 0;
  if (ntile > 0)
    { HIPCHK(hipMemsetAsync(d_tally,0,32,st));
      const int cgrid = kt_grid((unsigned long long)ntile+1);
      if (with_hi)
        { so_cut_kernel<true><<<cgrid,KT_BLOCK,0,st>>>(va,vb,ntile,ci,cj);
          so_tile_kernel<true,false><<<(unsigned)ntile,KS_BLOCK,0,st>>>(va,vb,r,ci,cj,tile_n,d_tally,nullptr,nullptr,nullptr,0,
                                                                      nullptr,0,0,false);
        }
      else
        { so_cut_kernel<false><<<cgrid,KT_BLOCK,0,st>>>(va,vb,ntile,ci,cj);
          so_tile_kernel<false,false><<<(unsigned)ntile,KS_BLOCK,0,st>>>(va,vb,r,ci,cj,tile_n,d_tally,nullptr,nullptr,nullptr,
                                                                       0,nullptr,0,0,false);
        }
      HIPCHK(hipGetLastError());
      rc = so_derived_counted(tile_n,ntile,sum,st,n_out);
      if (rc != CP_OK) return rc;
      HIPCHK(hipMemcpyAsync(h_tally,d_tally,24,hipMemcpyDeviceToHost,st));
    }
  HIPCHK(hipStreamSynchronize(st));
  if (tally)
    { for (int k = 0; k < 3; k++) tally[k] = (int64_t)h_tally[k];
      tally[3] = n_out;
    }
  if (!s) return CP_OK;
  so_dest o;
  rc = so_derived_alloc(who,s,n_out,st,&o);
  if (rc != CP_OK) return rc;
  if (n_out > 0)
    { if (with_hi)
        so_tile_kernel<true,true><<<(unsigned)ntile,KS_BLOCK,0,st>>>(va,vb,r,ci,cj,tile_n,nullptr,o.hi,o.lo,o.cnt,o.n,o.cnt_of,o.nb,
                                                                   o.shift,per_entry);
      else
        so_tile_kernel<false,true><<<(unsigned)ntile,KS_BLOCK,0,st>>>(va,vb,r,ci,cj,tile_n,nullptr,o.hi,o.lo,o.cnt,o.n,o.cnt_of,o.nb,
                                                                    o.shift,per_entry);
      HIPCHK(hipGetLastError());
      rc = so_derived_starts(s,sum,st);
      if (rc != CP_OK) return rc;
    }
  HIPCHK(hipStreamSynchronize(st));
  return CP_OK;
}

extern "C" int cp_kmer_sorted_combine(const cp_kmer_sorted *a, const cp_kmer_sorted *b, int set_op, int cnt_op,
                                      const int64_t *range, int64_t *tally, void *stream, cp_kmer_sorted **out)
{ if (out) *out = nullptr;
  if (!a || !b || (!out && !tally)) return set_err(CP_EINVAL,"cp_kmer_sorted_combine: bad argument");
  if (!a->ready || !b->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_combine: an operand is still being loaded");
  if (a->K != b->K)
    { char m[120];
      snprintf(m,sizeof(m),"cp_kmer_sorted_combine: the operands hold %d-mers and %d-mers",a->K,b->K);
      return set_err(CP_EINVAL,m);
    }
  if (set_op < CP_SET_AND || set_op > CP_SET_XOR) return set_err(CP_EINVAL,"cp_kmer_sorted_combine: set_op must lie in [0, 3]");
  if (cnt_op < CP_CNT_LEFT || cnt_op > CP_CNT_MAX) return set_err(CP_EINVAL,"cp_kmer_sorted_combine: cnt_op must lie in [0, 3]");
  so_rule r{ set_op, cnt_op, 1, (unsigned long long)INT64_MAX, 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0] || range[2] < 1 || range[3] < range[2])
        return set_err(CP_EINVAL,"cp_kmer_sorted_combine: a count range needs 1 <= min <= max");
      r.amin = (unsigned long long)range[0]; r.amax = (unsigned long long)range[1];
      r.bmin = (unsigned long long)range[2]; r.bmax = (unsigned long long)range[3];
    }
  hipStream_t st = (hipStream_t)stream;
  cp_kmer_sorted *s = nullptr;
  if (out && so_derived_new("cp_kmer_sorted_combine",a,&s) != CP_OK) return CP_ENOMEM;
  bool with_hi = 2*a->K > 63;                              // below that hi[] is zero for every key
  if (const char *e = getenv("CLASSPRO_SETOP_HI")) with_hi = with_hi || atoi(e) != 0;   // A/B knob of scripts/setop_bench.py
  bool per_entry = false;                                  // one atomic per result entry instead of two per bucket run
  if (const char *e = getenv("CLASSPRO_SETOP_ATOMICS")) per_entry = strcmp(e,"entry") == 0;            // A/B knob as well
  void *scratch = nullptr;
  const int rc = so_combine(a,b,r,with_hi,per_entry,tally,st,s,&scratch);
  return so_derived_finish(rc,st,scratch,s,out);
}

extern "C" int cp_kmer_sorted_hist(const cp_kmer_sorted *s, int64_t *hist, int64_t *ilowcnt, int64_t *ihighcnt)
{ if (!s || !hist || !ilowcnt || !ihighcnt) return set_err(CP_EINVAL,"cp_kmer_sorted_hist: bad argument");
  if (!s->ready) return set_err(CP_EINVAL,"cp_kmer_sorted_hist: the snapshot is still being loaded");
  const size_t cells = (size_t)CP_MAX_KMER_CNT+1, bytes = cells*sizeof(unsigned long long);
  unsigned long long *d_hist = nullptr;
  const int rc = ks_alloc("cp_kmer_sorted_hist",(void **)&d_hist,bytes,"the device histogram");
  if (rc != CP_OK) return rc;
  std::vector<unsigned long long> h(cells);
  hipError_t e = hipMemsetAsync(d_hist,0,bytes,nullptr);
  if (e == hipSuccess && s->n > 0)
    { so_hist_kernel<<<kt_grid((unsigned long long)s->n),KT_BLOCK,0,nullptr>>>(s->key+2*s->n,s->n,d_hist);
      e = hipGetLastError();
    }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(),d_hist,bytes,hipMemcpyDeviceToHost,nullptr);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  (void)hipFree(d_hist);
  if (e != hipSuccess) return set_err(CP_EHIP,std::string("cp_kmer_sorted_hist: ")+hipGetErrorString(e));
  for (int c = 0; c < CP_MAX_KMER_CNT; c++) hist[c] = (int64_t)h[(size_t)c];
  *ilowcnt = (int64_t)h[0];
  *ihighcnt = (int64_t)h[(size_t)CP_MAX_KMER_CNT];
  return CP_OK;
}

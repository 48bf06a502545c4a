// kmer_phase.hip -- heterozygous sites phased from reads (tabphase): the mated pairs of a snapshot of heterozygous k-mers
// become sites with two alleles, the reads that carry two sites say whether their smaller k-mers lie on one haplotype or
// on two, and a maximum spanning forest over those votes gives every site a block and a side.  Semantics:
// include/classpro_amd.h, "Phasing heterozygous sites from reads"; the rule: ph_rule.h; design: DESIGN.md 9.24.  Included
// by capi.hip after kmer_hetpairs.hip (hp_siblings, kl_view, kl_find_group, kt_walk_all, the ks_keep_ kernels, the so_derived_
// helpers, so_scan, ks_block_scan, ks_alloc, kc_wave_add, set_err and HIPCHK are in scope).  Every snapshot is only read.
//   sites    ph_sole_kernel, one lane per entry: the siblings of the entry inside P (hp_siblings, no range); an entry with
//            exactly one keeps its ordinal.  ph_mate_kernel looks at the sibling's degree: i and m are mates when each is
//            the other's only sibling.  The low members are counted per tile (ks_keep_count_kernel) and scanned (so_scan);
//            ph_mark_kernel repeats the count of its tile and writes the marks of both members from the low one.
//   markers  pl_marker_kernel has the lane shape of the profile kernels at half their block: a lane rolls the keys of its
//            KT_CHUNK positions once (kt_walk_all), searches each once and keeps the marks it meets in a column of LDS and
//            a 64-bit mask.  The block scans its lanes' counts, takes a range of the staging array from one cursor (one
//            atomic per block) and writes its markers there in position order; it leaves its range's start and its count.
//            The counts are scanned (so_scan): marker m of the batch is entry m - before(b) of the range of the block b
//            that holds it, so the ORDER of the markers does not depend on the order in which blocks took their ranges.
//            The staging array is sized by a guess (a marker per PL_GUESS bases); the cursor counts every marker, so a
//            pass that did not fit is repeated once at the exact size.
//   links    pl_link_kernel, one lane per marker: the marker and the one before it (each found through the scan of the
//            block counts), their reads by a binary search over d_seq_off; a link key, a `self` or nothing.  The output is
//            compacted by a SECOND COUNT AND SCAN: the kernel runs once to count the links per 256 markers and once more
//            to write them at their exact places (DESIGN.md 9.24 says why not a stage in LDS).
//   forest   Boruvka rounds over the sorted link keys (ph_rule.h).  ph_classify_kernel gives every pair's first key its
//            order word (0: not a kept edge) and sign.  A round: ph_best_kernel (atomicMax of the order word onto both
//            roots), ph_hook_kernel (a root's choice from the state at the start of the round, into an array of its own),
//            ph_apply_kernel, then ph_jump_kernel until every site points at its root -- a lane follows at most PH_JUMP
//            parents per launch, so no content of the arrays makes it run on; the host repeats the launch.  Then
//            ph_low_kernel (atomicMin of the sites onto their root, the tree sizes), ph_side_kernel and
//            ph_conflict_kernel.
//   split    the compaction by a predicate of kmer_setops.hip with "mated, linked, on this side" as the predicate.
// All sums are integer atomics and every word that two lanes may touch is read and written whole: nothing depends on grid,
// block size or scheduling.
#include "ph_rule.h"

#define PL_BLOCK  128                      // lanes of a marker block: 32 KiB of mark columns in LDS
#define PL_CELLS  (PL_BLOCK*KT_CHUNK)      // k-mer positions per marker block
#define PL_GUESS  64                       // bases per marker the first staging array has room for
#define PH_JUMP   64                       // parents a lane follows per launch of the jump kernel
#define PH_ROUNDS_MAX 64                   // more rounds than any forest of fewer than 2^63 sites takes
#define PH_NONE   0xFFFFFFFFFFFFFFFFull

struct pl_marker { int64_t pos; int32_t mark, pad; };      // 16 bytes: the k-mer position in the batch and mark[] of its key

// ---------------------------------------------------------------------------------------------------------------------
// sites

template <bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) ph_sole_kernel(kl_view t, int K, int64_t *sole)
{ const hp_slice none{ nullptr, nullptr, nullptr, 0, 0, 1, 0 };
  const hp_rule any{ 0, ~0ull };                           // the counts are not looked at
  const bool with_hi = 2*K > 63;
  for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < t.n; i += (int64_t)gridDim.x*blockDim.x)
    { int d = 0;
      int64_t at = -1;
      hp_siblings<LO_ONLY,false>(t,none,with_hi ? t.hi[i] : 0,t.lo[i],K,any,false,
                                 [&](int64_t a, unsigned long long) { d++; at = a; });
      sole[i] = d == 1 ? at : -1;
    }
}

// mate[i] = the only sibling of i when i is its only sibling too
__global__ void __launch_bounds__(KT_BLOCK) ph_mate_kernel(const int64_t *sole, int64_t n, int64_t *mate)
{ for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < n; i += (int64_t)gridDim.x*blockDim.x)
    { const int64_t m = sole[i];
      mate[i] = (m >= 0 && m < n && m != i && sole[m] == i) ? m : -1;
    }
}

struct ph_low { const int64_t *mate; __device__ bool operator()(int64_t i) const { return mate[i] > i; } };

// tile_n holds the inclusive sums of the low members per tile: a low member writes its own mark and its mate's
__global__ void __launch_bounds__(KS_BLOCK) ph_mark_kernel(const int64_t *mate, int64_t n, const int64_t *tile_n, int32_t *mark)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t t = blockIdx.x, i0 = t*KS_TILE+(int64_t)threadIdx.x*HP_PER_LANE;
  unsigned long long mine = 0;
  for (int k = 0; k < HP_PER_LANE; k++)
    if (i0+k < n && mate[i0+k] > i0+k) mine++;
  unsigned long long site = (unsigned long long)(t ? tile_n[t-1] : 0)+ks_block_scan(mine,part)-mine;
  for (int k = 0; k < HP_PER_LANE; k++)
    { const int64_t i = i0+k;
      if (i >= n) break;
      const int64_t m = mate[i];
      if (m < 0) mark[i] = -1;
      else if (m > i && m < n)
        { mark[i] = (int32_t)(site << 1);
          mark[m] = (int32_t)((site << 1) | 1u);
          site++;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// markers and links

template <bool CANON, bool LO_ONLY>
__global__ void __launch_bounds__(PL_BLOCK) pl_marker_kernel(kl_view t, const int32_t *mark, const char *seq, const int64_t *seq_off,
                                                             int nreads, int64_t total, int K, pl_marker *stage, int64_t cap,
                                                             int64_t *blk_start, int64_t *blk_n, unsigned long long *cursor)
{ __shared__ int32_t cell[PL_CELLS];                       // the mark of position c of lane l: cell[c*PL_BLOCK+l]
  __shared__ unsigned int part[PL_BLOCK];
  __shared__ int64_t start_s;
  const int64_t p0 = (int64_t)blockIdx.x*PL_CELLS+(int64_t)threadIdx.x*KT_CHUNK;
  unsigned long long has = 0;                              // bit c: position p0+c is a marker
  if (p0 < total)
    kt_walk_all<CANON>(seq,seq_off,nreads,total,K,p0,
      [&](int, int64_t j, bool ok, unsigned long long hi, unsigned long long lo)
      { if (!ok) return;
        const unsigned long long qh[1] = { hi }, ql[1] = { lo };
        int64_t pos[1];
        kl_find_group<LO_ONLY,KL_INTERP != 0,1>(t,qh,ql,1,pos);
        if (pos[0] < 0) return;
        const int32_t mk = mark[min(pos[0],t.n-1)];
        const int64_t c = j-p0;
        if (mk < 0 || (unsigned long long)c >= (unsigned long long)KT_CHUNK) return;
        cell[(int)c*PL_BLOCK+threadIdx.x] = mk;
        has |= 1ull << c;
      });
  const unsigned int mine = (unsigned int)__popcll(has);
  part[threadIdx.x] = mine;
  __syncthreads();
  for (int d = 1; d < PL_BLOCK; d <<= 1)
    { const unsigned int a = threadIdx.x >= (unsigned)d ? part[threadIdx.x-d] : 0;
      __syncthreads();
      part[threadIdx.x] += a;
      __syncthreads();
    }
  const unsigned int nb = part[PL_BLOCK-1];
  if (threadIdx.x == 0)
    { start_s = nb ? (int64_t)atomicAdd(cursor,(unsigned long long)nb) : 0;
      blk_start[blockIdx.x] = start_s;
      blk_n[blockIdx.x] = (int64_t)nb;
    }
  __syncthreads();
  int64_t at = start_s+(int64_t)(part[threadIdx.x]-mine);
  while (has)
    { const int c = __ffsll((unsigned long long)has)-1;
      has &= has-1;
      if (at >= 0 && at < cap) stage[at] = pl_marker{ p0+c, cell[c*PL_BLOCK+threadIdx.x], 0 };
      at++;
    }
}

// what the link kernel reads: the staged markers and where every block's lie
struct pl_list
  { const pl_marker *stage;
    const int64_t *blk_start, *blk_incl;                   // blk_incl: the inclusive scan of the block counts
    int64_t cap, nblk, n;                                  // n markers in all
  };

__device__ static inline pl_marker pl_marker_at(const pl_list &l, int64_t m)
{ int64_t a = 0, e = l.nblk-1;                             // the first block whose inclusive sum exceeds m
  for (int step = 0; step < 64 && a < e; step++)
    { const int64_t mid = (a+e) >> 1;
      if (l.blk_incl[mid] > m) e = mid; else a = mid+1;
    }
  const int64_t k = l.blk_start[a]+m-(a ? l.blk_incl[a-1] : 0);
  return l.stage[min(max(k,(int64_t)0),l.cap-1)];
}

__device__ static inline int pl_read_of(const int64_t *seq_off, int nreads, int64_t p)
{ int lo_r = 0, hi_r = nreads;                             // seq_off[r] <= p < seq_off[r+1], as kt_walk_all finds it
  while (hi_r-lo_r > 1)
    { const int mid = (lo_r+hi_r) >> 1;
      if (seq_off[mid] <= p) lo_r = mid; else hi_r = mid;
    }
  return lo_r;
}

// marker m against the marker before it: 0 nothing (the first marker of its read), 1 a link (*key), 2 the same site again
__device__ static inline int pl_link(const pl_list &l, const int64_t *seq_off, int nreads, int64_t m, unsigned long long *key)
{ if (m <= 0 || m >= l.n) return 0;
  const pl_marker x = pl_marker_at(l,m), w = pl_marker_at(l,m-1);
  if (pl_read_of(seq_off,nreads,x.pos) != pl_read_of(seq_off,nreads,w.pos)) return 0;
  const unsigned long long s = (unsigned long long)(unsigned int)x.mark >> 1, s2 = (unsigned long long)(unsigned int)w.mark >> 1;
  if (s == s2) return 2;
  *key = ph_link_key(s2,(unsigned)w.mark & 1u,s,(unsigned)x.mark & 1u);
  return 1;
}

// WRITE = false: tile_n[b] = the links among the markers [b*KS_BLOCK, (b+1)*KS_BLOCK), *nself += the selfs.
// WRITE = true: tile_n holds the inclusive sums; the keys go to their places.
template <bool WRITE>
__global__ void __launch_bounds__(KS_BLOCK) pl_link_kernel(pl_list l, const int64_t *seq_off, int nreads, int64_t *tile_n,
                                                           unsigned long long *nself, unsigned long long *links, int64_t capacity)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t m = (int64_t)blockIdx.x*KS_BLOCK+threadIdx.x;
  unsigned long long key = 0;
  const int kind = pl_link(l,seq_off,nreads,m,&key);
  const unsigned long long mine = kind == 1;
  const unsigned long long incl = ks_block_scan(mine,part);
  if (!WRITE)
    { if (threadIdx.x == KS_BLOCK-1) tile_n[blockIdx.x] = (int64_t)incl;
      kc_wave_add(nself,kind == 2);
      return;
    }
  const int64_t at = (blockIdx.x ? tile_n[blockIdx.x-1] : 0)+(int64_t)(incl-mine);
  if (mine && at >= 0 && at < capacity) links[at] = key;
}

__global__ void pl_tally_kernel(unsigned long long *tally, unsigned long long markers, unsigned long long nlinks,
                                const unsigned long long *nself)
{ if (threadIdx.x || blockIdx.x) return;
  tally[0] += markers;
  tally[1] += nlinks;
  tally[2] += *nself;
}

// ---------------------------------------------------------------------------------------------------------------------
// forest

struct ph_edges { const unsigned long long *hi, *lo, *cnt; int64_t n; };

// ord[i] = the order word of the pair whose first key is entry i when it is a kept edge, else 0; sgn[i] its sign
__global__ void __launch_bounds__(KT_BLOCK) ph_classify_kernel(ph_edges e, unsigned long long nsites, unsigned long long min_support,
                                                               unsigned long long *ord, uint8_t *sgn, unsigned long long *tally)
{ unsigned long long nedge = 0, nkept = 0, ntied = 0, nweak = 0, nbad = 0;
  for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < e.n; i += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long key = e.lo[i];
      unsigned long long o = 0;
      unsigned sign = 0;
      if (!ph_key_ok(e.hi[i],key,nsites)) nbad++;
      else if (i == 0 || e.hi[i-1] != 0 || (e.lo[i-1] >> 1) != (key >> 1))      // the first key of its pair
        { const bool two = i+1 < e.n && e.hi[i+1] == 0 && (e.lo[i+1] >> 1) == (key >> 1);
          const unsigned long long cis = ph_key_x(key) ? 0 : e.cnt[i], trans = ph_key_x(key) ? e.cnt[i] : two ? e.cnt[i+1] : 0;
          unsigned long long margin;
          const int cls = ph_class(cis,trans,min_support,&sign,&margin);
          nedge++;
          nkept += cls == PH_KEPT; ntied += cls == PH_TIED; nweak += cls == PH_WEAK;
          if (cls == PH_KEPT) o = ph_order(margin,(unsigned long long)i);
        }
      ord[i] = o;
      sgn[i] = (uint8_t)sign;
    }
  kc_wave_add(tally+PH_EDGES,nedge);
  kc_wave_add(tally+PH_NKEPT,nkept);
  kc_wave_add(tally+PH_NTIED,ntied);
  kc_wave_add(tally+PH_NWEAK,nweak);
  kc_wave_add(tally+PH_BAD,nbad);
}

__global__ void __launch_bounds__(KT_BLOCK) ph_init_kernel(unsigned long long *word, int64_t nsites)
{ for (int64_t v = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; v < nsites; v += (int64_t)gridDim.x*blockDim.x)
    word[v] = ph_word((unsigned long long)v,0);
}

// every site points at its root: a kept edge between two trees offers itself to both roots
__global__ void __launch_bounds__(KT_BLOCK) ph_best_kernel(ph_edges e, const unsigned long long *ord, const unsigned long long *word,
                                                           unsigned long long nsites, unsigned long long *best)
{ for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < e.n; i += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long o = ord[i];
      if (!o) continue;
      const unsigned long long key = e.lo[i], s = ph_key_s(key), t = ph_key_t(key);
      if (s >= nsites || t >= nsites) continue;            // a kept edge has passed ph_key_ok: cannot happen
      const unsigned long long rs = ph_parent(word[s]), rt = ph_parent(word[t]);
      if (rs == rt || rs >= nsites || rt >= nsites) continue;
      atomicMax(&best[rs],o);
      atomicMax(&best[rt],o);
    }
}

// hook[r] = the word root r takes (PH_NONE: it stays a root); in a mutual choice the larger root hooks
__global__ void __launch_bounds__(KT_BLOCK) ph_hook_kernel(ph_edges e, const uint8_t *sgn, const unsigned long long *word,
                                                           const unsigned long long *best, unsigned long long nsites,
                                                           unsigned long long *hook, unsigned long long *nhook)
{ unsigned long long mine = 0;
  for (int64_t r = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; r < (int64_t)nsites; r += (int64_t)gridDim.x*blockDim.x)
    { unsigned long long h = PH_NONE;
      const unsigned long long b = best[r];
      if (b && ph_parent(word[r]) == (unsigned long long)r)
        { const int64_t i = (int64_t)min(ph_order_ordinal(b),(unsigned long long)(e.n-1));
          const unsigned long long key = e.lo[i], s = min(ph_key_s(key),nsites-1), t = min(ph_key_t(key),nsites-1);
          const unsigned long long ws = word[s], wt = word[t], rs = ph_parent(ws), rt = ph_parent(wt);
          const unsigned long long other = rs == (unsigned long long)r ? rt : rs;
          if ((rs == (unsigned long long)r) != (rt == (unsigned long long)r) && other < nsites
              && !(best[other] == b && (unsigned long long)r < other))
            { h = ph_word(other,ph_hook_parity(ph_par(ws),sgn[i],ph_par(wt)));
              mine++;
            }
        }
      hook[r] = h;
    }
  kc_wave_add(nhook,mine);
}

__global__ void __launch_bounds__(KT_BLOCK) ph_apply_kernel(const unsigned long long *hook, unsigned long long *word, int64_t nsites)
{ for (int64_t r = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; r < nsites; r += (int64_t)gridDim.x*blockDim.x)
    if (hook[r] != PH_NONE) word[r] = hook[r];
}

// Pointer jumping in place.  A word is read and written whole, and at any moment word[v] names an ancestor of v and the
// parity of the path to it: whichever value of a parent's word a lane reads, what it writes is true again.
__global__ void __launch_bounds__(KT_BLOCK) ph_jump_kernel(unsigned long long *word, unsigned long long nsites, unsigned int *unfinished)
{ for (int64_t v = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; v < (int64_t)nsites; v += (int64_t)gridDim.x*blockDim.x)
    { unsigned long long w = kt_load(word+v);
      bool done = false;
      for (int hop = 0; hop < PH_JUMP; hop++)
        { const unsigned long long p = ph_parent(w);
          if (p == (unsigned long long)v || p >= nsites) { done = true; break; }
          const unsigned long long wp = kt_load(word+p);
          if (ph_parent(wp) == p) { done = true; break; }
          w = ph_hop(w,wp);
        }
      __hip_atomic_store(word+v,w,__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT);
      if (!done) atomicOr(unfinished,1u);
    }
}

// low[r] = the smallest site of root r's tree, size[r] its sites
__global__ void __launch_bounds__(KT_BLOCK) ph_low_kernel(const unsigned long long *word, unsigned long long nsites,
                                                          unsigned long long *low, unsigned long long *size)
{ for (int64_t v = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; v < (int64_t)nsites; v += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long r = min(ph_parent(word[v]),nsites-1);
      atomicMin(&low[r],(unsigned long long)v);
      atomicAdd(&size[r],1ull);
    }
}

__global__ void __launch_bounds__(KT_BLOCK) ph_side_kernel(const unsigned long long *word, unsigned long long nsites,
                                                           const unsigned long long *low, const unsigned long long *size,
                                                           int64_t *block, uint8_t *side, unsigned long long *tally)
{ unsigned long long nblock = 0, nsingle = 0, largest = 0;
  for (int64_t v = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; v < (int64_t)nsites; v += (int64_t)gridDim.x*blockDim.x)
    { const unsigned long long w = word[v], r = min(ph_parent(w),nsites-1), m = min(low[r],nsites-1);
      block[v] = (int64_t)m;
      side[v] = (uint8_t)(ph_par(w) ^ ph_par(word[m]));
      if (r != (unsigned long long)v) continue;
      if (size[r] >= 2) { nblock++; largest = max(largest,size[r]); }
      else nsingle++;
    }
  kc_wave_add(tally+PH_BLOCKS,nblock);
  kc_wave_add(tally+PH_SINGLE,nsingle);
  if (largest) atomicMax(tally+PH_LARGEST,largest);
}

__global__ void __launch_bounds__(KT_BLOCK) ph_conflict_kernel(ph_edges e, const unsigned long long *ord, const uint8_t *sgn,
                                                               const uint8_t *side, unsigned long long nsites,
                                                               unsigned long long *tally)
{ unsigned long long nconf = 0;
  for (int64_t i = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; i < e.n; i += (int64_t)gridDim.x*blockDim.x)
    { if (!ord[i]) continue;
      const unsigned long long key = e.lo[i], s = min(ph_key_s(key),nsites-1), t = min(ph_key_t(key),nsites-1);
      nconf += (unsigned)sgn[i] != (unsigned)(side[s] ^ side[t]);
    }
  kc_wave_add(tally+PH_CONFLICTS,nconf);
}

// ---------------------------------------------------------------------------------------------------------------------
// split

__global__ void __launch_bounds__(KT_BLOCK) ph_linked_kernel(const int64_t *block, int64_t nsites, uint8_t *linked)
{ for (int64_t v = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; v < nsites; v += (int64_t)gridDim.x*blockDim.x)
    { const int64_t b = block[v];
      if (b == v || b < 0 || b >= nsites) continue;
      linked[v] = 1;                                       // every writer writes the same value
      linked[b] = 1;
    }
}

struct ph_keep_side
  { const int32_t *mark;
    const uint8_t *side, *linked;
    int64_t nsites;
    unsigned which;
    __device__ bool operator()(int64_t i) const
    { const int32_t m = mark[i];
      if (m < 0 || (m >> 1) >= nsites || !linked[m >> 1]) return false;
      return (unsigned)((side[m >> 1] ^ m) & 1) == which;
    }
  };

// ---------------------------------------------------------------------------------------------------------------------
// host side

static int ph_sites_run(const cp_kmer_sorted *p, int64_t *d_mate, int32_t *d_mark, int64_t *nsites, hipStream_t st, void **scratch)
{ const char *who = "cp_kmer_sorted_het_sites";
  const kl_view t = kl_view_of(p);
  int64_t ntile, nsum;
  int rc = so_derived_tiles(who,p->n,0,true,&ntile,&nsum);
  if (rc != CP_OK) return rc;
  rc = ks_alloc(who,scratch,(size_t)(p->n*(d_mate ? 1 : 2)+ntile+nsum)*8,"the siblings, the mates and the tile counts");
  if (rc != CP_OK) return rc;
  int64_t *sole = (int64_t *)*scratch, *mate = d_mate ? d_mate : sole+p->n, *tile_n = sole+p->n*(d_mate ? 1 : 2);
  unsigned long long *sum = (unsigned long long *)(tile_n+ntile);
  const int grid = kt_grid((unsigned long long)p->n);
  if (kl_lo_only(p)) ph_sole_kernel<true><<<grid,KT_BLOCK,0,st>>>(t,p->K,sole);
  else ph_sole_kernel<false><<<grid,KT_BLOCK,0,st>>>(t,p->K,sole);
  HIPCHK(hipGetLastError());
  ph_mate_kernel<<<grid,KT_BLOCK,0,st>>>(sole,p->n,mate);
  ks_keep_count_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(ph_low{ mate },p->n,tile_n);
  HIPCHK(hipGetLastError());
  int64_t n_low = 0;
  rc = so_derived_counted(tile_n,ntile,sum,st,n_low);
  if (rc != CP_OK) return rc;
  HIPCHK(hipStreamSynchronize(st));
  if (n_low >= ((int64_t)1 << 30)) return set_err(CP_EINVAL,std::string(who)+": 2^30 sites or more (a mark is site << 1 | allele in an int32)");
  ph_mark_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(mate,p->n,tile_n,d_mark);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  *nsites = n_low;
  return CP_OK;
}

extern "C" int cp_kmer_sorted_het_sites(const cp_kmer_sorted *p, int64_t *d_mate, int32_t *d_mark, int64_t *nsites,
                                        int64_t *tally, void *stream)
{ const char *who = "cp_kmer_sorted_het_sites";
  if (!p || !nsites) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!p->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (p->n > 0 && !d_mark) return set_err(CP_EINVAL,std::string(who)+": null d_mark");
  *nsites = 0;
  hipStream_t st = (hipStream_t)stream;
  void *scratch = nullptr;
  int rc = CP_OK;
  if (p->n > 0)
    { rc = ph_sites_run(p,d_mate,d_mark,nsites,st,&scratch);
      if (rc != CP_OK) (void)hipStreamSynchronize(st);
      if (scratch) (void)hipFree(scratch);
    }
  if (rc == CP_OK && tally)
    { tally[0] = 2*(*nsites);
      tally[1] = p->n-2*(*nsites);
    }
  return rc;
}

// one pass over the batch into a staging array of cap markers; *nmark = the markers of the batch, which fit when <= cap
static hipError_t pl_marker_pass(const cp_kmer_sorted *p, const int32_t *d_mark, int canonical, const char *d_seq,
                                 const int64_t *d_seq_off, int nreads, int64_t total_bases, int64_t nblk, uint8_t *scratch,
                                 int64_t cap, hipStream_t st, int64_t *nmark)
{ unsigned long long *ctl = (unsigned long long *)scratch;                       // [0] the cursor, [1] the selfs
  int64_t *blk_start = (int64_t *)(ctl+2), *blk_n = blk_start+nblk;
  unsigned long long *sum = (unsigned long long *)(blk_n+nblk);
  pl_marker *stage = (pl_marker *)(sum+(nblk+KS_CHUNK-1)/KS_CHUNK);
  hipError_t e = hipMemsetAsync(ctl,0,16,st);
  if (e != hipSuccess) return e;
  const kl_view t = kl_view_of(p);
#define PL_RUN(C,L) pl_marker_kernel<C,L><<<(unsigned)nblk,PL_BLOCK,0,st>>>(t,d_mark,d_seq,d_seq_off,nreads,total_bases,p->K,stage, \
                                                                          cap,blk_start,blk_n,ctl)
  if (canonical) { if (kl_lo_only(p)) PL_RUN(true,true); else PL_RUN(true,false); }
  else { if (kl_lo_only(p)) PL_RUN(false,true); else PL_RUN(false,false); }
#undef PL_RUN
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  so_scan(blk_n,nblk,sum,st);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(nmark,ctl,8,hipMemcpyDeviceToHost,st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}

extern "C" int cp_kmer_sorted_read_links(const cp_kmer_sorted *p, const int32_t *d_mark, int canonical, const char *d_seq,
                                         const int64_t *d_seq_off, int nreads, int64_t total_bases, uint64_t *d_links,
                                         int64_t capacity, int64_t *total, int64_t *d_tally, void *stream)
{ const char *who = "cp_kmer_sorted_read_links";
  if (!p || !total || nreads < 0 || total_bases < 0 || capacity < 0) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!p->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if ((capacity > 0 && !d_links) || (nreads > 0 && !d_seq_off) || (total_bases > 0 && !d_seq)
      || (p->n > 0 && nreads > 0 && total_bases > 0 && !d_mark))
    return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  const int64_t nblk = nreads > 0 ? (total_bases+(int64_t)PL_CELLS-1)/(int64_t)PL_CELLS : 0;
  if (nblk > (int64_t)KS_CHUNK*KS_CHUNK) return set_err(CP_EINVAL,std::string(who)+": the batch is too long for one call");
  *total = 0;
  hipStream_t st = (hipStream_t)stream;
  if (nblk == 0 || p->n == 0)
    { HIPCHK(hipStreamSynchronize(st));
      return CP_OK;
    }
  // the markers: a staging array by a guess, once more at the exact size when that was too small
  const size_t head = 16+(size_t)(2*nblk+(nblk+KS_CHUNK-1)/KS_CHUNK)*8;
  int64_t cap = std::max<int64_t>(4096,total_bases/PL_GUESS), nmark = 0;
  if (const char *e = getenv("CLASSPRO_PHASE_GUESS")) cap = std::max<int64_t>(1,atoll(e));     // knob of the tests: markers
  uint8_t *scratch = nullptr, *scratch2 = nullptr;
  hipError_t e = hipSuccess;
  for (int attempt = 0; attempt < 2; attempt++)
    { const size_t bytes = head+(size_t)cap*sizeof(pl_marker);
      if (hipMalloc((void **)&scratch,bytes) != hipSuccess || !scratch)
        { (void)hipGetLastError();
          char m[160];
          snprintf(m,sizeof(m),"%s: cannot allocate %zu bytes for the markers and the block counts",who,bytes);
          return set_err(CP_ENOMEM,m);
        }
      e = pl_marker_pass(p,d_mark,canonical,d_seq,d_seq_off,nreads,total_bases,nblk,scratch,cap,st,&nmark);
      if (e != hipSuccess || nmark <= cap) break;
      (void)hipStreamSynchronize(st);
      (void)hipFree(scratch);
      scratch = nullptr;
      cap = nmark;
    }
  // the links: counted per KS_BLOCK markers, scanned, then written
  unsigned long long *ctl = (unsigned long long *)scratch;
  const int64_t ntile = (nmark+KS_BLOCK-1)/KS_BLOCK, nsum = (ntile+KS_CHUNK-1)/KS_CHUNK;
  int64_t nlinks = 0;
  if (e == hipSuccess && ntile > (int64_t)KS_CHUNK*KS_CHUNK)
    { (void)hipStreamSynchronize(st);
      (void)hipFree(scratch);
      return set_err(CP_EINVAL,std::string(who)+": more than 2^32 markers in one call");
    }
  if (e == hipSuccess && nmark > 0)
    { if (hipMalloc((void **)&scratch2,(size_t)(ntile+nsum)*8) != hipSuccess || !scratch2)
        { (void)hipGetLastError();
          (void)hipStreamSynchronize(st);
          (void)hipFree(scratch);
          return set_err(CP_ENOMEM,std::string(who)+": cannot allocate the link counts");
        }
      int64_t *blk_start = (int64_t *)(ctl+2), *tile_n = (int64_t *)scratch2;
      const pl_list l{ (const pl_marker *)(scratch+head), blk_start, blk_start+nblk, cap, nblk, nmark };
      pl_link_kernel<false><<<(unsigned)ntile,KS_BLOCK,0,st>>>(l,d_seq_off,nreads,tile_n,ctl+1,nullptr,0);
      e = hipGetLastError();
      if (e == hipSuccess)
        { so_scan(tile_n,ntile,(unsigned long long *)(tile_n+ntile),st);
          e = hipGetLastError();
        }
      if (e == hipSuccess) e = hipMemcpyAsync(&nlinks,tile_n+ntile-1,8,hipMemcpyDeviceToHost,st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e == hipSuccess && nlinks > 0 && nlinks <= capacity)
        { pl_link_kernel<true><<<(unsigned)ntile,KS_BLOCK,0,st>>>(l,d_seq_off,nreads,tile_n,nullptr,(unsigned long long *)d_links,capacity);
          e = hipGetLastError();
        }
    }
  if (e == hipSuccess && d_tally && nlinks <= capacity)
    { pl_tally_kernel<<<1,1,0,st>>>((unsigned long long *)d_tally,(unsigned long long)nmark,(unsigned long long)nlinks,ctl+1);
      e = hipGetLastError();
    }
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (scratch2) (void)hipFree(scratch2);                   // plain allocations, as kmer_fixes.hip: the counters are zeroed by a
  if (scratch) (void)hipFree(scratch);                     // fill in the stream, which the stream-ordered pool does not always order
  if (e != hipSuccess) return set_err(CP_EHIP,std::string(who)+": "+hipGetErrorString(e));
  *total = nlinks;
  if (nlinks > capacity)
    { char m[160];
      snprintf(m,sizeof(m),"%s: %lld links do not fit the %lld of d_links",who,(long long)nlinks,(long long)capacity);
      return set_err(CP_EOVERFLOW,m);
    }
  return CP_OK;
}

// the passes of the forest; the scratch is freed by the caller
static int ph_forest_run(const cp_kmer_sorted *edges, int64_t nsites, int64_t min_support, int64_t *d_block, uint8_t *d_side,
                         int64_t *tally, hipStream_t st, void **scratch)
{ const char *who = "cp_phase_forest";
  const int64_t n = edges->n;
  const ph_edges e{ edges->key, edges->key+n, edges->key+2*n, n };
  const size_t sgn_words = ((size_t)n+7)/8;
  int rc = ks_alloc(who,scratch,(16+(size_t)n+sgn_words+3*(size_t)nsites)*8,"the order words, the signs and three words per site");
  if (rc != CP_OK) return rc;
  unsigned long long *d_tally = (unsigned long long *)*scratch, *ctl = d_tally+PH_WIDTH;    // ctl[0] hooks, ctl[1] unfinished
  unsigned long long *ord = d_tally+16, *word = ord+n+sgn_words, *best = word+nsites, *hook = best+nsites;
  uint8_t *sgn = (uint8_t *)(ord+n);
  unsigned long long h[16];
  int64_t rounds = 0, forest = 0;
  HIPCHK(hipMemsetAsync(d_tally,0,128,st));
  const int egrid = kt_grid((unsigned long long)std::max<int64_t>(n,1)), sgrid = kt_grid((unsigned long long)std::max<int64_t>(nsites,1));
  if (n > 0)
    { ph_classify_kernel<<<egrid,KT_BLOCK,0,st>>>(e,(unsigned long long)nsites,(unsigned long long)min_support,ord,sgn,d_tally);
      HIPCHK(hipGetLastError());
    }
  if (nsites > 0)
    { ph_init_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,nsites);
      HIPCHK(hipGetLastError());
      for (int round = 0; n > 0; round++)
        { if (round >= PH_ROUNDS_MAX) return set_err(CP_EHIP,std::string(who)+": the forest did not settle");
          HIPCHK(hipMemsetAsync(best,0,(size_t)nsites*8,st));
          HIPCHK(hipMemsetAsync(ctl,0,8,st));
          ph_best_kernel<<<egrid,KT_BLOCK,0,st>>>(e,ord,word,(unsigned long long)nsites,best);
          ph_hook_kernel<<<sgrid,KT_BLOCK,0,st>>>(e,sgn,word,best,(unsigned long long)nsites,hook,ctl);
          ph_apply_kernel<<<sgrid,KT_BLOCK,0,st>>>(hook,word,nsites);
          HIPCHK(hipGetLastError());
          for (int pass = 0; ; pass++)
            { if (pass >= 64) return set_err(CP_EHIP,std::string(who)+": the trees did not flatten");
              HIPCHK(hipMemsetAsync(ctl+1,0,8,st));
              ph_jump_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,(unsigned long long)nsites,(unsigned int *)(ctl+1));
              HIPCHK(hipGetLastError());
              HIPCHK(hipMemcpyAsync(h,ctl,16,hipMemcpyDeviceToHost,st));
              HIPCHK(hipStreamSynchronize(st));
              if (!h[1]) break;
            }
          if (!h[0]) break;
          forest += (int64_t)h[0];
          rounds++;
        }
      unsigned long long *low = best, *size = hook;
      HIPCHK(hipMemsetAsync(low,0xff,(size_t)nsites*8,st));
      HIPCHK(hipMemsetAsync(size,0,(size_t)nsites*8,st));
      ph_low_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,(unsigned long long)nsites,low,size);
      ph_side_kernel<<<sgrid,KT_BLOCK,0,st>>>(word,(unsigned long long)nsites,low,size,d_block,d_side,d_tally);
      if (n > 0) ph_conflict_kernel<<<egrid,KT_BLOCK,0,st>>>(e,ord,sgn,d_side,(unsigned long long)nsites,d_tally);
      HIPCHK(hipGetLastError());
    }
  HIPCHK(hipMemcpyAsync(h,d_tally,PH_WIDTH*8,hipMemcpyDeviceToHost,st));
  HIPCHK(hipStreamSynchronize(st));
  if (tally)
    { for (int k = 0; k < PH_WIDTH; k++) tally[k] = (int64_t)h[k];
      tally[PH_FOREST] = forest;
      tally[PH_ROUNDS] = rounds;
    }
  return CP_OK;
}

extern "C" int cp_phase_forest(const cp_kmer_sorted *edges, int64_t nsites, int64_t min_support, int64_t *d_block,
                               uint8_t *d_side, int64_t *tally, void *stream)
{ const char *who = "cp_phase_forest";
  static_assert(PH_EDGES == CP_PH_EDGES && PH_NKEPT == CP_PH_KEPT && PH_NTIED == CP_PH_TIED && PH_NWEAK == CP_PH_WEAK
                && PH_FOREST == CP_PH_FOREST && PH_CONFLICTS == CP_PH_CONFLICTS && PH_BLOCKS == CP_PH_BLOCKS
                && PH_SINGLE == CP_PH_SINGLE && PH_LARGEST == CP_PH_LARGEST && PH_ROUNDS == CP_PH_ROUNDS && PH_BAD == CP_PH_BAD
                && PH_WIDTH == CP_PH_WIDTH,"ph_rule.h and the header name the same cells");
  if (!edges) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!edges->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (edges->K != 32) return set_err(CP_EINVAL,std::string(who)+": the edges are a snapshot of K = 32 link keys");
  if (min_support < 1) return set_err(CP_EINVAL,std::string(who)+": min_support must be 1 or more");
  if (nsites < 0 || nsites >= ((int64_t)1 << 31)) return set_err(CP_EINVAL,std::string(who)+": nsites must lie in [0, 2^31)");
  if (edges->n >= ((int64_t)1 << 48)) return set_err(CP_EINVAL,std::string(who)+": 2^48 keys or more");
  if (nsites > 0 && (!d_block || !d_side)) return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  hipStream_t st = (hipStream_t)stream;
  void *scratch = nullptr;
  const int rc = ph_forest_run(edges,nsites,min_support,d_block,d_side,tally,st,&scratch);
  if (rc != CP_OK) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  return rc;
}

// the passes of the split; scratch and the result's memory are freed by the caller when this fails
static int ph_split_run(const cp_kmer_sorted *p, const int32_t *d_mark, const int64_t *d_block, const uint8_t *d_side,
                        int64_t nsites, unsigned which, hipStream_t st, cp_kmer_sorted *res, void **scratch)
{ const char *who = "cp_kmer_sorted_phase_split";
  int64_t ntile, nsum, n_out = 0;
  int rc = so_derived_tiles(who,p->n,p->nb,true,&ntile,&nsum);
  if (rc != CP_OK) return rc;
  int64_t *tile_n = nullptr;
  unsigned long long *sum = nullptr;
  uint8_t *linked = nullptr;
  if (p->n > 0)
    { rc = ks_alloc(who,scratch,(size_t)(ntile+nsum)*8+(size_t)std::max<int64_t>(nsites,1),"the tile counts and a byte per site");
      if (rc != CP_OK) return rc;
      tile_n = (int64_t *)*scratch;
      sum = (unsigned long long *)(tile_n+ntile);
      linked = (uint8_t *)(sum+nsum);
      HIPCHK(hipMemsetAsync(linked,0,(size_t)std::max<int64_t>(nsites,1),st));
      if (nsites > 0) ph_linked_kernel<<<kt_grid((unsigned long long)nsites),KT_BLOCK,0,st>>>(d_block,nsites,linked);
      ks_keep_count_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(ph_keep_side{ d_mark, d_side, linked, nsites, which },p->n,tile_n);
      HIPCHK(hipGetLastError());
      rc = so_derived_counted(tile_n,ntile,sum,st,n_out);
      if (rc != CP_OK) return rc;
    }
  HIPCHK(hipStreamSynchronize(st));
  so_dest o;
  rc = so_derived_alloc(who,res,n_out,st,&o);
  if (rc != CP_OK) return rc;
  if (n_out > 0)
    { rc = so_derived_write(p,ph_keep_side{ d_mark, d_side, linked, nsites, which },2*p->K > 63,ntile,tile_n,o,st);
      if (rc == CP_OK) rc = so_derived_starts(res,sum,st);
      if (rc != CP_OK) return rc;
    }
  HIPCHK(hipStreamSynchronize(st));
  return CP_OK;
}

extern "C" int cp_kmer_sorted_phase_split(const cp_kmer_sorted *p, const int32_t *d_mark, const int64_t *d_block,
                                          const uint8_t *d_side, int64_t nsites, int which, void *stream, cp_kmer_sorted **out)
{ const char *who = "cp_kmer_sorted_phase_split";
  if (out) *out = nullptr;
  if (!p || !out || nsites < 0 || nsites >= ((int64_t)1 << 31)) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!p->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (which != 0 && which != 1) return set_err(CP_EINVAL,std::string(who)+": which must be 0 (A) or 1 (B)");
  if ((p->n > 0 && !d_mark) || (nsites > 0 && (!d_block || !d_side))) return set_err(CP_EINVAL,std::string(who)+": null device pointer");
  hipStream_t st = (hipStream_t)stream;
  cp_kmer_sorted *res = nullptr;
  if (so_derived_new(who,p,&res) != CP_OK) return CP_ENOMEM;
  void *scratch = nullptr;
  const int rc = ph_split_run(p,d_mark,d_block,d_side,nsites,(unsigned)which,st,res,&scratch);
  return so_derived_finish(rc,st,scratch,res,out);
}

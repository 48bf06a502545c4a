// kmer_prune.hip -- structural cleaning of the unitig graph of ONE sorted snapshot (tabclean): the islands, tips and simple
// bubbles of the graph marked by a rule that looks at the input graph alone, and the snapshot without the k-mers of the
// marked unitigs.  Semantics: include/classpro_amd.h, "Pruning the unitig graph"; design: DESIGN.md 9.22.  Included by
// capi.hip after kmer_paths.hip (cp_unitigs, cp_unitig_graph, ks_keep_write_kernel and the so_derived_ helpers of
// kmer_setops.hip, ks_alloc, ks_block_scan, kc_wave_add, set_err and HIPCHK are in scope).  Everything passed in is only read.
//   rule     one lane per unitig: why[u] = kn_why(u, graph) of kn_rule.h, whose loads come in groups; the islands, tips,
//            bubbles and removed bases summed per wave, then one atomic per wave and counter.
//   count    one block per tile of KS_TILE consecutive entries: an entry is kept when d_utg[i] >= 0 and the mark of that
//            unitig (clamped) is 0; the kept entries of the tile, and the kept and removed keys summed per wave.
//   write    the compaction by a predicate of kmer_setops.hip (so_derived_*, ks_keep_write_kernel) with "the entry is kept"
//            as the predicate.  The count pass stays this file's own: it also sums the kept and the removed keys, and it
//            runs without tile counts when no result is wanted.
// All sums are integer atomics: nothing depends on grid, block size or scheduling.
#include "kn_rule.h"

enum { KN_CTL = 8 };                                        // words of the control block: the tally

// why[u] of every unitig; ctl += islands, tips, bubbles, removed bases
__global__ void __launch_bounds__(KT_BLOCK) kn_rule_kernel(kn_graph g, uint8_t *why, unsigned long long *ctl)
{ unsigned long long nisl = 0, ntip = 0, nbub = 0, nbases = 0;
  for (int64_t u = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; u < g.count; u += (int64_t)gridDim.x*blockDim.x)
    { const int w = kn_why(u,g);
      why[u] = (uint8_t)w;
      nisl += w == KN_ISLAND;
      ntip += w == KN_TIP;
      nbub += w == KN_BUBBLE;
      if (w != KN_KEPT) nbases += (unsigned long long)max(kn_bases(g,u),(int64_t)0);
    }
  kc_wave_add(ctl+CP_PRUNE_ISLANDS,nisl);
  kc_wave_add(ctl+CP_PRUNE_TIPS,ntip);
  kc_wave_add(ctl+CP_PRUNE_BUBBLES,nbub);
  kc_wave_add(ctl+CP_PRUNE_REMOVED_BASES,nbases);
}

// 0 the entry is not in, 1 it is kept, 2 it goes
__device__ static inline int kn_state(const int64_t *utg, const uint8_t *why, int64_t count, int64_t i)
{ const int64_t u = utg[i];
  return u < 0 ? 0 : why[min(u,count-1)] == KN_KEPT ? 1 : 2;
}

// tile_n[t] = the kept entries among [t*KS_TILE, (t+1)*KS_TILE); ctl += kept keys, removed keys
__global__ void __launch_bounds__(KS_BLOCK) kn_count_kernel(const int64_t *utg, const uint8_t *why, int64_t count, int64_t n,
                                                            int64_t *tile_n, unsigned long long *ctl)
{ __shared__ unsigned long long part[KS_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x*KS_TILE;
  unsigned long long kept = 0, gone = 0;
  for (int s = threadIdx.x; s < KS_TILE; s += KS_BLOCK)
    if (i0+s < n)
      { const int st = kn_state(utg,why,count,i0+s);
        kept += st == 1;
        gone += st == 2;
      }
  kc_wave_add(ctl+CP_PRUNE_KEPT_KEYS,kept);
  kc_wave_add(ctl+CP_PRUNE_REMOVED_KEYS,gone);
  if (!tile_n) return;
  const unsigned long long tot = ks_block_scan(kept,part);
  if (threadIdx.x == KS_BLOCK-1) tile_n[blockIdx.x] = (int64_t)tot;
}

// the predicate of the write pass (ks_keep_write_kernel): entry i is kept
struct kn_keep
  { const int64_t *utg;
    const uint8_t *why;
    int64_t count;
    __device__ bool operator()(int64_t i) const { return kn_state(utg,why,count,i) == 1; }
  };

// ---------------------------------------------------------------------------------------------------------------------
// host side

// the passes; scratch and the result's memory are freed by the caller when this fails
static int kn_run(const cp_kmer_sorted *s, const cp_unitigs *u, const int64_t *d_utg, const cp_unitig_graph *g,
                  const int64_t *d_weight, const int64_t *limits, uint8_t *d_why, int64_t *tally, hipStream_t st,
                  cp_kmer_sorted *res, void **scratch)
{ const char *who = "cp_kmer_sorted_unitig_prune";
  const int64_t count = u->count, n = s->n;
  int64_t ntile, nsum;
  int rc = so_derived_tiles(who,n,s->nb,res != nullptr,&ntile,&nsum);
  if (rc != CP_OK) return rc;
  unsigned long long h_ctl[KN_CTL];
  memset(h_ctl,0,sizeof(h_ctl));
  int64_t n_out = 0;
  int64_t *tile_n = nullptr;
  unsigned long long *sum = nullptr;
  const uint8_t *why = d_why;
  const bool entries = count > 0 && n > 0 && (res || tally);
  if (count > 0)
    { // the control block, the tile counts and the words of the scan, a mark per unitig
      const size_t words = KN_CTL+(res ? (size_t)(ntile+nsum) : 0);
      rc = ks_alloc(who,scratch,words*8+(d_why ? 0 : (size_t)count),"the tile counts and the marks");
      if (rc != CP_OK) return rc;
      unsigned long long *ctl = (unsigned long long *)*scratch;
      tile_n = res ? (int64_t *)(ctl+KN_CTL) : nullptr;
      sum = (unsigned long long *)(ctl+KN_CTL)+ntile;
      uint8_t *wr = d_why ? d_why : (uint8_t *)(ctl+words);
      why = wr;
      const kn_graph kg{ g->loff, g->link, u->off, u->flag, d_weight ? d_weight : u->kc, count, g->links, u->K,
                         limits[0], limits[1], limits[2] };
      HIPCHK(hipMemsetAsync(ctl,0,KN_CTL*8,st));
      kn_rule_kernel<<<(int)std::min<int64_t>((count+KT_BLOCK-1)/KT_BLOCK,16384),KT_BLOCK,0,st>>>(kg,wr,ctl);
      HIPCHK(hipGetLastError());
      if (entries)
        { kn_count_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(d_utg,why,count,n,tile_n,ctl);
          HIPCHK(hipGetLastError());
          if (res)
            { rc = so_derived_counted(tile_n,ntile,sum,st,n_out);
              if (rc != CP_OK) return rc;
            }
        }
      HIPCHK(hipMemcpyAsync(h_ctl,ctl,KN_CTL*8,hipMemcpyDeviceToHost,st));
    }
  HIPCHK(hipStreamSynchronize(st));
  if (res)
    { if (n_out < 0 || n_out > n) return set_err(CP_EHIP,std::string(who)+": internal: the tile counts do not add up");
      so_dest o;
      rc = so_derived_alloc(who,res,n_out,st,&o);
      if (rc != CP_OK) return rc;
      if (n_out > 0)
        { rc = so_derived_write(s,kn_keep{ d_utg, why, count },2*s->K > 63,ntile,tile_n,o,st);
          if (rc == CP_OK) rc = so_derived_starts(res,sum,st);
          if (rc != CP_OK) return rc;
        }
      HIPCHK(hipStreamSynchronize(st));
    }
  if (tally)
    { for (int k = 0; k < CP_PRUNE_WIDTH; k++) tally[k] = (int64_t)h_ctl[k];
      tally[CP_PRUNE_UNITIGS] = count;
    }
  return CP_OK;
}

extern "C" int cp_kmer_sorted_unitig_prune(const cp_kmer_sorted *s, const cp_unitigs *u, const int64_t *d_utg,
                                           const cp_unitig_graph *g, const int64_t *d_weight, const int64_t *limits,
                                           uint8_t *d_why, int64_t *tally, void *stream, cp_kmer_sorted **out)
{ const char *who = "cp_kmer_sorted_unitig_prune";
  if (out) *out = nullptr;
  if (!s || !u || !g || !limits || (!d_why && !tally && !out) || (u->count > 0 && !d_utg))
    return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!s->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (u->K != s->K) return set_err(CP_EINVAL,std::string(who)+": the unitigs are of another K than the snapshot");
  if (g->count != u->count) return set_err(CP_EINVAL,std::string(who)+": the graph is not of these unitigs");
  if (u->count > 0 && (!u->off || !u->flag || !u->kc || !g->loff || (g->links > 0 && !g->link) || s->n <= 0))
    return set_err(CP_EINVAL,std::string(who)+": the unitigs or the graph hold no arrays or are not of this snapshot");
  if (limits[0] < 0 || limits[1] < 0 || limits[2] < 0) return set_err(CP_EINVAL,std::string(who)+": a limit is negative");
  hipStream_t st = (hipStream_t)stream;
  cp_kmer_sorted *res = nullptr;
  if (out && so_derived_new(who,s,&res) != CP_OK) return CP_ENOMEM;
  void *scratch = nullptr;
  const int rc = kn_run(s,u,d_utg,g,d_weight,limits,d_why,tally,st,res,&scratch);
  return so_derived_finish(rc,st,scratch,res,out);
}

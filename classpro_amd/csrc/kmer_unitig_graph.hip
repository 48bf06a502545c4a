// kmer_unitig_graph.hip -- the links between the unitigs of ONE sorted snapshot and the connected components of the graph
// they form (tabgraph).  Semantics: include/classpro_amd.h, "Links between unitigs"; design: DESIGN.md 9.20.  Included by
// capi.hip after kmer_unitigs.hip (cp_unitigs, ug_succ, ug_find, ug_scan, kl_view, hp_rule, hp_revcomp, ks_alloc,
// kc_wave_add, set_err and HIPCHK are in scope).  The snapshot, the unitigs and the two where arrays are only read.
//   ends     one lane per ORIENTED unitig x = 2u+o.  The end k-mer is packed from the K bytes at the end of u's sequence
//            (o = 0) or from its first K bytes, reverse complemented (o = 1); its reverse complement is formed once, each
//            of the four successors by ug_succ, and each is looked up by ug_find, ONE SEARCH AFTER THE OTHER (the form
//            the adjacency pass keeps: lock-step searches measured slower in tab2prof, tabbin and tabhet).  A successor
//            that is found and in at entry j in state 2j+b is the start of the oriented unitig 2*utg[j] + (b ^ at[j]&1).
//            The lane stages its four targets (-1 for none) and stores its arc count: 8 look-ups per unitig, whatever its
//            length.
//   scan     ug_scan over the 2*count arc counts: loff.
//   write    one lane per oriented unitig again: its staged targets to link[] and base[] at loff[x], in ascending c; the
//            dead ends, tips and isolated unitigs from loff alone.
//   label    comp[u] = u, then rounds of two kernels until a round's hook lowers nothing:
//              hook      one lane per oriented unitig, over its arcs u - v: with a = comp[u], b = comp[v] and a != b,
//                        atomicMin(comp + max(a,b), min(a,b)), 64-bit, agent scope; a lane counts an atomicMin that
//                        lowered the slot.
//              shortcut  one lane per unitig: follows c = comp[c] from comp[u] until comp[c] == c, stores that into
//                        comp[u] (only lane u stores slot u here).
//            Why the end state is the component's minimum whatever the scheduling: three things hold after every store.
//            (1) comp[s] <= s: a slot only ever receives a minimum with a smaller value, or a value reached by following
//            such slots.  So following comp strictly descends until a root (comp[r] == r) and never cycles.  (2) comp[s]
//            is a unitig of s's component: a hook stores a label of one end of an arc into the slot named by the label
//            of the other end, and both labels are, by induction, in the component of the arc.  (3) a value read late
//            or from a stale copy is an older value of the slot, for which (1) and (2) held as well.  A hook kernel whose
//            lanes lowered nothing stored nothing, so each lane read the memory as the kernel found it and saw equal
//            labels on both ends of every arc: comp is constant on every component, by (2) that constant is a member m'
//            of it, and by (1) the component's smallest member m has comp[m] <= m, hence comp[m] = m = m'.  A round
//            that does lower a slot turns a root into a non-root, and nothing turns a non-root back, so there are at
//            most count rounds; the loop has no other cap.  Only the NUMBER of rounds depends on scheduling.
//   sizes    one lane per unitig: its bases added to sum[comp[u]] by 64-bit atomics, one per wave and label, the roots
//            counted; then the largest sum by an atomic max.
// All sums are integer atomics: nothing but CP_UGL_ROUNDS depends on grid, block size or scheduling.
enum { GL_CHANGED = CP_UGL_WIDTH, GL_CTL = CP_UGL_WIDTH+1 };        // words of the control block

struct cp_unitig_graph
  { int64_t count, links;
    int64_t *loff, *link;                  // 2*count+1 and links (null when count = 0, link also when links = 0)
    uint8_t *base;                         // links
    int64_t *comp;                         // count, null without want_comp
  };

__device__ static inline int64_t gl_clamp(int64_t v, int64_t n) { return min(max(v,(int64_t)0),n-1); }

// stage[4x+c] = the oriented unitig that x reaches by c, or -1; cnt[x] = how many it reaches; tally[SELF] += arcs into
// the source's own unitig
template <bool LO_ONLY>
__global__ void __launch_bounds__(KT_BLOCK) gl_end_kernel(kl_view t, int K, hp_rule r, const char *seq, const int64_t *off,
                                                          int64_t count, int64_t bases, const int64_t *utg, const int64_t *at,
                                                          int64_t *stage, int64_t *cnt, unsigned long long *tally)
{ unsigned long long nself = 0;
  for (int64_t x = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; x < 2*count; x += (int64_t)gridDim.x*blockDim.x)
    { const int64_t u = x >> 1, b0 = (x & 1) ? off[u] : off[u+1]-K;
      int64_t tgt[4] = { -1, -1, -1, -1 };
      int n = 0;
      if (b0 >= 0 && b0+K <= bases)
        { kt_u128 p = 0;
          for (int k = 0; k < K; k++)
            { const unsigned int v = ((unsigned int)(unsigned char)seq[b0+k] >> 1) & 3u;      // A C G T -> 0 1 3 2
              p = (p << 2) | (kt_u128)(v ^ (v >> 1));
            }
          const kt_u128 q = hp_revcomp(p,K), w = (x & 1) ? q : p, rc = (x & 1) ? p : q;
          for (int c = 0; c < 4; c++)
            { bool fwd, pal;
              const kt_u128 y = ug_succ(w,rc,K,c,&fwd,&pal);
              const int64_t j = ug_find<LO_ONLY>(t,y,r);
              if (j < 0) continue;
              const int64_t v = gl_clamp(utg[j],count);
              tgt[c] = 2*v+(int64_t)((fwd ? 0 : 1) ^ (int)(at[j] & 1));
              nself += v == u;
              n++;
            }
        }
      for (int c = 0; c < 4; c++) stage[4*x+c] = tgt[c];
      cnt[x] = n;
    }
  kc_wave_add(tally+CP_UGL_SELF,nself);
}

// the staged targets of x to link[] and base[] from loff[x] on; the dead ends, tips and isolated unitigs
__global__ void __launch_bounds__(KT_BLOCK) gl_write_kernel(const int64_t *stage, const int64_t *loff, int64_t count, int64_t links,
                                                            int64_t *link, uint8_t *base, unsigned long long *tally)
{ unsigned long long ndead = 0, ntip = 0, niso = 0;
  for (int64_t x = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; x < 2*count; x += (int64_t)gridDim.x*blockDim.x)
    { int64_t a = loff[x];
      const int64_t e = loff[x+1];
      for (int c = 0; c < 4; c++)
        { const int64_t y = stage[4*x+c];
          if (y < 0 || a >= e || a >= links) continue;
          link[a] = y;
          base[a] = (uint8_t)c;
          a++;
        }
      ndead += e == loff[x];
      if (!(x & 1))
        { const bool d0 = e == loff[x], d1 = loff[x+2] == e;
          ntip += d0 != d1;
          niso += d0 && d1;
        }
    }
  kc_wave_add(tally+CP_UGL_DEAD_ENDS,ndead);
  kc_wave_add(tally+CP_UGL_TIP_UNITIGS,ntip);
  kc_wave_add(tally+CP_UGL_ISOLATED_UNITIGS,niso);
}

__global__ void __launch_bounds__(KT_BLOCK) gl_init_kernel(int64_t *comp, unsigned long long *sum, int64_t count)
{ for (int64_t u = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; u < count; u += (int64_t)gridDim.x*blockDim.x)
    { comp[u] = u;
      sum[u] = 0;
    }
}

__device__ static inline int64_t gl_label(const int64_t *comp, int64_t s, int64_t count)
{ return gl_clamp(__hip_atomic_load(comp+s,__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT),count); }

// one hook over every arc; *changed += the slots it lowered
__global__ void __launch_bounds__(KT_BLOCK) gl_hook_kernel(const int64_t *loff, const int64_t *link, int64_t count, int64_t links,
                                                           int64_t *comp, unsigned long long *changed)
{ unsigned long long nch = 0;
  for (int64_t x = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; x < 2*count; x += (int64_t)gridDim.x*blockDim.x)
    { const int64_t e = min(loff[x+1],links);
      for (int64_t k = max(loff[x],(int64_t)0); k < e; k++)
        { const int64_t a = gl_label(comp,x >> 1,count), b = gl_label(comp,gl_clamp(link[k] >> 1,count),count);
          if (a == b) continue;
          const int64_t lo = min(a,b), hi = max(a,b);
          nch += __hip_atomic_fetch_min(comp+hi,lo,__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT) > lo;
        }
    }
  kc_wave_add(changed,nch);
}

// comp[u] = the root that following comp from u reaches
__global__ void __launch_bounds__(KT_BLOCK) gl_shortcut_kernel(int64_t *comp, int64_t count)
{ for (int64_t u = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; u < count; u += (int64_t)gridDim.x*blockDim.x)
    { int64_t c = gl_label(comp,u,count);
      for (int64_t d = gl_label(comp,c,count); d < c; d = gl_label(comp,c,count)) c = d;
      __hip_atomic_store(comp+u,c,__ATOMIC_RELAXED,__HIP_MEMORY_SCOPE_AGENT);
    }
}

// sum[comp[u]] += the bases of u; tally[COMPONENTS] += the roots.  The lanes of a wave that share a label add once: a
// component of millions of unitigs is ONE address, and an atomic per lane onto it took as long as everything else together
__global__ void __launch_bounds__(KT_BLOCK) gl_sum_kernel(const int64_t *comp, const int64_t *off, int64_t count,
                                                          unsigned long long *sum, unsigned long long *tally)
{ unsigned long long nroot = 0;
  for (int64_t u0 = (int64_t)blockIdx.x*blockDim.x; u0 < count; u0 += (int64_t)gridDim.x*blockDim.x)      // the same trips for a whole wave
    { const int64_t u = u0+threadIdx.x, c = u < count ? gl_clamp(comp[u],count) : -1;
      const unsigned long long len = u < count ? (unsigned long long)(off[u+1]-off[u]) : 0;
      nroot += c == u;
      for (unsigned long long todo = __ballot(c >= 0); todo; )
        { const int64_t lc = __shfl(c,__ffsll((long long)todo)-1);          // the label of the first lane still to add
          const bool mine = c == lc;
          kc_wave_add(sum+lc,mine ? len : 0);
          todo &= ~__ballot(mine);
        }
    }
  kc_wave_add(tally+CP_UGL_COMPONENTS,nroot);
}

__global__ void __launch_bounds__(KT_BLOCK) gl_max_kernel(const unsigned long long *sum, int64_t count, unsigned long long *tally)
{ unsigned long long big = 0;
  for (int64_t u = (int64_t)blockIdx.x*blockDim.x+threadIdx.x; u < count; u += (int64_t)gridDim.x*blockDim.x) big = max(big,sum[u]);
  for (int w = warpSize/2; w > 0; w >>= 1) big = max(big,(unsigned long long)__shfl_down(big,w));
  if ((threadIdx.x & (warpSize-1)) == 0 && big) atomicMax(tally+CP_UGL_LARGEST_BASES,big);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

static void gl_free(cp_unitig_graph *g)
{ if (!g) return;
  if (g->loff) (void)hipFree(g->loff);
  if (g->link) (void)hipFree(g->link);
  if (g->base) (void)hipFree(g->base);
  if (g->comp) (void)hipFree(g->comp);
  delete g;
}

// the passes; scratch and the result's memory are freed by the caller when this fails
static int gl_run(const cp_kmer_sorted *s, hp_rule r, const cp_unitigs *u, const int64_t *d_utg, const int64_t *d_at,
                  int64_t *tally, bool want_comp, hipStream_t st, cp_unitig_graph *res, void **scratch)
{ const char *who = "cp_kmer_sorted_unitig_links";
  const int64_t count = u->count, nx = 2*count;
  unsigned long long h_ctl[GL_CTL];
  memset(h_ctl,0,sizeof(h_ctl));
  int64_t rounds = 0;
  if (count > 0)
    { // the control block, four staged targets per oriented unitig, the words of the scan, a sum per unitig
      const int64_t nfirst = (nx+KS_CHUNK-1)/KS_CHUNK+2, nsecond = (nfirst+KS_CHUNK-1)/KS_CHUNK+1;
      const size_t words = GL_CTL+(size_t)(4*nx+nfirst+nsecond)+(want_comp ? (size_t)count : 0);
      int rc = ks_alloc(who,scratch,words*8,"the staged links and the scan");
      if (rc == CP_OK) rc = ks_alloc(who,(void **)&res->loff,(size_t)(nx+1)*8,"the link offsets");
      if (rc == CP_OK && want_comp) rc = ks_alloc(who,(void **)&res->comp,(size_t)count*8,"the component labels");
      if (rc != CP_OK) return rc;
      unsigned long long *ctl = (unsigned long long *)*scratch;
      int64_t *stage = (int64_t *)(ctl+GL_CTL);
      unsigned long long *first = (unsigned long long *)(stage+4*nx), *second = first+nfirst, *sum = second+nsecond;
      const kl_view t = kl_view_of(s);
      const int xgrid = (int)std::min<int64_t>((nx+KT_BLOCK-1)/KT_BLOCK,16384);
      const int ugrid = (int)std::min<int64_t>((count+KT_BLOCK-1)/KT_BLOCK,16384);
      HIPCHK(hipMemsetAsync(ctl,0,GL_CTL*8,st));
      HIPCHK(hipMemsetAsync(res->loff,0,8,st));
      if (kl_lo_only(s)) gl_end_kernel<true><<<xgrid,KT_BLOCK,0,st>>>(t,s->K,r,u->seq,u->off,count,u->bases,d_utg,d_at,stage,res->loff+1,ctl);
      else gl_end_kernel<false><<<xgrid,KT_BLOCK,0,st>>>(t,s->K,r,u->seq,u->off,count,u->bases,d_utg,d_at,stage,res->loff+1,ctl);
      HIPCHK(hipGetLastError());
      rc = ug_scan(res->loff+1,nx,first,second,st);
      if (rc != CP_OK) return rc;
      HIPCHK(hipMemcpyAsync(&res->links,res->loff+nx,8,hipMemcpyDeviceToHost,st));
      HIPCHK(hipStreamSynchronize(st));
      const int64_t links = res->links;
      if (links < 0 || links > 4*nx) return set_err(CP_EHIP,std::string(who)+": internal: the link counts do not add up");
      if (links > 0)
        { rc = ks_alloc(who,(void **)&res->link,(size_t)links*8,"the links");
          if (rc == CP_OK) rc = ks_alloc(who,(void **)&res->base,(size_t)links,"the bases of the links");
          if (rc != CP_OK) return rc;
        }
      gl_write_kernel<<<xgrid,KT_BLOCK,0,st>>>(stage,res->loff,count,links,res->link,res->base,ctl);
      HIPCHK(hipGetLastError());
      if (want_comp)
        { gl_init_kernel<<<ugrid,KT_BLOCK,0,st>>>(res->comp,sum,count);
          HIPCHK(hipGetLastError());
          for (unsigned long long changed = links > 0; changed > 0; rounds++)
            { HIPCHK(hipMemsetAsync(ctl+GL_CHANGED,0,8,st));
              gl_hook_kernel<<<xgrid,KT_BLOCK,0,st>>>(res->loff,res->link,count,links,res->comp,ctl+GL_CHANGED);
              HIPCHK(hipGetLastError());
              gl_shortcut_kernel<<<ugrid,KT_BLOCK,0,st>>>(res->comp,count);
              HIPCHK(hipGetLastError());
              HIPCHK(hipMemcpyAsync(&changed,ctl+GL_CHANGED,8,hipMemcpyDeviceToHost,st));
              HIPCHK(hipStreamSynchronize(st));
              if (rounds > count) return set_err(CP_EHIP,std::string(who)+": internal: the labels do not settle");
            }
          gl_sum_kernel<<<ugrid,KT_BLOCK,0,st>>>(res->comp,u->off,count,sum,ctl);
          HIPCHK(hipGetLastError());
          gl_max_kernel<<<ugrid,KT_BLOCK,0,st>>>(sum,count,ctl);
          HIPCHK(hipGetLastError());
        }
      HIPCHK(hipMemcpyAsync(h_ctl,ctl,GL_CTL*8,hipMemcpyDeviceToHost,st));
    }
  HIPCHK(hipStreamSynchronize(st));
  res->count = count;
  if (tally)
    { for (int k = 0; k < CP_UGL_WIDTH; k++) tally[k] = (int64_t)h_ctl[k];
      tally[CP_UGL_LINKS] = res->links;
      tally[CP_UGL_ROUNDS] = rounds;
    }
  return CP_OK;
}

extern "C" int cp_kmer_sorted_unitig_links(const cp_kmer_sorted *s, const int64_t *range, const cp_unitigs *u, const int64_t *d_utg,
                                           const int64_t *d_at, int64_t *tally, int want_comp, void *stream, cp_unitig_graph **out)
{ const char *who = "cp_kmer_sorted_unitig_links";
  if (out) *out = nullptr;
  if (!s || !u || (!tally && !out) || (u->count > 0 && (!d_utg || !d_at))) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!s->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  if (u->K != s->K) return set_err(CP_EINVAL,std::string(who)+": the unitigs are of another K than the snapshot");
  if (u->count > 0 && (!u->seq || !u->off || s->n <= 0))
    return set_err(CP_EINVAL,std::string(who)+": the unitigs hold no sequences or are not of this snapshot");
  hp_rule r{ 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0]) return set_err(CP_EINVAL,std::string(who)+": a count range needs 1 <= min <= max");
      r.cmin = (unsigned long long)range[0];
      r.cmax = (unsigned long long)range[1];
    }
  hipStream_t st = (hipStream_t)stream;
  cp_unitig_graph *res = new (std::nothrow) cp_unitig_graph();
  if (!res) return set_err(CP_ENOMEM,std::string(who)+": out of memory");
  void *scratch = nullptr;
  const int rc = gl_run(s,r,u,d_utg,d_at,tally,want_comp != 0,st,res,&scratch);
  if (rc != CP_OK) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  if (rc != CP_OK || !out)
    { gl_free(res);
      return rc;
    }
  *out = res;
  return CP_OK;
}

extern "C" int64_t cp_unitig_graph_links(const cp_unitig_graph *g) { return g ? g->links : 0; }

extern "C" int cp_unitig_graph_arrays(const cp_unitig_graph *g, const int64_t **d_loff, const int64_t **d_link, const uint8_t **d_base,
                                      const int64_t **d_comp)
{ if (!g) return set_err(CP_EINVAL,"cp_unitig_graph_arrays: bad argument");
  if (d_loff) *d_loff = g->loff;
  if (d_link) *d_link = g->link;
  if (d_base) *d_base = g->base;
  if (d_comp) *d_comp = g->comp;
  return CP_OK;
}

extern "C" void cp_unitig_graph_destroy(cp_unitig_graph *g) { gl_free(g); }

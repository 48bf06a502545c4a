// kmer_hetpairs.hip -- the heterozygous k-mer pairs of ONE sorted snapshot (tabhet): every key is paired with the keys
// that differ from it, in some orientation, only at the centre base; the 2-D histogram of the two counts of such pairs
// (the first step of Smudgeplot), the degree of every key, and the paired keys as a snapshot of their own.  Semantics:
// include/classpro_amd.h, "Heterozygous pairs of sorted k-mers"; design: DESIGN.md 9.17.  Included by capi.hip after
// kmer_cmphist.hip (kl_view, kl_find_group, the ks_keep_ kernels and the so_derived_ helpers of kmer_setops.hip, CM_CX,
// CM_CY, cm_put, ks_alloc, kc_wave_add, set_err and HIPCHK are in scope).  The operand is only read.
//   key      one lane per entry.  X = hi << 63 | lo as 128 bits; rc(X) once per key: the 64 two-bit groups of the 128 bits
//            reversed (a bit reversal and a swap inside every pair), shifted down to 2K bits and complemented.
//   sibling  a candidate is min(sub(X, p, c), sub(rcX, K-1-p, 3-c)) for p = m = K/2 and, where K is even, p = K-1-m, and
//            the three c that are not X's base at p; X itself and repeats are dropped (at most 8 compares of 128 bits).
//            Every candidate is looked up by kl_find_group (clamped ranges, at most 64 probes); a sibling is a candidate
//            that is found and whose count lies in the range.  The substituted base may straddle hi and lo (a shift of
//            62 at K = 62 and 63): all of this is arithmetic on kt_u128.
//   degree   the first pass: deg[i] = the siblings of entry i, one byte, and four of the tally's sums.
//   pair     the second pass: an entry with a degree looks its candidates ABOVE itself up once more, so that a pair is met
//            once, from its smaller key; it reads the partner's byte, decides unique or not, and adds the cell: the low
//            corner of the matrix is 64-bit counters in LDS (tabcmp's), everything else a 64-bit atomic on the matrix.
//            With a result wanted in unique mode it sets bit 7 in both members' bytes: a unique pair's two bytes are
//            written by that one lane alone, with the value every reader expects under the mask.
//   stage    CLASSPRO_HET_STAGE=1, the A/B form: a block stages its tile of KS_TILE consecutive entries in LDS (48 KiB) and
//            searches a candidate that lies between the tile's first and last key there (cm_tile_kernel's partner search);
//            only the others go to kl_find_group.  Same results; the build's default is HP_STAGE.
//   result   the compaction by a predicate of kmer_setops.hip (ks_keep_count_kernel, ks_keep_write_kernel, so_derived_*)
//            with "is a member" as the predicate.  The write pass's predicate clears bit 7 again, so after a call that
//            succeeds a caller's d_deg holds plain degrees; that is why it runs even when no entry is a member.
// All sums are integer atomics: nothing depends on grid, block size or scheduling.
#define HP_PER_CU   6                      // persistent blocks of the pair pass per CU: what 24 KiB of corner leave resident
#define HP_PER_CU_STAGED 2                 // ... and what 72 KiB of corner and staged tile leave
#define HP_STAGE    0                      // the staged form (CLASSPRO_HET_STAGE; measured: DESIGN.md 9.17)
#define HP_MEMBER   0x80u                  // bit 7 of a degree byte: a member of a unique pair (between the passes only)
#define HP_DEG      0x7fu

struct hp_rule { unsigned long long cmin, cmax; };

__device__ static inline unsigned long long hp_rev2(unsigned long long x)  // the 32 two-bit groups of x in reverse order
{ x = __brevll(x);
  return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
}

__device__ static inline kt_u128 hp_revcomp(kt_u128 x, int K)
{ const kt_u128 r = (((kt_u128)hp_rev2((unsigned long long)x)) << 64) | (kt_u128)hp_rev2((unsigned long long)(x >> 64));
  return (r >> (128-2*K)) ^ ((((kt_u128)1) << (2*K))-1);
}

// A block's tile of consecutive entries [base, base+n) staged in LDS (STAGE), and the keys it spans.
struct hp_slice
  { const unsigned long long *hi, *lo, *cnt;
    int n;
    int64_t base;
    kt_u128 first, last;
  };

// Loads the tile into LDS and returns its view; without STAGE nothing is loaded and no candidate falls inside it.
template <bool STAGE>
__device__ static inline hp_slice hp_stage(const kl_view &t, bool with_hi, int64_t i0, int nt, unsigned long long *shi,
                                           unsigned long long *slo, unsigned long long *scn)
{ hp_slice sl{ shi, slo, scn, STAGE ? nt : 0, i0, 1, 0 };
  if (!STAGE) return sl;
  for (int s = threadIdx.x; s < nt; s += KT_BLOCK)
    { shi[s] = with_hi ? t.hi[i0+s] : 0;
      slo[s] = t.lo[i0+s];
      scn[s] = t.cnt[i0+s];
    }
  __syncthreads();
  if (nt > 0)
    { sl.first = (((kt_u128)shi[0]) << 63) | (kt_u128)slo[0];
      sl.last = (((kt_u128)shi[nt-1]) << 63) | (kt_u128)slo[nt-1];
    }
  return sl;
}

// Calls f(ordinal, count) for every sibling of the key (kh, kl) -- with above_only, for those above the key alone.
// STAGE: a candidate between the first and the last key of the block's tile is searched for in LDS and nowhere else.
template <bool LO_ONLY, bool STAGE, class F>
__device__ static inline void hp_siblings(const kl_view &t, const hp_slice &sl, unsigned long long kh, unsigned long long kl,
                                          int K, hp_rule r, bool above_only, F f)
{ const kt_u128 x = (((kt_u128)kh) << 63) | (kt_u128)kl, rc = hp_revcomp(x,K);
  const int m = K >> 1, np = (K & 1) ? 1 : 2;
  kt_u128 seen[8];
  bool live[8];
#pragma unroll
  for (int q = 0; q < 8; q++)
    { const int j = q >> 2, c = q & 3;
      live[q] = false;
      seen[q] = 0;
      if (j >= np) continue;
      const int p = j ? K-1-m : m;
      const int sh = 2*(K-1-p), rsh = 2*p;                 // the base at p of X is the base at K-1-p of rc(X)
      if ((int)((unsigned long long)(x >> sh) & 3) == c) continue;
      const kt_u128 fw = (x & ~(((kt_u128)3) << sh)) | (((kt_u128)c) << sh);
      const kt_u128 bw = (rc & ~(((kt_u128)3) << rsh)) | (((kt_u128)(3-c)) << rsh);
      const kt_u128 y = fw < bw ? fw : bw;
      bool fresh = y != x && (!above_only || y > x);
#pragma unroll
      for (int o = 0; o < q; o++) fresh = fresh && !(live[o] && seen[o] == y);
      if (!fresh) continue;
      live[q] = true;
      seen[q] = y;
      const unsigned long long qh[1] = { (unsigned long long)(y >> 63) }, ql[1] = { (unsigned long long)y & KT_M63 };
      int64_t at;
      unsigned long long cy;
      if (STAGE && y >= sl.first && y <= sl.last)
        { int a = 0, e = sl.n;                             // the first entry of the tile that is not below the candidate
          for (int step = 0; step < 16 && a < e; step++)
            { const int mid = (a+e) >> 1;
              if (sl.hi[mid] < qh[0] || (sl.hi[mid] == qh[0] && sl.lo[mid] < ql[0])) a = mid+1; else e = mid;
            }
          a = min(a,sl.n-1);
          if (sl.lo[a] != ql[0] || sl.hi[a] != qh[0]) continue;
          at = sl.base+a;
          cy = sl.cnt[a];
        }
      else
        { int64_t pos[1];
          kl_find_group<LO_ONLY,KL_INTERP != 0,1>(t,qh,ql,1,pos);
          if (pos[0] < 0) continue;
          at = min(max(pos[0],(int64_t)0),t.n-1);
          cy = t.cnt[at];
        }
      if (cy >= r.cmin && cy <= r.cmax) f(at,cy);
    }
}

// deg[i] = the siblings of entry i; tally += in keys, keys with a sibling, keys with two or more, the sum of the degrees
// Block b takes the tiles b, b + gridDim.x, ... of KS_TILE consecutive entries.
template <bool LO_ONLY, bool STAGE>
__global__ void __launch_bounds__(KT_BLOCK) hp_degree_kernel(kl_view t, int K, hp_rule r, uint8_t *deg,
                                                             unsigned long long *tally)
{ __shared__ unsigned long long shi[STAGE ? KS_TILE : 1], slo[STAGE ? KS_TILE : 1], scn[STAGE ? KS_TILE : 1];
  unsigned long long nkeys = 0, npaired = 0, nmulti = 0, nsum = 0;
  const int64_t ntile = (t.n+KS_TILE-1)/KS_TILE;
  const bool with_hi = 2*K > 63;                           // below that hi[] is zero for every key and is not loaded
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x)
    { const int64_t i0 = tile*KS_TILE;
      const int nt = (int)min((int64_t)KS_TILE,t.n-i0);
      const hp_slice sl = hp_stage<STAGE>(t,with_hi,i0,nt,shi,slo,scn);
      for (int s = threadIdx.x; s < nt; s += KT_BLOCK)
        { const int64_t i = i0+s;
          const unsigned long long cx = STAGE ? scn[s] : t.cnt[i];
          unsigned int d = 0;
          if (cx >= r.cmin && cx <= r.cmax)
            { hp_siblings<LO_ONLY,STAGE>(t,sl,STAGE ? shi[s] : with_hi ? t.hi[i] : 0,STAGE ? slo[s] : t.lo[i],K,r,false,
                                         [&](int64_t, unsigned long long) { d++; });
              nkeys++;
              npaired += d >= 1;
              nmulti += d >= 2;
              nsum += d;
            }
          deg[i] = (uint8_t)d;
        }
      if (STAGE) __syncthreads();                          // the tile is read to the end before the next load
    }
  kc_wave_add(tally+CP_HET_KEYS,nkeys);
  kc_wave_add(tally+CP_HET_PAIRED,npaired);
  kc_wave_add(tally+CP_HET_MULTI,nmulti);
  kc_wave_add(tally+CP_HET_PAIRS,nsum);                    // twice the pairs: halved on the host
}

// the pairs, each from its smaller key: the cells, tally[CP_HET_UNIQUE], and with `mark` bit 7 of the members' bytes
template <bool LO_ONLY, bool STAGE>
__global__ void __launch_bounds__(KT_BLOCK) hp_pair_kernel(kl_view t, int K, hp_rule r, uint8_t *deg, bool unique, bool mark,
                                                           int xmax, int ymax, bool use_corner, unsigned long long *mat,
                                                           unsigned long long *tally)
{ __shared__ unsigned long long shi[STAGE ? KS_TILE : 1], slo[STAGE ? KS_TILE : 1], scn[STAGE ? KS_TILE : 1];
  __shared__ unsigned long long corner[CM_CX*CM_CY];
  const int ny = ymax+1, cells = (xmax+1)*ny;
  for (int i = threadIdx.x; i < CM_CX*CM_CY; i += KT_BLOCK) corner[i] = 0;
  __syncthreads();
  unsigned long long nuniq = 0;
  const int64_t ntile = (t.n+KS_TILE-1)/KS_TILE;
  const bool with_hi = 2*K > 63;                           // below that hi[] is zero for every key and is not loaded
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x)
    { const int64_t i0 = tile*KS_TILE;
      const int nt = (int)min((int64_t)KS_TILE,t.n-i0);
      const hp_slice sl = hp_stage<STAGE>(t,with_hi,i0,nt,shi,slo,scn);
      for (int s = threadIdx.x; s < nt; s += KT_BLOCK)
        { const int64_t i = i0+s;
          const unsigned int d = deg[i] & HP_DEG;
          if (d == 0 || (unique && d != 1)) continue;      // no pair, or none that is counted or unique
          const unsigned long long cx = STAGE ? scn[s] : t.cnt[i];
          hp_siblings<LO_ONLY,STAGE>(t,sl,STAGE ? shi[s] : with_hi ? t.hi[i] : 0,STAGE ? slo[s] : t.lo[i],K,r,true,
            [&](int64_t at, unsigned long long cy)
            { const bool uniq = d == 1 && (deg[at] & HP_DEG) == 1;
              nuniq += uniq;
              if (unique && !uniq) return;
              if (mat)
                { const int a = (int)min(min(cx,cy),(unsigned long long)xmax), b = (int)min(max(cx,cy),(unsigned long long)ymax);
                  cm_put(corner,use_corner,mat,ny,cells,a,b,1ull);
                }
              if (mark && unique)
                { deg[i] = (uint8_t)(HP_MEMBER | 1u);
                  deg[at] = (uint8_t)(HP_MEMBER | 1u);
                }
            });
        }
      if (STAGE) __syncthreads();                          // the tile is read to the end before the next load
    }
  kc_wave_add(tally+CP_HET_UNIQUE,nuniq);
  if (!use_corner || !mat) return;
  __syncthreads();
  for (int i = threadIdx.x; i < CM_CX*CM_CY; i += KT_BLOCK)
    { const unsigned long long c = corner[i];
      const int x = i/CM_CY, y = i%CM_CY;
      if (c && x <= xmax && y <= ymax) atomicAdd(&mat[min(x*ny+y,cells-1)],c);
    }
}

__device__ static inline bool hp_member(unsigned int d, bool unique)
{ return unique ? (d & HP_MEMBER) != 0 : (d & HP_DEG) != 0; }

// the predicates of the compaction (ks_keep_count_kernel, ks_keep_write_kernel): entry i is a member; the write pass also
// takes bit 7 out of its byte
struct hp_keep
  { const uint8_t *deg;
    bool unique;
    __device__ bool operator()(int64_t i) const { return hp_member(deg[i],unique); }
  };

struct hp_keep_clear
  { uint8_t *deg;
    bool unique;
    __device__ bool operator()(int64_t i) const
    { const unsigned int d = deg[i];
      if (d & HP_MEMBER) deg[i] = (uint8_t)(d & HP_DEG);
      return hp_member(d,unique);
    }
  };

// ---------------------------------------------------------------------------------------------------------------------
// host side

// the passes; scratch and the result's memory are freed by the caller when this fails
static int hp_run(const cp_kmer_sorted *s, hp_rule r, bool unique, int xmax, int ymax, bool use_corner, bool stage, int64_t *mat,
                  int64_t *tally, uint8_t *d_deg, hipStream_t st, cp_kmer_sorted *res, void **scratch)
{ const char *who = "cp_kmer_sorted_het_pairs";
  const kl_view t = kl_view_of(s);
  const bool lo_only = kl_lo_only(s), with_hi = 2*s->K > 63;
  const size_t cells = mat ? (size_t)(xmax+1)*(size_t)(ymax+1) : 0;
  int64_t ntile, nsum;
  int rc = so_derived_tiles(who,s->n,s->nb,res != nullptr,&ntile,&nsum);
  if (rc != CP_OK) return rc;
  unsigned long long h_tally[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
  int64_t n_out = 0;
  int64_t *tile_n = nullptr;
  unsigned long long *sum = nullptr;
  uint8_t *deg = d_deg;
  if (s->n > 0)
    { const size_t words = 8+cells+(res ? (size_t)(ntile+nsum) : 0);
      rc = ks_alloc(who,scratch,words*8+(d_deg ? 0 : (size_t)s->n),"the matrix, the tile counts and the degrees");
      if (rc != CP_OK) return rc;
      unsigned long long *d_tally = (unsigned long long *)*scratch, *d_mat = mat ? d_tally+8 : nullptr;
      tile_n = (int64_t *)(d_tally+8+cells);
      sum = (unsigned long long *)tile_n+ntile;
      if (!d_deg) deg = (uint8_t *)(d_tally+words);
      HIPCHK(hipMemsetAsync(d_tally,0,(8+cells)*8,st));
      const int grid = (int)std::min<int64_t>(ntile,8192);
#define HP_LAUNCH(KERNEL,GRID,...) do { if (lo_only) { if (stage) KERNEL<true,true><<<GRID,KT_BLOCK,0,st>>>(__VA_ARGS__); \
                                                       else KERNEL<true,false><<<GRID,KT_BLOCK,0,st>>>(__VA_ARGS__); } \
                                        else if (stage) KERNEL<false,true><<<GRID,KT_BLOCK,0,st>>>(__VA_ARGS__); \
                                        else KERNEL<false,false><<<GRID,KT_BLOCK,0,st>>>(__VA_ARGS__); } while (0)
      HP_LAUNCH(hp_degree_kernel,grid,t,s->K,r,deg,d_tally);
      HIPCHK(hipGetLastError());
      if (mat || tally || res)
        { int dev = 0, ncu = 0;
          HIPCHK(hipGetDevice(&dev));
          HIPCHK(hipDeviceGetAttribute(&ncu,hipDeviceAttributeMultiprocessorCount,dev));
          const int pgrid = std::min(grid,std::max(ncu,1)*(stage ? HP_PER_CU_STAGED : HP_PER_CU));    // persistent: the corner lives across it
          const bool mark = res != nullptr;
          HP_LAUNCH(hp_pair_kernel,pgrid,t,s->K,r,deg,unique,mark,xmax,ymax,use_corner,d_mat,d_tally);
#undef HP_LAUNCH
          HIPCHK(hipGetLastError());
        }
      if (res)
        { ks_keep_count_kernel<<<(unsigned)ntile,KS_BLOCK,0,st>>>(hp_keep{ deg, unique },s->n,tile_n);
          HIPCHK(hipGetLastError());
          rc = so_derived_counted(tile_n,ntile,sum,st,n_out);
          if (rc != CP_OK) return rc;
        }
      HIPCHK(hipMemcpyAsync(h_tally,d_tally,64,hipMemcpyDeviceToHost,st));
      if (mat) HIPCHK(hipMemcpyAsync(mat,d_mat,cells*8,hipMemcpyDeviceToHost,st));
    }
  HIPCHK(hipStreamSynchronize(st));
  if (mat && s->n == 0) memset(mat,0,cells*8);
  if (res)
    { so_dest o;
      rc = so_derived_alloc(who,res,n_out,st,&o);
      if (rc != CP_OK) return rc;
      if (s->n > 0)                                        // also with no member: the pass takes bit 7 out of the bytes again
        { rc = so_derived_write(s,hp_keep_clear{ deg, unique },with_hi,ntile,tile_n,o,st);
          if (rc == CP_OK && n_out > 0) rc = so_derived_starts(res,sum,st);
          if (rc != CP_OK) return rc;
        }
      HIPCHK(hipStreamSynchronize(st));
    }
  if (tally)
    { for (int k = 0; k < CP_HET_WIDTH; k++) tally[k] = (int64_t)h_tally[k];
      tally[CP_HET_PAIRS] = (int64_t)(h_tally[CP_HET_PAIRS]/2);
      tally[CP_HET_OUT] = unique ? 2*tally[CP_HET_UNIQUE] : tally[CP_HET_PAIRED];
    }
  return CP_OK;
}

extern "C" int cp_kmer_sorted_het_pairs(const cp_kmer_sorted *s, const int64_t *range, int unique, int xmax, int ymax,
                                        int64_t *mat, int64_t *tally, uint8_t *d_deg, void *stream, cp_kmer_sorted **out)
{ const char *who = "cp_kmer_sorted_het_pairs";
  if (out) *out = nullptr;
  if (!s || (!mat && !tally && !d_deg && !out)) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!s->ready) return set_err(CP_EINVAL,std::string(who)+": the snapshot is still being loaded");
  hp_rule r{ 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0]) return set_err(CP_EINVAL,std::string(who)+": a count range needs 1 <= min <= max");
      r.cmin = (unsigned long long)range[0];
      r.cmax = (unsigned long long)range[1];
    }
  if (mat)
    { if (xmax < 1 || xmax > CP_MAX_KMER_CNT || ymax < 1 || ymax > CP_MAX_KMER_CNT)
        return set_err(CP_EINVAL,std::string(who)+": xmax and ymax must lie in [1, 32767]");
      if ((int64_t)(xmax+1)*(ymax+1) > CM_MAX_CELLS) return set_err(CP_EINVAL,std::string(who)+": more than 2^22 cells");
    }
  else xmax = ymax = 1;
  bool use_corner = true;                                  // A/B knob of scripts/hetpairs_bench.py and of the tests
  if (const char *e = getenv("CLASSPRO_HET_LDS")) use_corner = atoi(e) != 0;
  bool stage = HP_STAGE != 0;                              // the block's tile in LDS, candidates inside it resolved there
  if (const char *e = getenv("CLASSPRO_HET_STAGE")) stage = atoi(e) != 0;
  hipStream_t st = (hipStream_t)stream;
  cp_kmer_sorted *res = nullptr;
  if (out && so_derived_new(who,s,&res) != CP_OK) return CP_ENOMEM;
  void *scratch = nullptr;
  const int rc = hp_run(s,r,unique != 0,xmax,ymax,use_corner,stage,mat,tally,d_deg,st,res,&scratch);
  return so_derived_finish(rc,st,scratch,res,out);
}

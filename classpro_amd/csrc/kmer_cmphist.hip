// kmer_cmphist.hip -- the 2-D count comparison of two sorted snapshots (tabcmp): mat[min(cntA, xmax)][min(cntB, ymax)]
// over every key that is in A or in B, counting keys or summing either side's counts, and the k-mer QV that follows from
// such a matrix.  Semantics: include/classpro_amd.h, "Count comparison of sorted k-mers"; design: DESIGN.md 9.16.
// Included by capi.hip after kmer_setops.hip (so_view, so_less, so_cut_kernel, SO_CAP, ks_alloc, set_err and HIPCHK are
// in scope).  Both operands are only read.
//   cut      so_cut_kernel, unchanged: tiles of the merged sequence that never split an equal pair.
//   tile     the load and the in-LDS partner search of the count pass of so_tile_kernel.  The blocks are persistent: block
//            b takes the tiles b, b + gridDim.x, ... with a barrier between two tiles, so that what it sums on chip lives
//            across all of them.
//   cell     an A entry decides for itself and its partner, a B entry without a partner for itself.
//   corner   the cells with x < CM_CX and y < CM_CY are 64-bit counters in LDS, added to by LDS atomics and flushed to the
//            matrix once per block, the non-zero ones only; every other cell goes to the matrix by a 64-bit atomic.
//            There is no 32-bit counter anywhere, so no sum can wrap before 2^64.
// All sums are integer atomics: the matrix does not depend on tile size, grid or scheduling.  Every search has a constant
// bound and every index is clamped to its array.
// LDS of a block: the tile arrays (48 KiB with hi[], 32 KiB without) and CM_CX*CM_CY*8 = 24 KiB of corner, 72 KiB at most:
// two blocks per CU of 160 KiB.
#define CM_CX    32                        // rows of the corner
#define CM_CY    96                        // columns of the corner
#define CM_PER_CU 2                        // persistent blocks per CU: what the LDS above leaves resident
#define CM_MAX_CELLS (1 << 22)

// adds v to cell (x, y): in the corner when it lies there, otherwise in the matrix
__device__ static inline void cm_put(unsigned long long *corner, bool use_corner, unsigned long long *mat, int ny, int cells,
                                     int x, int y, unsigned long long v)
{ if (use_corner && x < CM_CX && y < CM_CY) atomicAdd(&corner[x*CM_CY+y],v);
  else atomicAdd(&mat[min(max(x*ny+y,0),cells-1)],v);
}

template <bool HI>
__global__ void __launch_bounds__(KS_BLOCK) cm_tile_kernel(so_view a, so_view b, unsigned long long amin,
                                                           unsigned long long amax, unsigned long long bmin,
                                                           unsigned long long bmax, const int64_t *ci, const int64_t *cj,
                                                           int64_t ntile, int weight, int xmax, int ymax, bool use_corner,
                                                           unsigned long long *mat)
{ __shared__ unsigned long long shi[HI ? SO_CAP : 1], slo[SO_CAP], scn[SO_CAP];
  __shared__ unsigned long long corner[CM_CX*CM_CY];
  const int ny = ymax+1, cells = (xmax+1)*ny;
  for (int i = threadIdx.x; i < CM_CX*CM_CY; i += KS_BLOCK) corner[i] = 0;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x)
    { const int64_t i0 = min(max(ci[t],(int64_t)0),a.n), j0 = min(max(cj[t],(int64_t)0),b.n);
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
      __syncthreads();                                     // the first one also orders the zeroed corner before its adds
      for (int s = threadIdx.x; s < nt; s += KS_BLOCK)
        { const bool is_a = s < na;
          const unsigned long long kh = HI ? shi[s] : 0, kl = slo[s];
          int x = is_a ? na : 0, x1 = is_a ? nt : na;      // the first entry of the other side that is not below the key
          const int xe = x1;
          for (int step = 0; step < 16 && x < x1; step++)
            { const int mid = (x+x1) >> 1;
              if (so_less<HI>(HI ? shi[mid] : 0,slo[mid],kh,kl)) x = mid+1; else x1 = mid;
            }
          const bool found = x < xe && slo[x] == kl && (!HI || shi[x] == kh);
          const unsigned long long ca = is_a ? scn[s] : 0, cb = is_a ? (found ? scn[x] : 0) : scn[s];
          const bool decides = is_a || !found;             // a B entry with a partner leaves the pair to it
          const bool in_a = decides && is_a && ca >= amin && ca <= amax;
          const bool in_b = decides && (!is_a || found) && cb >= bmin && cb <= bmax;
          if (!in_a && !in_b) continue;
          const int cx = in_a ? (int)min(ca,(unsigned long long)xmax) : 0;
          const int cy = in_b ? (int)min(cb,(unsigned long long)ymax) : 0;
          const unsigned long long v = weight == CP_CMP_KEYS ? 1 : weight == CP_CMP_A ? (in_a ? ca : 0) : (in_b ? cb : 0);
          cm_put(corner,use_corner,mat,ny,cells,cx,cy,v);
        }
      __syncthreads();                                     // the tile arrays are read to the end before the next load
    }
  if (!use_corner) return;
  __syncthreads();                                         // a block without a tile has not met one since the zeroing
  for (int i = threadIdx.x; i < CM_CX*CM_CY; i += KS_BLOCK)
    { const unsigned long long c = corner[i];
      const int x = i/CM_CY, y = i%CM_CY;
      if (c && x <= xmax && y <= ymax) atomicAdd(&mat[min(x*ny+y,cells-1)],c);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side

// the cuts and the matrix in one allocation; scratch is freed by the caller
static int cm_hist(const cp_kmer_sorted *a, const cp_kmer_sorted *b, const unsigned long long *rng, int weight, int xmax,
                   int ymax, bool with_hi, bool use_corner, int want_grid, int64_t *mat, hipStream_t st, void **scratch)
{ const char *who = "cp_kmer_sorted_compare_hist";
  const so_view va = so_view_of(a), vb = so_view_of(b);
  const int64_t tot = a->n+b->n, ntile = (tot+KS_TILE-1)/KS_TILE;
  const size_t cells = (size_t)(xmax+1)*(size_t)(ymax+1);
  if (ntile == 0)
    { HIPCHK(hipStreamSynchronize(st));
      memset(mat,0,cells*8);
      return CP_OK;
    }
  int rc = ks_alloc(who,scratch,(cells+2*(size_t)(ntile+1))*8,"the matrix and the cuts");
  if (rc != CP_OK) return rc;
  unsigned long long *d_mat = (unsigned long long *)*scratch;
  int64_t *ci = (int64_t *)(d_mat+cells), *cj = ci+ntile+1;
  int dev = 0, ncu = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&ncu,hipDeviceAttributeMultiprocessorCount,dev));
  int grid = (int)std::min<int64_t>(ntile,std::min(std::max(ncu,1)*CM_PER_CU,8192));      // persistent, and within kt_grid's bound
  if (want_grid > 0) grid = std::min(want_grid,grid);
  HIPCHK(hipMemsetAsync(d_mat,0,cells*8,st));
  const int cgrid = kt_grid((unsigned long long)ntile+1);
  if (with_hi) so_cut_kernel<true><<<cgrid,KT_BLOCK,0,st>>>(va,vb,ntile,ci,cj);
  else so_cut_kernel<false><<<cgrid,KT_BLOCK,0,st>>>(va,vb,ntile,ci,cj);
  if (with_hi) cm_tile_kernel<true><<<grid,KS_BLOCK,0,st>>>(va,vb,rng[0],rng[1],rng[2],rng[3],ci,cj,ntile,weight,xmax,ymax,use_corner,d_mat);
  else cm_tile_kernel<false><<<grid,KS_BLOCK,0,st>>>(va,vb,rng[0],rng[1],rng[2],rng[3],ci,cj,ntile,weight,xmax,ymax,use_corner,d_mat);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(mat,d_mat,cells*8,hipMemcpyDeviceToHost,st));
  HIPCHK(hipStreamSynchronize(st));
  return CP_OK;
}

extern "C" int cp_kmer_sorted_compare_hist(const cp_kmer_sorted *a, const cp_kmer_sorted *b, const int64_t *range, int weight,
                                           int xmax, int ymax, int64_t *mat, void *stream)
{ const char *who = "cp_kmer_sorted_compare_hist";
  if (!a || !b || !mat) return set_err(CP_EINVAL,std::string(who)+": bad argument");
  if (!a->ready || !b->ready) return set_err(CP_EINVAL,std::string(who)+": an operand is still being loaded");
  if (a->K != b->K)
    { char m[120];
      snprintf(m,sizeof(m),"%s: the operands hold %d-mers and %d-mers",who,a->K,b->K);
      return set_err(CP_EINVAL,m);
    }
  unsigned long long rng[4] = { 1, (unsigned long long)INT64_MAX, 1, (unsigned long long)INT64_MAX };
  if (range)
    { if (range[0] < 1 || range[1] < range[0] || range[2] < 1 || range[3] < range[2])
        return set_err(CP_EINVAL,std::string(who)+": a count range needs 1 <= min <= max");
      for (int k = 0; k < 4; k++) rng[k] = (unsigned long long)range[k];
    }
  if (weight < CP_CMP_KEYS || weight > CP_CMP_B) return set_err(CP_EINVAL,std::string(who)+": weight must lie in [0, 2]");
  if (xmax < 1 || xmax > CP_MAX_KMER_CNT || ymax < 1 || ymax > CP_MAX_KMER_CNT)
    return set_err(CP_EINVAL,std::string(who)+": xmax and ymax must lie in [1, 32767]");
  if ((int64_t)(xmax+1)*(ymax+1) > CM_MAX_CELLS) return set_err(CP_EINVAL,std::string(who)+": more than 2^22 cells");
  const bool with_hi = 2*a->K > 63;                        // below that hi[] is zero for every key
  bool use_corner = true;                                  // A/B knobs of scripts/cmphist_bench.py and of the tests
  if (const char *e = getenv("CLASSPRO_CMP_LDS")) use_corner = atoi(e) != 0;
  int want_grid = 0;
  if (const char *e = getenv("CLASSPRO_CMP_GRID")) want_grid = std::max(atoi(e),1);
  hipStream_t st = (hipStream_t)stream;
  void *scratch = nullptr;
  const int rc = cm_hist(a,b,rng,weight,xmax,ymax,with_hi,use_corner,want_grid,mat,st,&scratch);
  if (rc != CP_OK) (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  return rc;
}

extern "C" int cp_kmer_qv(int K, int64_t a_only, int64_t a_total, double *qv, double *err)
{ if (!qv || !err) return set_err(CP_EINVAL,"cp_kmer_qv: bad argument");
  if (K < 1 || a_total <= 0 || a_only < 0 || a_only > a_total)
    return set_err(CP_EINVAL,"cp_kmer_qv: needs K >= 1 and 0 <= a_only <= a_total, a_total > 0");
  *err = 1.0-pow(1.0-(double)a_only/(double)a_total,1.0/(double)K);
  *qv = a_only == 0 ? INFINITY : -10.0*log10(*err);
  return CP_OK;
}

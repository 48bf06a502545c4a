// rel_anchor_probe.cpp -- TEST-ONLY (tests/test_rel_anchor_cells.py).  One direction of classify_rel (cp_class.h, sequential
// form, with the coverage heuristics and the optional second pass of cp_rel_dir_full) under either cell policy:
//   anchored = 0: cp_cell, the anchors of cp_dh_ratio looked up through `eff` (a view that also counts the look-ups
//                 that land on a stand-in, eff[k] != k);
//   anchored = 1: cp_cell_anc, the anchors' (end_pos, end_cnt) pairs carried in the cells, no view.
// This library is never loaded by the product (classpro_amd/), only by tests/.
#include <cstring>
#include <cmath>
#include <cstdlib>
#include <vector>
#include "../classpro_amd/csrc/cp_host_setup.h"
#include "../classpro_amd/csrc/cp_class.h"

struct counting_view                 // cp_aos_view that counts the look-ups answered by another interval's data
  { const cp_intvl *rintvl; const int *eff; long long *standins;
    cp_riv operator()(int k) const
    { if (eff[k] != k) ++*standins;
      return cp_riv_of(rintvl[eff[k]]);
    }
  };

extern "C" {

void *rap_params_new(int K, int read_len, int hcov, int dcov)
{ cp_dev_params *P = (cp_dev_params *)malloc(sizeof(cp_dev_params));
  if (cp_host_fill_params(P,K,read_len,hcov,dcov) != CP_OK) { free(P); return NULL; }
  return P;
}
void rap_params_free(void *P) { free(P); }

// asgn_dp[M] (the traceback of the last pass), asgn[M] (after cp_rel_post2), parent[M*4], rpos[M] out; hdrr_bits: the bits of the double cp_rel_post2 returns;
// standins: added to.  Returns 1 when the pass was repeated, 0 when not.
int rap_direction(void *Pv, const cp_intvl *rintvl, int M, int plen, int F, int anchored,
                  int8_t *asgn_dp, int8_t *asgn, int8_t *parent, uint8_t *rpos, uint64_t *hdrr_bits, long long *standins)
{ const cp_dev_params *P = (const cp_dev_params *)Pv;
  int COV[4] = { P->cov[0], P->cov[1], P->cov[2], P->cov[3] };
  std::vector<int> eff(M);
  cp_aos_rv rv; rv.rintvl = rintvl;
  counting_view cv; cv.rintvl = rintvl; cv.eff = eff.data(); cv.standins = standins;
  bool rerun = false;
  for (int pass = 0; pass < 2; pass++)
    { if (anchored) cp_rel_direction_c<cp_cell_anc>(P,rintvl,M,plen,F,COV,parent,eff.data(),rpos,asgn,cp_no_view());
      else          cp_rel_direction_c<cp_cell>(P,rintvl,M,plen,F,COV,parent,eff.data(),rpos,asgn,cv);
      if (pass == 1) break;
      rerun = cp_rel_post1(P,rv,M,F,asgn,COV);
      if (!rerun) break;
    }
  memcpy(asgn_dp,asgn,(size_t)M);
  const double hdrr = cp_rel_post2(P,rv,M,F,asgn,rerun);
  memcpy(hdrr_bits,&hdrr,sizeof(double));
  return rerun ? 1 : 0;
}

}

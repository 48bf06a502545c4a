// rel_cell_probe.cpp -- TEST-ONLY (tests/test_rel_cell_layout.py).  The DP cell of the main class of k_classify_rel_grp as it
// lies in LDS (cp_class.h: cp_cell_piece, cp_cell_pack / cp_cell_unpack, cp_rel_cell_off, cp_rel_record_bytes), compiled
// for the host.  This library is never loaded by the product (classpro_amd/), only by tests/.
#include <cstring>
#include <cmath>
#include "../classpro_amd/csrc/cp_host_setup.h"
#include "../classpro_amd/csrc/cp_class.h"

static_assert(sizeof(cp_cell_piece) == 16 && alignof(cp_cell_piece) == 16,"a piece is one 128-bit access");

extern "C" {

int rcp_cell_off(int g, int d, int s, int p) { return cp_rel_cell_off(g,d,s,p); }
int rcp_cells_bytes(void) { return CP_REL_CELLS_BYTES; }
int rcp_record_bytes(int maxm) { return cp_rel_record_bytes(maxm); }
int rcp_pieces(void) { return CP_PC_N; }
int rcp_none(void) { return CP_NONE; }

// A cell from its fields -> the four pieces -> a cell again.  in / out: dp, dhr; iv[15] = pos[R,H,D], cnt[R,H,D], lastH, lastD,
// lastHbD, lastDbH, anc[0..3] (as int32 bit patterns), then nothing.  pieces: the 64 packed bytes.
void rcp_round_trip(const double *dv_in, const int32_t *iv_in, double *dv_out, int32_t *iv_out, uint8_t *pieces)
{ cp_cell_anc c, r;
  c.dp = dv_in[0]; c.dhr = dv_in[1];
  c.pos[0] = 12345; c.cnt[0] = 54321;                    // the E entries: not kept, read back as 0
  for (int k = 0; k < 3; k++) { c.pos[k+1] = iv_in[k]; c.cnt[k+1] = iv_in[3+k]; }
  c.lastH = iv_in[6]; c.lastD = iv_in[7]; c.lastHbD = iv_in[8]; c.lastDbH = iv_in[9];
  for (int k = 0; k < 4; k++) c.anc[k] = (uint32_t)iv_in[10+k];
  cp_cell_piece p[CP_PC_N];
  cp_cell_pack(c,p);
  memcpy(pieces,p,sizeof p);
  memset(&r,0xa5,sizeof r);
  cp_cell_unpack(p,r);
  dv_out[0] = r.dp; dv_out[1] = r.dhr;
  for (int k = 0; k < 3; k++) { iv_out[k] = r.pos[k+1]; iv_out[3+k] = r.cnt[k+1]; }
  iv_out[6] = r.lastH; iv_out[7] = r.lastD; iv_out[8] = r.lastHbD; iv_out[9] = r.lastDbH;
  for (int k = 0; k < 4; k++) iv_out[10+k] = (int32_t)r.anc[k];
  iv_out[14] = r.pos[0]; iv_out[15] = r.cnt[0];
}

}

/*
 * ref_thres.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference's own calc_init_thres (wall.c:167-243) with the default error model, as a stand-alone program:
 *
 *     ref_thres H D out.bin
 *
 * calc_init_thres(NULL) -> load_emodel(NULL) fills pe[t][l] = 0.002 l^2 + 0.002 itself (wall.c:137-143) and never
 * calls load_himodel or polynomialfit: only the -M branch needs GSL.  oracle/Makefile `ref` therefore writes
 *     sed -n '1,8p;44,1051p' wall.c         (everything but the GSL include, line 9, and polynomialfit, 11-42)
 * into a temporary file outside the repo and this file #includes it as <wall_thres.inc>, after the same files
 * ref_driver.c includes before its own slice.  No line of it is edited and nothing stands in for polynomialfit:
 * load_himodel's call to it stays an unresolved symbol of the executable (the Makefile says why that is safe).
 *
 * This file holds only what ClassPro.c holds around that call: the includes, the globals of ClassPro.c:27-32, and a
 * main that sets GLOBAL_COV as ClassPro.c:537,544-547 do and writes what calc_init_thres left behind:
 *
 *     double  CMAX, HC_ERATE, lmax[3], pe[3][21]        (1 + 1 + 3 + 63 doubles; pe beyond lmax[t] is 0)
 *     uint8   cthres[3][21][256][2][2]                  ([ctype][l][cout][INIT|FINAL][SELF|OTHERS]; the reference
 *                                                        sets l in 1..lmax[t], cout in 1..CMAX-1; 0 elsewhere)
 *
 * Too high a coverage ends in the reference's own exit(1) and message (wall.c:174-177) before anything is written.
 * Output: oracle/_ref/ref_thres (git-ignored).
 */
#include <stdio.h>
#include <stdlib.h>
#include <stdbool.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include <limits.h>

#include "ClassPro.h"

bool  VERBOSE;
int   READ_LEN;
bool  IS_DB;
bool  IS_DAM;
cnt_t GLOBAL_COV[N_STATE];

#include "const.c"
#include "prob.c"
#include "util.c"
#include "hist.c"
#include "context.c"
#include <wall_thres.inc>        /* wall.c:1-8,44-1051, made by oracle/Makefile (see the header) */

#define TH_LMAX 21               /* MAX_N_LC+1: rows l = 0..lmax[HP], the table's l extent for every t */

int main(int argc, char **argv)
{ if (argc != 4)
    { fprintf(stderr,"usage: ref_thres H D out.bin\n");
      return 2;
    }
  int hcov = atoi(argv[1]), dcov = atoi(argv[2]);
  if (hcov < 1 || dcov < 1 || dcov > 30000)
    { fprintf(stderr,"ref_thres: H and D must be positive counts\n");
      return 2;
    }
  VERBOSE = false; IS_DB = false; IS_DAM = false;
  READ_LEN = 20000;                                       /* not read by calc_init_thres */
  precompute_logfact();                                   /* ClassPro.c:537 */
  GLOBAL_COV[HAPLO]  = hcov;                              /* ClassPro.c:544-547 */
  GLOBAL_COV[DIPLO]  = dcov;
  GLOBAL_COV[ERROR]  = 1;
  GLOBAL_COV[REPEAT] = plus_sigma(GLOBAL_COV[DIPLO],N_SIGMA_RCOV);

  Error_Model *emodel = calc_init_thres(NULL);            /* ClassPro.c:554 without -M; exit(1) inside if too high */

  static double        head[2+N_CTYPE+N_CTYPE*TH_LMAX];
  static unsigned char tab[N_CTYPE][TH_LMAX][256][N_THRES][N_ETYPE];
  head[0] = CMAX;
  head[1] = HC_ERATE;
  for (int t = HP; t <= TS; t++)
    { if (emodel[t].lmax >= TH_LMAX)
        { fprintf(stderr,"ref_thres: lmax[%d] = %d does not fit %d rows\n",t,emodel[t].lmax,TH_LMAX);
          return 2;
        }
      head[2+t] = emodel[t].lmax;
      for (int l = 0; l <= emodel[t].lmax; l++)
        head[2+N_CTYPE+t*TH_LMAX+l] = emodel[t].pe[l];
      for (int l = 1; l <= emodel[t].lmax; l++)
        for (int c = 1; c < CMAX; c++)
          for (int s = INIT; s <= FINAL; s++)
            for (int e = SELF; e <= OTHERS; e++)
              tab[t][l][c][s][e] = emodel[t].cthres[l][c][s][e];
    }
  FILE *f = fopen(argv[3],"wb");
  if (f == NULL || fwrite(head,sizeof(head),1,f) != 1 || fwrite(tab,sizeof(tab),1,f) != 1 || fclose(f) != 0)
    { fprintf(stderr,"ref_thres: cannot write %s\n",argv[3]);
      return 2;
    }
  return 0;
}

/*
 * ref_driver.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Thin export layer over the reference's OWN source files, compiled where they lie under
 * /root/reference/src (nothing is copied into this repo).  ClassPro is a unity build whose hot-path
 * functions are `static inline`, so the only way to call them is to #include the .c files into one
 * translation unit, exactly as ClassPro.c:16-25 does.  This driver includes every hot-path file that
 * compiles from the image's own headers:
 *     const.c  prob.c(+bessel.c)  util.c  hist.c  context.c  class_rel.c  class_unrel.c  seed.c(+nthash.h, kdq.h)
 * and is linked with libfastk.c (which includes gene_core.c), DB.c and QV.c (DB.c:38 defines Prog_Name),
 * the same objects the reference links into ClassPro (src/Makefile:23-24).
 *
 * wall.c: `#include <gsl/gsl_multifit.h>` (wall.c:9) cannot be satisfied -- GSL is not installed and
 * src/gsl-2.7.tar.gz is a missing blob; no stand-in header is provided.  Only the -M quadratic fit needs GSL:
 * `polynomialfit` (11-42), called by `load_himodel` (55-115) alone, which `load_emodel` (120-165) <- `calc_init_thres`
 * (167-243) reaches only when a model file is named.  This library leaves lines 9-115 and the threshold builder out.
 * Everything else of the file compiles as it stands: oracle/Makefile `ref` pipes
 *     sed -n '1,8p;117,118p;245,1051p' wall.c      (headers; `CMAX`, `HC_ERATE`; alloc_wall_arg ... find_rel_intvl)
 * into a temporary file OUTSIDE the repo (deleted after the compile; nothing of it is committed) and this driver
 * #includes it as <wall_gslfree.inc> when REF_HAVE_WALL is defined: the reference's own text for find_wall,
 * find_gain/find_drop, correct_wall_cnt, find_rel_intvl and their helpers, no line edited, no stub.
 * `find_wall` takes the Error_Model as a PARAMETER; `ref_wall_setup` fills one from a table the caller hands in
 * (calc_init_thres(NULL) itself, wall.c:167-243 with the default error model, is built as a program of its own,
 * oracle/_ref/ref_thres from oracle/ref_thres.c: its table is what the tests hand in here, and what pins the oracle's and
 * the product's, tests/test_oracle_thres.py).
 *
 * The globals below are the ones ClassPro.c:27-32 defines for the unity build.
 * Output: oracle/_ref/libclasspro_ref.so (git-ignored; travels to the GPU box with gpurun).
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
#include "class_rel.c"
#include "class_unrel.c"
#include "seed.c"
#ifdef REF_HAVE_WALL
#include <wall_gslfree.inc>      /* wall.c:1-8,117-118,245-1051, made by oracle/Makefile (see the header) */
#endif

/* ---- setup (what ClassPro.c:536-548 does, minus calc_init_thres which lives in wall.c) ---- */
void ref_setup(int read_len, int hcov, int dcov)
{ static int done = 0;
  VERBOSE = false; IS_DB = false; IS_DAM = false;
  READ_LEN = read_len;
  if (!done) { precompute_logfact(); done = 1; }
  GLOBAL_COV[HAPLO]  = hcov;
  GLOBAL_COV[DIPLO]  = dcov;
  GLOBAL_COV[ERROR]  = 1;
  GLOBAL_COV[REPEAT] = plus_sigma(GLOBAL_COV[DIPLO],N_SIGMA_RCOV);
  DR_RATIO = 1.+(double)N_SIGMA_R*(1./sqrt(GLOBAL_COV[DIPLO]));
}
void ref_globals(int *cov4, double *dr_ratio)
{ for (int i = 0; i < 4; i++) cov4[i] = GLOBAL_COV[i];
  *dr_ratio = DR_RATIO;
}
const double *ref_logfact(void) { return logfact; }

/* ---- primitives ---- */
double ref_bessi(int n, double x)                         { return bessi(n,x); }
double ref_logp_poisson(int k, int lambda)                { return logp_poisson((cnt_t)k,lambda); }
double ref_logp_skellam(int k, double lambda)             { return logp_skellam(k,lambda); }
double ref_logp_binom(int k, int n, double p)             { return logp_binom((cnt_t)k,(cnt_t)n,p); }
double ref_binom_test_g(int k, int n, double pe, int ex)  { return binom_test_g((cnt_t)k,(cnt_t)n,pe,ex); }
double ref_logp_trans(int b, int e, int cb, int ce, int cov) { return logp_trans(b,e,cb,ce,(cnt_t)cov); }
double ref_p_errorin(int e, double erate, int cout, int cin) { return p_errorin(e,erate,(cnt_t)cout,(cnt_t)cin); }
int    ref_plus_sigma(int cnt, int n)                     { return plus_sigma((cnt_t)cnt,n); }

/* ---- histogram: process_global_hist on <root>.hist (hist.c:28) ---- */
void ref_hist_covs(char *fk_root, int coverage, int *hcov, int *dcov)
{ process_global_hist(fk_root,coverage);
  *hcov = lambda_prior[0];
  *dcov = lambda_prior[1];
}

/* ---- FASTK profiles: Open_Profiles / Fetch_Profile (libfastk.c:1267,1414) ---- */
void *ref_open_profiles(char *root)                       { return Open_Profiles(root); }
void  ref_free_profiles(void *P)                          { Free_Profiles((Profile_Index *)P); }
int   ref_profiles_nreads(void *P)                        { return ((Profile_Index *)P)->nreads; }
int   ref_profiles_kmer(void *P)                          { return ((Profile_Index *)P)->kmer; }
int   ref_fetch_profile(void *P, long long id, int cap, unsigned short *out)
{ return Fetch_Profile((Profile_Index *)P,(int64)id,cap,out); }

/* ---- context.c; buffers laid out as the caller at ClassPro.c:136-142 does ---- */
void ref_seq_context(char *seq, int rlen, unsigned char *lctx_out, unsigned char *rctx_out)
{ Seq_Ctx *_lctx = Malloc((rlen+1)*sizeof(Seq_Ctx),"l");
  Seq_Ctx *rctx  = Malloc((rlen+1)*sizeof(Seq_Ctx),"r");
  memset(_lctx,0,(rlen+1)*sizeof(Seq_Ctx));
  memset(rctx,0,(rlen+1)*sizeof(Seq_Ctx));
  _lctx[0][HP] = 1;
  _lctx[0][DS] = _lctx[0][TS] = _lctx[1][TS] = 0;
  calc_seq_context(_lctx,rctx,seq,rlen);
  memcpy(lctx_out,_lctx,(size_t)rlen*3);
  memcpy(rctx_out,rctx,(size_t)rlen*3);
  free(_lctx); free(rctx);
}

/* ---- interval exchange record (same field set as oracle's cpo_intvl, 48 B) ---- */
typedef struct
  { int b, e;
    unsigned short cb, ce, ccb, cce;
    unsigned char is_rel;
    signed char asgn;
    unsigned char _pad[6];
    double pe, peo_b, peo_e;
  } xintvl;

static void x2i(const xintvl *x, Intvl *I)
{ memset(I,0,sizeof(Intvl));
  I->b = x->b; I->e = x->e; I->cb = x->cb; I->ce = x->ce; I->ccb = x->ccb; I->cce = x->cce;
  I->is_rel = x->is_rel; I->pe = x->pe; I->pe_o.b = x->peo_b; I->pe_o.e = x->peo_e; I->asgn = x->asgn;
}
static void i2x(const Intvl *I, xintvl *x)
{ x->b = I->b; x->e = I->e; x->cb = I->cb; x->ce = I->ce; x->ccb = I->ccb; x->cce = I->cce;
  x->is_rel = I->is_rel; x->pe = I->pe; x->peo_b = I->pe_o.b; x->peo_e = I->pe_o.e; x->asgn = I->asgn;
}

/* classify_rel (class_rel.c:871) + classify_unrel (class_unrel.c:248) on caller-supplied intervals.
 * stage: 1 = classify_rel only, 2 = classify_rel then classify_unrel. */
void ref_classify(xintvl *rx, int M, xintvl *ix, int N, int plen, int stage)
{ int cap = (M > N ? M : N)+8;
  Rel_Arg *arg   = alloc_rel_arg(cap);
  Intvl *rintvl  = Malloc(sizeof(Intvl)*cap,"r");
  Intvl *intvl   = Malloc(sizeof(Intvl)*cap,"i");
  for (int i = 0; i < M; i++) x2i(&rx[i],&rintvl[i]);
  for (int i = 0; i < N; i++) x2i(&ix[i],&intvl[i]);
  classify_rel(arg,rintvl,M,intvl,N,plen);
  if (stage >= 2)
    classify_unrel(intvl,N);
  for (int i = 0; i < M; i++) i2x(&rintvl[i],&rx[i]);
  for (int i = 0; i < N; i++) i2x(&intvl[i],&ix[i]);
  free_rel_arg(arg,cap);
  free(rintvl); free(intvl);
}

/* directional runs, to expose the fw / bw assignments separately (class_rel.c:623,737) */
void ref_classify_rel_dir(xintvl *rx, int M, int plen, int forward, signed char *asgn_out, double *hdrr)
{ int cap = M+8;
  Rel_Arg *arg  = alloc_rel_arg(cap);
  Intvl *rintvl = Malloc(sizeof(Intvl)*cap,"r");
  for (int i = 0; i < M; i++) x2i(&rx[i],&rintvl[i]);
  Iter_Rel r = forward ? classify_rel_fw(arg,rintvl,M,plen) : classify_rel_bw(arg,rintvl,M,plen);
  for (int i = 0; i < M; i++) asgn_out[i] = r.asgn[i];
  *hdrr = r.hdrr;
  free_rel_arg(arg,cap);
  free(rintvl);
}

/* ---- DAZZ_DB access through the reference's own DB.c: pins the test-side database writer
 *      (classpro_amd/dazz.py) and the track files the product writes ------------------------------ */
static DAZZ_DB  g_db;
static int      g_db_open = 0;
static char    *g_db_buf = NULL;

int ref_db_open(const char *path)
{ if (g_db_open) { Close_DB(&g_db); g_db_open = 0; }
  int st = Open_DB((char *)path,&g_db);
  if (st < 0) return -1;
  g_db_open = 1;
  g_db_buf = New_Read_Buffer(&g_db);
  return st;                                  /* 0 = .db, 1 = .dam */
}
int ref_db_nreads(void) { return g_db.nreads; }
int ref_db_maxlen(void) { return g_db.maxlen; }
int ref_db_read(int i, char *out, int *origin, int *fpulse, long long *coff)   /* Load_Read(db,i,buf,2) */
{ if (!g_db_open || i < 0 || i >= g_db.nreads) return -1;
  DAZZ_READ *r = g_db.reads+i;
  Load_Read(&g_db,i,g_db_buf,2);
  memcpy(out,g_db_buf,r->rlen);
  *origin = r->origin; *fpulse = r->fpulse; *coff = r->coff;
  return r->rlen;
}
/* Open_Track + Load_All_Track_Data: lengths per read into alen[nreads], concatenated data into data */
long long ref_db_track(const char *name, int *alen, unsigned char *data, long long cap)
{ if (!g_db_open) return -1;
  DAZZ_TRACK *t = Open_Track(&g_db,(char *)name);
  if (t == NULL) return -1;
  if (t->data == NULL)                        /* a mask-less header-only track opens with data == NULL */
    { Close_Track(&g_db,t); return 0; }
  Load_All_Track_Data(t);
  long long tot = 0;
  int64 *a = (int64 *)t->anno;
  for (int i = 0; i < t->nreads; i++)
    { alen[i] = t->alen[i];
      if (tot+t->alen[i] <= cap)
        memcpy(data+tot,(char *)t->data+a[i],t->alen[i]);
      tot += t->alen[i];
    }
  Close_Track(&g_db,t);
  return tot;
}
void ref_db_close(void) { if (g_db_open) { Close_DB(&g_db); g_db_open = 0; } }

/* ---- seed.c: find_seeds (seed.c:966-1032) for one read, with the buffers of ClassPro.c:120-134.
 *      `mintvl` is zeroed before the call: the reference searches and sorts one slot past the live part of this
 *      array (seed.c:141,161-166), i.e. it reads whatever an earlier read of the same thread left there; the
 *      defined behaviour of this build is "the array is all zeros at the start of every read" (within a read
 *      the three passes see each other's leftovers exactly as the reference code does).
 *      Outputs: sasgn[plen] ('E','H','D','R' per k-mer, seed.c:1007-1015), the repeat-mask intervals written to
 *      the .rep data track (int pairs, read coordinates, seed.c:531-566) and the canonical hashes. ---- */
int ref_find_seeds(const char *seq, const char *pasgn, const unsigned short *profile, int plen, int K,
                   int *sasgn, int *hash_out, int *rep_pairs, int rep_cap)
{ kdq_t(hmer_t) *Q = kdq_init(hmer_t);
  seg_t   *cprofile = Malloc((plen+1)*sizeof(seg_t),"c");
  int     *hash     = Malloc((plen+1)*sizeof(int),"h");
  intvl_t *mintvl   = Malloc((plen+2)*sizeof(intvl_t),"m");
  memset(mintvl,0,(plen+2)*sizeof(intvl_t));
  char *abuf = NULL, *dbuf = NULL; size_t alen = 0, dlen = 0;
  FILE *ranno = open_memstream(&abuf,&alen), *rdata = open_memstream(&dbuf,&dlen);
  int64 ridx = 0;
  find_seeds(Q,seq,pasgn,profile,cprofile,hash,sasgn,mintvl,plen,K,ranno,rdata,&ridx);
  fclose(ranno); fclose(rdata);
  int npair = (int)(dlen/(2*sizeof(int)));
  if (rep_pairs)
    memcpy(rep_pairs,dbuf,sizeof(int)*2*(npair < rep_cap ? npair : rep_cap));
  if (hash_out) memcpy(hash_out,hash,sizeof(int)*plen);
  free(abuf); free(dbuf);
  kdq_destroy(hmer_t,Q);
  free(cprofile); free(hash); free(mintvl);
  return npair;
}

/* =====================================================================================================
 *  wall.c (GSL-free part): find_wall (570-958) + find_rel_intvl (960-1051), the reference's own text.
 * ===================================================================================================== */
#ifdef REF_HAVE_WALL
#include <pthread.h>
#include <sys/wait.h>
#include <unistd.h>
#include <time.h>

int ref_have_wall(void) { return 1; }

static Error_Model g_emodel[N_CTYPE];
static int         g_emodel_set = 0;

/* What calc_init_thres (wall.c:167-243) leaves behind, filled from the caller's table instead:
 *   cthres = uint8 [3][21][256][2][2]  ([ctype][l][cout][thresT][etype], entries cout < cmax used),
 *   pe     = double [3][21], lmax[3], CMAX, HC_ERATE.   Layout of Error_Model: ClassPro.h:129-133, wall.c:120-147. */
void ref_wall_setup(const unsigned char *cthres, const double *pe, const int *lmax, int cmax, double hc_erate)
{ if (g_emodel_set)
    for (int t = 0; t < N_CTYPE; t++)
      { for (int l = 0; l <= g_emodel[t].lmax; l++)
          { for (int c = 0; c < 256; c++)
              { for (int s = 0; s < N_THRES; s++) free(g_emodel[t].cthres[l][c][s]);
                free(g_emodel[t].cthres[l][c]);
              }
            free(g_emodel[t].cthres[l]);
          }
        free(g_emodel[t].cthres); free(g_emodel[t].pe);
      }
  for (int t = 0; t < N_CTYPE; t++)
    { g_emodel[t].lmax = (uint8)lmax[t];
      g_emodel[t].pe = Malloc(sizeof(double)*(lmax[t]+1),"pe");
      g_emodel[t].cthres = Malloc(sizeof(uint8***)*(lmax[t]+1),"cthres");
      for (int l = 0; l <= lmax[t]; l++)
        { g_emodel[t].pe[l] = pe[t*21+l];
          g_emodel[t].cthres[l] = Malloc(sizeof(uint8**)*256,"cthres l");
          for (int c = 0; c < 256; c++)
            { g_emodel[t].cthres[l][c] = Malloc(sizeof(uint8*)*N_THRES,"cthres c");
              for (int s = 0; s < N_THRES; s++)
                { g_emodel[t].cthres[l][c][s] = Malloc(sizeof(uint8)*N_ETYPE,"cthres s");
                  for (int e = 0; e < N_ETYPE; e++)
                    g_emodel[t].cthres[l][c][s][e] = cthres[((((size_t)t*21+l)*256+c)*2+s)*2+e];
                }
            }
        }
    }
  CMAX = (uint8)cmax;
  HC_ERATE = hc_erate;
  g_emodel_set = 1;
}

/* Per-read scratch laid out as ClassPro.c:114-143; `fresh` = every buffer newly allocated and zeroed
 * (wall / perror index plen reset, Intvl slots zero, profile cells at and beyond plen zero, unwritten ctx cells zero):
 * the state the reference itself is in for the first read of a thread (SURVEY hazards 1, 2; DESIGN 3.3 hazard 8). */
typedef struct
  { int       rlen_max;
    Wall_Arg *warg;
    Rel_Arg  *rel_arg;
    Intvl    *intvl, *rintvl;
    cnt_t    *profile;
    Seq_Ctx  *_lctx, *rctx, *ctx[N_WTYPE];
    char     *rasgn;
  } ref_scratch;

#define REF_PROF_TAIL 256     /* correct_wall_cnt reads up to 126 cells beyond plen (hazard 8) */

static ref_scratch *scratch_new(int rlen_max, int K, int with_rel)
{ ref_scratch *S = Malloc(sizeof(ref_scratch),"scratch");
  S->rlen_max = rlen_max;
  S->warg    = alloc_wall_arg(rlen_max);                                   /* ClassPro.c:127 */
  S->rel_arg = with_rel ? alloc_rel_arg(rlen_max) : NULL;                  /* ClassPro.c:126 */
  S->intvl   = calloc(rlen_max,sizeof(Intvl));                             /* ClassPro.c:132-134 */
  S->rintvl  = calloc(rlen_max,sizeof(Intvl));
  S->profile = calloc((size_t)rlen_max+REF_PROF_TAIL,sizeof(cnt_t));
  S->_lctx   = calloc(rlen_max,sizeof(Seq_Ctx));                           /* ClassPro.c:136-142 */
  S->rctx    = calloc(rlen_max,sizeof(Seq_Ctx));
  S->_lctx[0][HP] = 1;
  S->_lctx[0][DS] = S->_lctx[0][TS] = S->_lctx[1][TS] = 0;
  S->ctx[DROP] = S->_lctx + (K-1) - 1;
  S->ctx[GAIN] = S->rctx;
  S->rasgn   = Malloc((size_t)rlen_max+1,"rasgn");                         /* ClassPro.c:115-118 */
  for (int i = 0; i < K-1; i++) S->rasgn[i] = 'N';
  memset(S->warg->wall,0,(size_t)rlen_max+1);
  for (int i = 0; i <= rlen_max; i++)
    for (int e = 0; e < N_ETYPE; e++)
      for (int w = 0; w < N_WTYPE; w++)
        S->warg->perror[i][e][w] = -INFINITY;
  return S;
}
static void scratch_free(ref_scratch *S)
{ free_wall_arg(S->warg);
  if (S->rel_arg) free_rel_arg(S->rel_arg,S->rlen_max);
  free(S->intvl); free(S->rintvl); free(S->profile); free(S->_lctx); free(S->rctx); free(S->rasgn); free(S);
}

/* The three per-read resets that make a read's result independent of the reads a thread saw before it
 * (the reference resets none of them; its result then depends on -T and on the read order). */
static inline void scratch_define(ref_scratch *S, int rlen, int plen, int prev_plen)
{ S->warg->wall[plen] = 0;                                                 /* hazard 1 */
  for (int e = 0; e < N_ETYPE; e++)
    for (int w = 0; w < N_WTYPE; w++)
      S->warg->perror[plen][e][w] = -INFINITY;
  int top = (prev_plen > plen ? prev_plen : plen);
  for (int i = 0; i < top; i++)                                            /* hazard 2: position-indexed slots */
    S->intvl[i].ccb = S->intvl[i].cce = 0;
  memset(S->profile+plen,0,sizeof(cnt_t)*REF_PROF_TAIL);                   /* hazard 8 */
  (void)rlen;
}

static int run_wall_rel(ref_scratch *S, const char *seq, int rlen, const cnt_t *prof, int K, int *M)
{ int plen = rlen-(K-1);
  calc_seq_context(S->_lctx,S->rctx,(char *)seq,rlen);                     /* ClassPro.c:230 */
  memcpy(S->profile,prof,sizeof(cnt_t)*plen);                              /* stands for Fetch_Profile, :233 */
  int N = find_wall(S->warg,S->intvl,S->profile,plen,S->ctx,g_emodel,K);   /* ClassPro.c:240 */
  *M = find_rel_intvl(S->intvl,N,S->rintvl,S->profile,S->ctx,K);           /* ClassPro.c:246 */
  return N;
}

/* One read, fresh buffers: intervals after find_wall + find_rel_intvl (iv[N], is_rel / ccb / cce set) and the
 * reliable copies (rv[M]).
 * Returns N, or -2 if the caller's arrays are too small.  A read on which the reference's `#define DEBUG`
 * abort fires ("# E-intvls >= plen", wall.c:783-788, 803-808, 827-832, 847-852, 900-905) ends the PROCESS:
 * use ref_find_wall_exit_status for those. */
int ref_find_wall_rel(const char *seq, int rlen, const unsigned short *prof, int K,
                      xintvl *iv, int cap, int *M_out, xintvl *rv)
{ if (!g_emodel_set || rlen < K) return -1;
  ref_scratch *S = scratch_new(rlen+1,K,0);
  int M, N = run_wall_rel(S,seq,rlen,prof,K,&M);
  if (N > cap) { scratch_free(S); return -2; }
  for (int i = 0; i < N; i++) i2x(&S->intvl[i],&iv[i]);
  for (int i = 0; i < M; i++) i2x(&S->rintvl[i],&rv[i]);
  *M_out = M;
  scratch_free(S);
  return N;
}

/* The same call in a child process: returns the child's exit status (0 = find_wall returned, 1 = the reference's
 * own exit(1)), or -1 if it died otherwise.  stderr of the child goes to /dev/null. */
int ref_find_wall_exit_status(const char *seq, int rlen, const unsigned short *prof, int K)
{ if (!g_emodel_set || rlen < K) return -1;
  fflush(NULL);
  pid_t pid = fork();
  if (pid < 0) return -1;
  if (pid == 0)
    { FILE *f = freopen("/dev/null","w",stderr); (void)f;
      ref_scratch *S = scratch_new(rlen+1,K,0);
      int M; run_wall_rel(S,seq,rlen,prof,K,&M);
      _exit(0);
    }
  int st = 0;
  if (waitpid(pid,&st,0) < 0 || !WIFEXITED(st)) return -1;
  return WEXITSTATUS(st);
}

/* The whole loop body for one read on scratch S (ClassPro.c:229-271): labels[rlen]. */
static void run_read(ref_scratch *S, const char *seq, int rlen, const cnt_t *prof, int K, char *labels)
{ int Km1 = K-1;
  if (rlen <= Km1)                                                         /* ClassPro.c:209-226 */
    { memset(labels,'N',rlen); return; }
  int plen = rlen-Km1, M;
  int N = run_wall_rel(S,seq,rlen,prof,K,&M);
  classify_rel(S->rel_arg,S->rintvl,M,S->intvl,N,plen);                    /* ClassPro.c:261 */
  classify_unrel(S->intvl,N);                                              /* ClassPro.c:262 */
  char *pasgn = S->rasgn+Km1;
  for (int i = 0; i < N; i++)                                              /* ClassPro.c:263-269 */
    { Intvl I = S->intvl[i];
      char c = stoc[(int)I.asgn];
      for (pos_t j = I.b; j < I.e; j++)
        pasgn[j] = c;
    }
  memcpy(labels,S->rasgn,rlen);
}

/* One read through the whole per-read path on fresh buffers -> label string (reference text only:
 * context.c -> wall.c slice -> class_rel.c -> class_unrel.c -> paint).  Optionally the final interval records. */
int ref_classify_read(const char *seq, int rlen, const unsigned short *prof, int K, char *labels,
                      xintvl *iv, int cap)
{ if (!g_emodel_set) return -1;
  ref_scratch *S = scratch_new((rlen > K ? rlen : K)+1,K,1);
  run_read(S,seq,rlen,prof,K,labels);
  int N = 0;
  if (rlen >= K && iv)
    { /* N is not kept by run_read: recount from the tiling of [0,plen) */
      int plen = rlen-(K-1), e = 0;
      while (e < plen && N < cap) { i2x(&S->intvl[N],&iv[N]); e = S->intvl[N].e; N++; }
    }
  scratch_free(S);
  return N;
}

/* The reference's thread loop (kmer_class_thread, ClassPro.c:34-335) without its I/O: nthreads pthreads over
 * contiguous read ranges split by read count as ClassPro.c:530 / io.c:315-331 do, per thread ONE set of scratch sized by
 * rlen_max (ClassPro.c:110: MAX_READ_LEN for FASTX; 0 selects it) and reused across reads.
 * defined != 0: the three resets of scratch_define before every read (result = a function of the read alone).
 * seconds[0] = allocation phase (max over threads; alloc_rel_arg dominates, SURVEY hazard 7),
 * seconds[1] = classification phase (wall clock from the moment every thread has its scratch).
 * Reads on which the reference aborts end the process, as in the reference. */
typedef struct
  { const char *seq; const long long *seq_off; const cnt_t *prof; const long long *prof_off;
    int beg, end, K, rlen_max, defined; char *labels;
    pthread_barrier_t *bar; double t_alloc;
  } ref_job;

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC,&ts); return ts.tv_sec+1e-9*ts.tv_nsec; }

static void *ref_thread(void *arg)
{ ref_job *J = arg;
  double t0 = now_s();
  ref_scratch *S = scratch_new(J->rlen_max,J->K,1);
  J->t_alloc = now_s()-t0;
  pthread_barrier_wait(J->bar);
  int prev_plen = 0;
  char *buf = Malloc((size_t)J->rlen_max+1,"seq");
  for (int id = J->beg; id < J->end; id++)
    { int rlen = (int)(J->seq_off[id+1]-J->seq_off[id]);
      int plen = rlen-(J->K-1);
      memcpy(buf,J->seq+J->seq_off[id],rlen); buf[rlen] = '\0';
      if (J->defined && plen > 0)
        { scratch_define(S,rlen,plen,prev_plen); prev_plen = plen; }
      run_read(S,buf,rlen,J->prof+J->prof_off[id],J->K,J->labels+J->seq_off[id]);
    }
  pthread_barrier_wait(J->bar);
  free(buf);
  scratch_free(S);
  return NULL;
}

int ref_classify_batch(const char *seq, const long long *seq_off, const unsigned short *prof,
                       const long long *prof_off, int nreads, int K, char *labels, int nthreads,
                       int rlen_max, int defined, double *seconds)
{ if (!g_emodel_set) return -1;
  if (rlen_max <= 0) rlen_max = MAX_READ_LEN;
  for (int i = 0; i < nreads; i++)
    if (seq_off[i+1]-seq_off[i] > rlen_max) return -2;               /* ClassPro.c:184: rlen > MAX_READ_LEN is the reference's error */
  if (nthreads < 1) nthreads = 1;
  if (nthreads > nreads && nreads > 0) nthreads = nreads;
  pthread_t *th = Malloc(sizeof(pthread_t)*nthreads,"th");
  ref_job *J = Malloc(sizeof(ref_job)*nthreads,"jobs");
  pthread_barrier_t bar;
  pthread_barrier_init(&bar,NULL,nthreads+1);
  int nparts = (nreads/nthreads)+(nreads%nthreads == 0 ? 0 : 1);           /* ClassPro.c:530; io.c prepare_param */
  double t0 = now_s();
  for (int t = 0; t < nthreads; t++)
    { int beg = t*nparts, end = (t+1)*nparts;
      if (beg > nreads) beg = nreads;
      if (end > nreads) end = nreads;
      J[t] = (ref_job){ seq,seq_off,prof,prof_off,beg,end,K,rlen_max,defined,labels,&bar,0. };
      pthread_create(&th[t],NULL,ref_thread,&J[t]);
    }
  pthread_barrier_wait(&bar);
  double t1 = now_s();
  pthread_barrier_wait(&bar);
  double t2 = now_s();
  for (int t = 0; t < nthreads; t++) pthread_join(th[t],NULL);
  if (seconds) { seconds[0] = t1-t0; seconds[1] = t2-t1; }
  pthread_barrier_destroy(&bar);
  free(th); free(J);
  return 0;
}
#else
int ref_have_wall(void) { return 0; }
#endif

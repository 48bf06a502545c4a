/*
 * classpro_amd.h -- C ABI of the MI355X-native per-read k-mer classifier (libclasspro_amd.so).
 *
 * Drop-in boundary for ClassPro's per-read hot path.  The reference has no FFI; what a maintainer
 * would bind is (i) the one-time global setup and (ii) the six per-read calls of the thread loop
 * (src/ClassPro.c:229-271).  Each entry point below names the reference interface it replaces.
 * The per-read calls are replaced by *batched* calls over many reads laid out flat in HBM:
 *
 *     seq      char   [seq_off[nreads]]   read bases, ASCII, concatenated, no terminators
 *     seq_off  int64  [nreads+1]          read r = seq[seq_off[r] .. seq_off[r+1])
 *     prof     uint16 [prof_off[nreads]]  k-mer counts (what Fetch_Profile yields), concatenated;
 *                                         base address 16-byte aligned
 *     prof_off int64  [nreads+1]          plen_r = prof_off[r+1]-prof_off[r] = rlen_r-(K-1)
 *     labels   char   [seq_off[nreads]]   out: 'N'*(K-1) then E/H/D/R per k-mer (ClassPro.c:116-119,265-271)
 *
 * All reads of a batch must have rlen >= K (the caller prints shorter reads itself, as
 * ClassPro.c:209-226 does).  CP_MAX_READ_LEN is the reference's limit for FASTX inputs (ClassPro.c:184-187: the
 * command line enforces it there); the library itself takes longer reads (a Dazzler database is sized by its
 * longest read, ClassPro.c:87,110): reads beyond 65535 k-mers go through the sequential classify kernels.
 *
 * Pointers named d_* are DEVICE pointers (HBM); everything else is host memory.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No torch types appear in this ABI.
 * Every function returns CP_OK (0) or a negative CP_E* code; cp_last_error() gives the message.
 * The reference's behaviour on these errors is fprintf(stderr)+exit(1); the CLI mirrors that.
 */
#ifndef CLASSPRO_AMD_H
#define CLASSPRO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CP_MAX_KMER_CNT 32767          /* src/const.c:38  MAX_KMER_CNT */
#define CP_MAX_READ_LEN 60000          /* src/const.c:55  MAX_READ_LEN (FASTX inputs) */

enum { CP_OK = 0, CP_EINVAL = -1, CP_ENOPEAK = -2, CP_ERCOV = -3, CP_EHIP = -4, CP_EOVERFLOW = -5, CP_ENOMEM = -6 };

/* State codes (src/ClassPro.h:57) and their characters (src/const.c:19). */
enum { CP_ERROR = 0, CP_REPEAT = 1, CP_HAPLO = 2, CP_DIPLO = 3, CP_N_STATE = 4 };

/* Interval record exchanged by the stage entry points: the fields of the reference's `Intvl`
 * (src/ClassPro.h:159-170) in a fixed 48-byte layout. */
typedef struct
  { int32_t  b, e;                 /* [b,e) in profile coordinates */
    uint16_t cb, ce;               /* counts at b and e-1 */
    uint16_t ccb, cce;             /* error-corrected boundary counts (find_rel_intvl) */
    uint8_t  is_rel;
    int8_t   asgn;                 /* CP_ERROR..CP_DIPLO, CP_N_STATE = unclassified */
    uint8_t  _pad[6];
    double   pe;                   /* log P(interval is a sequencing error in this read) or -inf */
    double   peo_b, peo_e;         /* log P(boundary explained by errors in other reads) or -inf */
  } cp_intvl;

const char *cp_last_error(void);
const char *cp_version(void);

/* ------------------------------------------------------------------------------------------
 * One-time global setup (host).
 * ------------------------------------------------------------------------------------------ */

/* Replaces process_global_hist (src/hist.c:28-105) on a loaded FASTK histogram
 * (Load_Histogram/Modify_Histogram, src/libfastk.c:51-147).  `hist` is the on-disk array
 * hist[0..high-low] of <root>.hist (unique counts); coverage_opt is `-c` (0 = estimate).
 * CP_ENOPEAK when no peak count >= 10 exists (the reference exits, hist.c:66-69). */
int cp_hist_covs(const int64_t *hist, int low, int high, int64_t ilowcnt, int64_t ihighcnt,
                 int coverage_opt, int *hcov, int *dcov);

/* Replaces precompute_logfact (src/prob.c:14-19), the GLOBAL_COV / DR_RATIO block
 * (src/ClassPro.c:544-548) and calc_init_thres(NULL) (src/wall.c:167-244): builds the read-only
 * tables on the host and uploads them to the current HIP device.  It also has the device fill a table of
 * logp_trans values (util.c:35-44: a function of |ce-cb| and the integer cov*|e-b| alone; 1 GB of device memory by
 * default, environment CLASSPRO_SKELLAM_TABLE_MB, 0 = no such table; and a second table of the same size with their
 * exponentials, which is what classify_rel's DP step uses of a transition -- CLASSPRO_EXP_TABLE=0: without it) and two small ones (classify_unrel's
 * binomial-test logs, the walk's P(error in): 74 MB) with the code the kernels otherwise run on the spot, so results
 * are the same bits with or without them (CLASSPRO_TABLES=0: none of the three).  The tables depend on READ_LEN / the
 * error model only, so all cp_params of a process that agree on those share one reference-counted copy per device.
 * A table that finds no device memory is left out (slower, same results); cp_params_tables tells which are in use.
 * CP_ERCOV when the repeat threshold exceeds 255 (wall.c:174-177). */
typedef struct cp_params cp_params;
int  cp_params_create(int K, int read_len, int hcov, int dcov, cp_params **out);

/* -M<model_path> (ClassPro.c:451-453, load_himodel wall.c:55-115): as cp_params_create, with the
 * low-complexity error rates pe[t][l] fitted from a HIsim error-model file instead of the default
 * 0.002 l^2 + 0.002.  model_path == NULL is the default model.  The quadratic fit the reference does
 * with GSL is solved in closed form here (no GSL).  cp_load_error_model returns just the fitted table
 * (pe63 = double[3][21], rows HP/DS/TS). */
int  cp_params_create_model(int K, int read_len, int hcov, int dcov, const char *model_path, cp_params **out);
int  cp_load_error_model(const char *model_path, double *pe63);
/* The error model handed in as a table (pe63 = double[3][21], rows HP / DS / TS; entries l = 1 .. 20/(t+1) are used and
 * must lie in (0,1)): for a caller that has the rates already -- e.g. the reference's own load_himodel (wall.c:55-115) with
 * its GSL fit, when bit-identity with THAT fit is wanted -- or from cp_load_error_model.  find_wall (wall.c:570) takes the
 * Error_Model as a parameter in the reference too. */
int  cp_params_create_pe(int K, int read_len, int hcov, int dcov, const double *pe63, cp_params **out);
void cp_params_destroy(cp_params *p);
/* Device bytes of the look-up tables this cp_params uses (0 = that table is not in use: its values are
 * computed on the spot).  skel_bytes counts the logp_trans table AND, when present, the table of its exponentials
 * (same shape: CLASSPRO_SKELLAM_TABLE_MB costs twice its value unless CLASSPRO_EXP_TABLE=0). */
int  cp_params_tables(const cp_params *p, size_t *skel_bytes, size_t *uerr_bytes, size_t *petab_bytes);
/* The device's scalar numerics, for inspection/tests: y[i] = f(x[i]) computed ON THE DEVICE by the functions the kernels
 * call -- fn 0: exp, 1: log (csrc/cp_libm.h: glibc 2.35's routines, the libm the reference's prob.c / class_rel.c /
 * class_unrel.c / wall.c results come from; bit-identical to the host's exp()/log() on an x86-64 host with FMA),
 * 2: sqrt, 3: bessi(n = (int)x2[i], x[i]) (bessel.c:478-521), 4: logp_skellam(k = (int)x2[i], lambda = x[i])
 * (prob.c:41-44).  d_x2 may be null for fn 0-2. */
int  cp_math_eval(int fn, const double *d_x, const double *d_x2, double *d_y, int64_t n, void *stream);
/* Host copies of the tables, for inspection/tests: cov[4]=GLOBAL_COV[E,R,H,D]; cthres is
 * [3][21][256][2][2] = [ctype][l][cout][INIT|FINAL][SELF|OTHERS]; pe is [3][21]; logfact[32768]. */
int  cp_params_export(const cp_params *p, int *cov4, double *dr_ratio, int *cmax, double *hc_erate,
                      uint8_t *cthres, double *pe, double *logfact);

/* Replaces the decoder of Fetch_Profile (src/libfastk.c:1467-1534) for one read's code string
 * (host; the north star keeps FASTK decoding on the host).  Returns the profile length (may
 * exceed `cap`, in which case only `cap` counts were written), or a negative CP_E* code. */
int cp_decode_profile(const uint8_t *code, int64_t len, uint16_t *profile, int cap);

/* Inverse of cp_decode_profile: the FASTK code string of one read's counts (what FastK writes;
 * tooling for tests / synthetic inputs).  `code` needs 2*n+2 bytes; returns the code length. */
int64_t cp_encode_profile(const uint16_t *profile, int n, uint8_t *code, int64_t cap);

/* ------------------------------------------------------------------------------------------
 * Batched device path.
 * ------------------------------------------------------------------------------------------ */
/* Streams.  A call that takes a `stream` does all of its device work -- kernels, fills, copies, its scratch from the
 * stream-ordered pool -- in that stream's order and on no other stream: it may be given inputs that earlier work on the same
 * stream has not written yet, and NULL is the null stream, nothing special.  "Asynchronous on `stream`" means the call
 * returns without waiting; a call that reads something back waits for `stream` alone.  An object that is written in a
 * stream's order (a cp_workspace, a cp_kmer_table, a cp_kmer_counts, a cp_acc) remembers the stream of the last call that
 * queued work on it, and a call WITHOUT a stream argument that reads device state waits for that stream -- not for the
 * device, not for the caller's current stream -- and runs what it launches there; it may be made from any host thread or
 * under any current stream once the call that queued the work has returned.  Two calls that queue work on ONE object on
 * two DIFFERENT streams are the caller's to order (an event, or a call of this kind in between); cp_kmer_counts_sort and
 * cp_kmer_table_sort are the exception and wait for the table's stream themselves.  A cp_kmer_sorted, a cp_unitigs and a
 * cp_unitig_graph are complete when the call that made them returns (each such call waits for its stream last), are only
 * read afterwards, and so may be used on any stream at once.  tests/test_gpu_streams.py holds every call family to this on
 * a side stream whose inputs arrive late. */
typedef struct cp_workspace cp_workspace;          /* device scratch, grown on demand, reusable */
int  cp_workspace_create(cp_workspace **out);
void cp_workspace_destroy(cp_workspace *ws);
size_t cp_workspace_bytes(const cp_workspace *ws); /* device bytes currently held */

/* Whole hot path for a batch: replaces the body of the read loop, ClassPro.c:229-271
 * (calc_seq_context, find_wall, find_rel_intvl, classify_rel, classify_unrel, label paint).
 * Asynchronous on `stream` except for one small D2H size read-back after the scan stage.
 * A read's labels are a function of that read alone (its bases, its counts, the parameters): they do not depend on
 * the batch it travels in, its place in it, or what lies before or after its counts in memory.  (The reference reads
 * profile[plen] in correct_wall_cnt, wall.c:976-978, when a low-complexity run reaches the end of the read; that
 * cell is defined as 0 here.)
 * Limit: a batch holds at most CP_MAX_BATCH_KMERS k-mer positions (its scratch capacities, up to 16 per position,
 * are summed in 40 bits); a larger one is refused with CP_EINVAL -- split it. */
#define CP_MAX_BATCH_KMERS ((int64_t)1 << 35)
int cp_classify_batch(const cp_params *p, cp_workspace *ws,
                      const char *d_seq, const int64_t *d_seq_off,
                      const uint16_t *d_prof, const int64_t *d_prof_off,
                      int nreads, int64_t total_bases, int64_t total_kmers,
                      char *d_labels, void *stream);

/* Fetch_Profile's decoder on the device: d_codes holds the concatenated code
 * strings of the batch (read r = d_codes[d_code_off[r] .. d_code_off[r+1])), d_prof receives the
 * counts at d_prof_off (plen_r = rlen_r-(K-1), known from the read lengths).  Bit-exact with
 * cp_decode_profile for every code whose counts stay in [0,32767] (FastK caps counts there).  A code
 * that does not expand to exactly plen_r counts (the reference's "rlen != plen+Km1" abort,
 * ClassPro.c:234-237), ends inside a 2-byte token or steps out of [0,32767] is reported as CP_EINVAL by the
 * next cp_workspace_check; d_prof is then unspecified. */
int cp_decode_profiles(cp_workspace *ws, const uint8_t *d_codes, const int64_t *d_code_off,
                       const int64_t *d_prof_off, int nreads, uint16_t *d_prof, void *stream);

/* Dazzler 2-bit bases on the device (Load_Read(db,i,buf,2), DB.c:1232-1298 with Uncompress_Read / Upper_Read,
 * DB.c:342-381): read r's COMPRESSED_LEN(rlen_r) = (rlen_r+3)/4 bytes start at d_packed[d_pack_off[r]] (the bytes
 * of the .bps file at DAZZ_READ.boff), 4 bases per byte, first base in the top two bits; d_seq receives
 * 'A' 'C' 'G' 'T' at d_seq_off[r].  A database input then crosses PCIe at 0.25 B/base. */
int  cp_unpack_bases(const uint8_t *d_packed, const int64_t *d_pack_off, const int64_t *d_seq_off,
                     int nreads, char *d_seq, void *stream);

/* 2-bit payloads across PCIe for FASTX inputs too.  Bases: cp_pack_bases (host) packs one read in
 * the layout cp_unpack_bases expands, when it holds upper-case A, C, G, T only (returns 1; 0 = another letter: send the
 * batch as characters -- calc_seq_context compares raw characters, context.c:8-108).  Labels: cp_pack_labels (device)
 * turns the label string of every read into 2-bit codes, four per byte, first label in the top bits: ctos (const.c:21-36:
 * N, E -> 0, R -> 1, H -> 2, D -> 3) + Compress_Read (gene_core.c:235-254), i.e. exactly the read's payload of the
 * .class.data track (ClassPro.c:291-300); read r's (rlen_r+3)/4 bytes start at d_packed[d_pack_off[r]] (the offsets of
 * cp_unpack_bases).  cp_unpack_labels (host) is the inverse for one read: K-1 'N', then E/R/H/D (stoc, const.c:19).
 * A batch then crosses PCIe at about 0.52 B/base in (bases + FASTK codes) and 0.25 B/base out instead of 1.27 and 1. */
int cp_pack_bases(const char *seq, int rlen, uint8_t *packed);
/* cp_pack_bases for every read of a host batch on `nthreads` host threads: read r's (rlen_r+3)/4 bytes go to
 * packed[pack_off[r]]; 1 = every read packed, 0 = a read holds another letter (send the batch as characters). */
int cp_pack_bases_batch(const char *seq, const int64_t *seq_off, int nreads, uint8_t *packed, const int64_t *pack_off,
                        int nthreads);
int cp_pack_labels(const char *d_labels, const int64_t *d_seq_off, const int64_t *d_pack_off, int nreads,
                   uint8_t *d_packed, void *stream);
int cp_unpack_labels(const uint8_t *packed, int rlen, int K, char *labels);

/* Labels as RUNS, the smallest form in which a batch's result crosses PCIe (~0.05 B/base): the label string of a read
 * (ClassPro.c:265-271: K-1 'N', then the class of every interval over its k-mers) is K-1 'N' followed by runs; run j
 * covers label positions [ends[j-1], ends[j]) (ends[-1] = K-1) with the character cls[j] (stoc, const.c:19).  After
 * cp_classify_batch -- or cp_run_stages(..., CP_STAGE_CLASS_ALL, ...), which skips painting the 1 B/base label string
 * altogether -- cp_label_runs writes the runs of read r at index d_cap_off[r] .. d_cap_off[r]+d_nruns[r] of d_ends /
 * d_cls; the arrays take cp_label_runs_capacity(ws) entries (a loose bound: the interval capacity of the batch, about
 * 0.01 per base), d_nruns nreads, d_cap_off nreads+1 entries.  cp_expand_label_runs (host) rebuilds one read's string. */
int64_t cp_label_runs_capacity(const cp_workspace *ws);
int cp_label_runs(const cp_params *p, cp_workspace *ws, int32_t *d_ends, uint8_t *d_cls, int32_t *d_nruns, int64_t *d_cap_off,
                  void *stream);
int cp_expand_label_runs(const int32_t *ends, const uint8_t *cls, int nruns, int rlen, int K, char *labels);

/* -s: replaces find_seeds (src/seed.c:966-1032; call site ClassPro.c:281-282) for every read of a batch that
 * cp_classify_batch has labelled.  d_labels is that call's output; d_seeds[total_bases] receives, in the same layout,
 * 'N' for the first K-1 bases of a read and per k-mer 'E' (no seed) or the class of the seed, 'H' / 'D' / 'R' (a seed
 * inside a repetitive stretch) -- the values the .class.data track carries under -s (ClassPro.c:293).  The repeat-mask
 * intervals of anno_repeat (seed.c:482-566, the .rep.data track) stay in `ws`: cp_get_rep_masks copies, per read, their
 * number and the (b,e) pairs in read coordinates (read r's pairs start at pairs[2*cap_off[r]]; cp_rep_masks_capacity
 * gives the pairs' total capacity).  Defined behaviour: the reference's masked-interval array starts as zeros at
 * every read (it is read one slot past its live part, seed.c:141,161-166). */
int cp_find_seeds_batch(const cp_params *p, cp_workspace *ws,
                        const char *d_seq, const int64_t *d_seq_off,
                        const uint16_t *d_prof, const int64_t *d_prof_off, const char *d_labels,
                        int nreads, int64_t total_bases, int64_t total_kmers,
                        char *d_seeds, void *stream);
/* cp_get_rep_masks waits for the stream of the last call on `ws` (cp_workspace_check) before it copies;
 * cp_rep_masks_capacity returns a number the host already holds when cp_find_seeds_batch returns. */
int cp_get_rep_masks(cp_workspace *ws, int32_t *count, int64_t *cap_off, int32_t *pairs, int64_t capacity);
int64_t cp_rep_masks_capacity(const cp_workspace *ws);

/* Waits for the stream of the last call that queued work on `ws` and returns CP_EOVERFLOW if, in ANY call on `ws` since the previous check, a read
 * needed more E-interval / interval / seed scratch than its capacity (the reference aborts likewise: "# E-intvls >=
 * plen", src/wall.c:783-788), CP_EINVAL for a bad code string in cp_decode_profiles.  The device-side flags are sticky
 * and are cleared by this call only.  Call after cp_classify_batch before trusting the labels. */
int cp_workspace_check(cp_workspace *ws);

/* Stage entry points (the reference's per-read internal contract, batched).  They run the
 * pipeline up to and including the named stage and keep the results in `ws`:
 *   CP_STAGE_SCAN      candidate scan of find_wall (wall.c:590-607): bitmap of wall candidates
 *   CP_STAGE_WALL      find_wall       (src/wall.c:570-958)
 *   CP_STAGE_REL       find_rel_intvl  (src/wall.c:1016-1051)
 *   CP_STAGE_CLASS_REL classify_rel    (src/class_rel.c:871-963)
 *   CP_STAGE_CLASS_ALL classify_unrel  (src/class_unrel.c:248-300)
 *   CP_STAGE_LABELS    label paint     (src/ClassPro.c:265-271)   == cp_classify_batch */
enum { CP_STAGE_SCAN = 1, CP_STAGE_WALL = 2, CP_STAGE_REL = 3, CP_STAGE_CLASS_REL = 4,
       CP_STAGE_CLASS_ALL = 5, CP_STAGE_LABELS = 6 };
int cp_run_stages(const cp_params *p, cp_workspace *ws,
                  const char *d_seq, const int64_t *d_seq_off,
                  const uint16_t *d_prof, const int64_t *d_prof_off,
                  int nreads, int64_t total_bases, int64_t total_kmers,
                  char *d_labels, int last_stage, void *stream);

/* Read-back of stage results of the last cp_run_stages/cp_classify_batch on `ws` (host buffers; each waits for the
 * stream of that call, through cp_workspace_check or directly, before it copies).  counts: n_intvl[nreads], n_rel[nreads]; offsets into the flat arrays
 * are the exclusive prefix sums of the per-read capacities returned in cap_off[nreads+1].
 * After a whole-path call (cp_classify_batch = CP_STAGE_LABELS) the interval records come back complete (the final classes
 * included), but the copies of the reliable intervals and the forward / backward assignments do not exist -- that path
 * hands classify_rel 24-byte records and the label paint 4-byte (end, class) words instead: `rintvl`
 * is returned zeroed.  Stop at CP_STAGE_REL .. CP_STAGE_CLASS_ALL for them.  (CLASSPRO_COMPACT_REL=0: the full records
 * on every call.) */
int cp_get_counts(cp_workspace *ws, int32_t *n_cand, int32_t *n_intvl, int32_t *n_rel, int64_t *cap_off);
int cp_get_intervals(cp_workspace *ws, cp_intvl *intvl, cp_intvl *rintvl, int64_t capacity);
int cp_get_rel_asgn(cp_workspace *ws, int8_t *fw, int8_t *bw, int64_t capacity);   /* after a run that stopped at CP_STAGE_CLASS_REL or CP_STAGE_CLASS_ALL */
int cp_get_bitmap(cp_workspace *ws, uint64_t *words, int64_t nwords);

/* calc_seq_context (src/context.c:8-108), batched and dense: d_lctx/d_rctx are [total_bases][3]
 * uint8 indexed by read position (the `_lctx`/`rctx` buffers of ClassPro.c:136-142).  The hot path
 * evaluates contexts on demand and never materialises these arrays; this entry point exists for
 * the reference's own call and for parity tests. */
int cp_seq_context(const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases,
                   uint8_t *d_lctx, uint8_t *d_rctx, void *stream);

/* Profile-scan kernel alone (the HBM-roofline kernel): d_bitmap holds ceil(total_kmers/64)+1 words. */
int cp_scan_candidates(const cp_params *p, const uint16_t *d_prof, int64_t total_kmers,
                       uint64_t *d_bitmap, void *stream);

/* ------------------------------------------------------------------------------------------
 * Per-k-mer label table (class2cns): how often each distinct k-mer got each label across all the reads that hold
 * it.  Replaces the reference's text pipeline scripts/naive_consensus.sh (src/class2cns.c:62-68, then
 * `sort | uniq -c`, then scripts/agg2cons.py) with a hashed count on the device.
 *
 *   Input        reads and labels in the flat layout above, as cp_classify_batch leaves them: K-1 'N', then one of
 *                E/H/D/R per k-mer.  Reads shorter than K contribute nothing.
 *   Occurrences  the k-mer ending at read position i, for i in [K-1, rlen) (class2cns.c:63).
 *   Skipped      a k-mer holding a base other than upper-case A C G T is not counted, only tallied in n_skipped.
 *                (Difference from the reference: its text pipeline keeps such a k-mer as a string of its own.)
 *   Bad label    a label other than E/H/D/R at a counted position is an error, CP_EINVAL, reported by the next
 *                cp_kmer_table_stats (deferred, as cp_workspace_check does for the classifier).
 *   Key          2 bits per base, A=0 C=1 G=2 T=3, first base most significant, so numeric key order is LC_ALL=C
 *                text order.  2 <= K <= 63 (a key holds 2K <= 126 bits); any other K is CP_EINVAL.  Exported as
 *                hi = key bits 125..63, lo = key bits 62..0.
 *   Forward      (canonical = 0) the key is the k-mer as read: the reference pipeline's semantics.
 *   Canonical    (canonical = 1) the key is min(forward, reverse complement): a k-mer and its reverse complement
 *                share one entry (as FASTK counts k-mers).
 *   Counts       four exact u32 per distinct key, in label order E, H, D, R.  A count that would pass 2^32-1 makes
 *                every later cp_kmer_table_stats return CP_EOVERFLOW: a wrapped count is never reported.
 *   Consensus    the label with the largest count; a tie goes to the label of larger copy number, R > D > H > E
 *                (a project choice: the reference defines none).
 *   Consistency  n_distinct / S with S = sum over distinct keys of total/max (each term in [1, 4]): the harmonic
 *                mean of agg2cons.py's most-common fraction mcf = max/total.  Each term is accumulated as
 *                floor(total * 2^64 / max) in 128-bit fixed point (s_fixed_hi:s_fixed_lo) and `consistency` is the
 *                correctly rounded double of n_distinct * 2^64 / S_fixed, so it is the same bit for bit whatever the
 *                batching, read order or thread schedule (NaN when the table is empty).
 *
 * The table sizes itself: inserts that run past the probe bound are replayed after the table grows (rehash into at
 * least twice the slots), and it also grows when more than half of its slots are occupied.  Nothing is dropped.
 * initial_slots (0 = default) exists so that tests can force growth.  A growth step that cannot allocate returns
 * CP_ENOMEM and leaves the table as it was.  One GPU per table.
 */
typedef struct cp_kmer_table cp_kmer_table;
typedef struct
  { int64_t  n_kmers;              /* counted occurrences (= sum of label_total) */
    int64_t  n_skipped;            /* occurrences skipped: a base other than upper-case A C G T */
    int64_t  n_distinct;           /* distinct keys */
    int64_t  n_unanimous;          /* distinct keys whose occurrences all carry one label (mcf == 1) */
    int64_t  label_total[4];       /* occurrences per input label, order E, H, D, R */
    int64_t  cns_total[4];         /* occurrences per consensus label of their key, order E, H, D, R */
    uint64_t s_fixed_hi, s_fixed_lo;   /* S in 64.64 fixed point (see Consistency) */
    double   consistency;
    int64_t  slots, bytes;         /* table slots now; device bytes held (slots of 32 bytes + failure bitmaps) */
    int64_t  growths;              /* growth steps so far */
  } cp_kmer_stats;
int  cp_kmer_table_create(int K, int canonical, int64_t initial_slots, cp_kmer_table **out);
void cp_kmer_table_destroy(cp_kmer_table *t);
/* Counts every k-mer occurrence of a labelled batch.  Asynchronous on `stream` except for one read-back of the
 * failed-insert and occupancy counters (and, when the table grows, the growth itself). */
int  cp_kmer_table_add(cp_kmer_table *t, const char *d_seq, const int64_t *d_seq_off, const char *d_labels,
                       int nreads, int64_t total_bases, void *stream);
/* Runs on and waits for the stream of the last add or consensus on `t`; reports deferred device errors (CP_EINVAL,
 * CP_EOVERFLOW) first. */
int  cp_kmer_table_stats(cp_kmer_table *t, cp_kmer_stats *out);
/* Consensus labels in place: d_labels[i] becomes the consensus label of the k-mer ending at i for every counted
 * position; the K-1 leading positions and skipped k-mers keep what d_labels holds.  A k-mer that is not in the
 * table is reported as CP_EINVAL by the next cp_kmer_table_stats.  Asynchronous on `stream`. */
int  cp_kmer_table_consensus(cp_kmer_table *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                             int64_t total_bases, char *d_labels, void *stream);
/* Occupied entries in key order into host arrays (counts4 holds 4 per entry, order E, H, D, R).  Returns the number of
 * entries; when capacity is smaller than that (or an array is NULL) nothing is written.  Runs on and waits for the stream
 * of the last add or consensus on `t`. */
int64_t cp_kmer_table_export(cp_kmer_table *t, uint64_t *hi, uint64_t *lo, uint32_t *counts4, int64_t capacity);

/* ------------------------------------------------------------------------------------------
 * K-mer count table (kprof): how often each distinct k-mer occurs in a read set, then the per-read count profiles and
 * the histogram that `FastK -k<K> -t1 -p` leaves for ClassPro, counted on the device.  Three passes: add every batch,
 * then profile every batch, and sweep the table once for the histogram.
 *
 *   Key          always canonical: min(forward, reverse complement), 2 bits per base, as FastK counts; the same key as
 *                cp_kmer_table with canonical = 1.  A k-mer that is its own reverse complement counts once per
 *                occurrence.  2 <= K <= 63; any other K is CP_EINVAL.
 *   Occurrences  the k-mer ending at read position i, for i in [K-1, rlen).  Reads shorter than K contribute nothing
 *                and their span of prof_off is empty: prof_off[r+1] - prof_off[r] = max(rlen_r - (K-1), 0).
 *   Count        the number of occurrences over everything added so far, exact: the counter has 64 bits and cannot
 *                wrap.  Only what is given out is clamped to CP_MAX_KMER_CNT, so a profile holds counts in [0, 32767]
 *                as cp_decode_profiles leaves them.
 *   Other bytes  a k-mer holding a byte other than upper-case A C G T is not counted; its profile cell is 0 and it is
 *                tallied in n_skipped (the rule of cp_kmer_table).  FastK's own treatment of such bases is not part
 *                of the reference tree and is not reproduced.
 *   Absent       a profile pass over a k-mer that is not in the table (a batch that was never added) writes 0 and
 *                makes the next cp_kmer_counts_stats return CP_EINVAL, once (the contract of cp_kmer_table_consensus);
 *                the table stays usable.
 *   Histogram    low = 1, high = 32767: hist[c-1] = distinct keys with exactly c occurrences for c < 32767,
 *                hist[32766] = distinct keys with >= 32767; ilowcnt = the occurrences of the keys with count <= 1
 *                (= hist[0]); ihighcnt = the occurrences of the keys with count >= 32767.  The two are what
 *                Load_Histogram / Modify_Histogram (libfastk.c:92-93, 116-123) keep in the hidden cells to switch
 *                between distinct k-mers and occurrences.
 * All sums are integers: profiles, histogram and statistics do not depend on the batching or the read order.
 *
 * The table grows as cp_kmer_table does: inserts past the probe bound are replayed after a rehash into at least twice
 * the slots, and it also grows past half load.  With initial_slots = 0 the first batch added sizes the still empty
 * table for all its k-mers at half load (nothing to rehash, not a growth step); a positive initial_slots is taken as
 * it is and exists so that tests can force growth.  A growth step that cannot allocate returns CP_ENOMEM and leaves
 * the table as it was.  One GPU per table; offsets are 64-bit throughout.
 */
typedef struct cp_kmer_counts cp_kmer_counts;
typedef struct
  { int64_t n_kmers;               /* counted occurrences */
    int64_t n_skipped;             /* occurrences skipped: a byte other than upper-case A C G T */
    int64_t n_distinct;            /* distinct keys */
    int64_t slots, bytes;          /* table slots now; device bytes held (slots + failure bitmaps) */
    int64_t growths;               /* growth steps so far */
  } cp_kmer_count_stats;
int  cp_kmer_counts_create(int K, int64_t initial_slots, cp_kmer_counts **out);
void cp_kmer_counts_destroy(cp_kmer_counts *t);
/* Pass 1: counts every k-mer occurrence of a batch (flat layout; neither labels nor profiles are needed).  Asynchronous
 * on `stream` except for one read-back of the failed-insert and occupancy counters (and the growth, when it grows). */
int  cp_kmer_counts_add(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                        int64_t total_bases, void *stream);
/* Pass 2: d_prof[d_prof_off[r] + i] = min(count of the k-mer at positions [i, i+K) of read r, 32767).  Asynchronous on
 * `stream`. */
int  cp_kmer_counts_profiles(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off,
                             const int64_t *d_prof_off, int nreads, int64_t total_bases, uint16_t *d_prof,
                             void *stream);
/* The FASTK histogram of the table into a host array of 32767 (see Histogram).  Runs on and waits for the stream of the
 * last add, mark, profiles or rel_labels call on `t`. */
int  cp_kmer_counts_hist(cp_kmer_counts *t, int64_t *hist, int64_t *ilowcnt, int64_t *ihighcnt);
/* Waits for the stream of the last add, mark, profiles or rel_labels call on `t`; reports a deferred device error
 * (CP_EINVAL, see Absent) first. */
int  cp_kmer_counts_stats(cp_kmer_counts *t, cp_kmer_count_stats *out);

/* ------------------------------------------------------------------------------------------
 * Filtered count table: a count table that keeps the k-mers seen ONCE out of its slots.  In a read set most distinct
 * k-mers are sequencing errors that occur once; a profile only has to say 1 for them and the histogram only needs their
 * number.  A bit array of filter_bits bits in device memory stands in front of the table, and there are three passes
 * over the same batches instead of two:
 *
 *   mark      every batch: each k-mer occurrence tests and sets its key's bits in the filter (one 64-bit word per key,
 *             up to four bits in it, one returning atomic OR); only a key whose bits were all set already enters the
 *             table, without a count.  Of two or more occurrences of a key at most one can find a bit unset, in one
 *             launch or across batches, so every key that occurs at least twice is in the table afterwards.
 *   add       the same batches through cp_kmer_counts_add: the keys are fixed now; an occurrence whose key is in the
 *             table is counted there, any other is tallied (its key occurs exactly once).  Nothing grows and nothing is
 *             read back.  Other bytes are tallied in n_skipped here, as without a filter.
 *   profiles  as before, but a valid k-mer that is not in the table gets the cell 1 and is no error.  So profiles on a
 *             filtered table CANNOT detect a batch that was never added: its k-mers read 1, or the count of the others.
 *
 * Profiles, histogram, n_kmers, n_distinct and n_skipped equal those of the unfiltered table bit for bit, for any filter
 * size, batching and order (hist[0] and ilowcnt include the keys kept outside).  A singleton whose bits were all set by
 * other keys is a false positive: it holds a slot with the exact count 1.  Which singletons those are, and so the number
 * of table keys, may depend on the order.  `bytes` of cp_kmer_count_stats includes the filter.
 *
 *   filter_bits   rounded up to a power of two; must lie in [64, 2^40], otherwise CP_EINVAL.  A rule of thumb, from a
 *                 model and not from a measurement: 16 bits (2 bytes) per expected distinct k-mer.
 *   Sizing        with initial_slots = 0 the first batch marked sizes the still empty table to the power of two at or
 *                 above total_bases / 2 slots (never below the default 2^20), a quarter of the unfiltered rule: room
 *                 for one key per four bases at half load, without reserving a slot for every k-mer of the batch.
 *                 Then the table grows as usual, except for the size of a step: failed claims are replayed after a
 *                 rehash (the replay does not ask the filter again) and the table grows past half load, but each step
 *                 only doubles it.  A failed claim of a mark pass is a second or later occurrence, many per key, so
 *                 their number says nothing about the keys still to come.
 *   Protocol      CP_EINVAL, the table left as it was: cp_kmer_counts_mark on a table without a filter or after the
 *                 first cp_kmer_counts_add; cp_kmer_counts_rel_labels on a filtered table (it cannot tell a count of 0
 *                 from a count of 1); cp_kmer_counts_hist and cp_kmer_counts_stats while n_marked != n_counted (the
 *                 marked and the added batches differ; the message gives both numbers).
 */
typedef struct { int64_t filter_bits, filter_bytes, n_marked, n_counted, n_table_keys, n_outside, n_false; } cp_kmer_filter_stats;
int  cp_kmer_counts_create_filtered(int K, int64_t initial_slots, int64_t filter_bits, cp_kmer_counts **out);
/* The mark pass over a batch.  Asynchronous on `stream` except for the read-back and growth of cp_kmer_counts_add. */
int  cp_kmer_counts_mark(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                         int64_t total_bases, void *stream);
/* Runs on and waits for the stream of the last call that queued work on `t`; legal at any time and on any count table (filter_bits = 0 without a filter).  n_marked / n_counted: valid
 * k-mer occurrences of the mark / add passes so far; n_table_keys: keys that hold a slot; n_outside: keys kept outside
 * (known once the batches are added); n_false: table keys with count 1 (a slot sweep). */
int  cp_kmer_counts_filter_stats(cp_kmer_counts *t, cp_kmer_filter_stats *out);

/* ------------------------------------------------------------------------------------------
 * Relative labels (genome2class): the ground truth of a read set from a count table of ANOTHER sequence set, the
 * assembly.  What `FastK -p:genome` + prof2class give (src/prof2class.c:241-254), in one pass over a batch in the flat
 * layout; the batch need not be (and usually is not) what was added to `t`.
 *
 *   Key       one canonical lookup per k-mer position, the key of "K-mer count table".  c = the count in the table.
 *   Label     c == 0 -> E, 1 -> H, 2 -> D, >= 3 -> R.  Read r gets 'N' on its first min(K-1, rlen_r) positions (the
 *             read rule of cp_threshold_labels); reads shorter than K and empty reads are legal.
 *   Absent    a k-mer that is not in the table has c = 0, and so has one that holds a byte other than upper-case
 *             A C G T.  Neither is an error: the call never sets the table's deferred error and never changes the
 *             table (cp_kmer_counts_stats and cp_kmer_counts_hist give the same before and after).
 *   Outputs   each optional (NULL = not wanted, at least one required; a pair with one half NULL is CP_EINVAL):
 *             d_prof   + d_prof_off [nreads+1]: min(c, 32767) in the cell layout of cp_kmer_counts_profiles;
 *             d_labels [total_bases]  the characters;
 *             d_packed + d_pack_off [nreads+1]: the 2-bit layout of cp_pack_labels, written directly;
 *             d_counts int64 [4] on the device, order E, H, D, R, ADDED TO, so several batches accumulate.
 * All results are integers and do not depend on the batching or the read order.  Asynchronous on `stream`.
 */
int  cp_kmer_counts_rel_labels(cp_kmer_counts *t, const char *d_seq, const int64_t *d_seq_off, int nreads,
                               int64_t total_bases, uint16_t *d_prof, const int64_t *d_prof_off, char *d_labels,
                               uint8_t *d_packed, const int64_t *d_pack_off, int64_t *d_counts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Sorted k-mers (kprof -t): a snapshot of a count table in key order, and the payload of the FASTK k-mer table
 * (`<root>.ktab`, `.<root>.ktab.N`) that libfastk.c's Open_Kmer_Stream / Load_Kmer_Table / Find_Kmer read, encoded on
 * the device.
 *
 *   Snapshot   every key of the table with count >= min_count, ascending by the 2K-bit key read as the integer
 *              hi << 63 | lo: the first base is the most significant, A < C < G < T, FastK's order.  Keys are distinct,
 *              so the result does not depend on the slot order or on scheduling.  d_cnt holds the exact 64-bit count.
 *              The table is only read (cp_kmer_counts_hist and cp_kmer_counts_stats give the same before and after); a
 *              snapshot does not follow later adds, a second sort after more adds does.  An empty result is no error:
 *              the size is 0 and the array pointers are null.
 *   min_count  must lie in [1, 32767], otherwise CP_EINVAL.  On a filtered table min_count = 1 is CP_EINVAL (the keys
 *              seen once hold no slot), and so is a table whose marked and added batches differ (the check of
 *              cp_kmer_counts_stats, made first); with min_count >= 2 the result is that of the unfiltered table.
 *   Record     kbyte = (K+3)>>2 bytes hold the key left-aligned: the first base in bits 7..6 of byte 0, unused low
 *              bits of the last byte 0.  The first ibyte = cp_ktab_ibyte(K) bytes are the prefix: 3 for K >= 13, 2 for
 *              K in 9..12, 1 for K in 5..8; 0 for K < 5, for which there is no .ktab (cp_kmer_sorted_ktab is
 *              CP_EINVAL).  A record is the other hbyte = kbyte - ibyte bytes, then min(count, CP_MAX_KMER_CNT) as a
 *              little-endian uint16: pbyte = hbyte + 2 bytes.
 *   ktab       d_records receives the records of the entries [first, first+n), n * pbyte bytes (any alignment; a range
 *              outside the snapshot is CP_EINVAL, n = 0 is legal).  d_index, when not NULL, receives 1 << (8*ibyte)
 *              int64: index[p] = the number of entries of the WHOLE snapshot whose prefix is <= p.  Asynchronous on
 *              `stream`.
 *   Memory     24 bytes per entry and 8 bytes per prefix ((1 << 8*ibyte) + 1 of them; 4^K + 1 for K < 5) on top of
 *              the table: cp_kmer_sorted_bytes.  An allocation that fails is CP_ENOMEM with the byte count in the
 *              message; the table is untouched.  cp_kmer_counts_sort synchronises `stream`.
 *   Tile       cp_ktab_tile: the number of entries one block sorts on chip.  A prefix with more entries than that is
 *              sorted by a path of its own; the constant is exported so that tests can place sizes around it.
 */
typedef struct cp_kmer_sorted cp_kmer_sorted;
int     cp_kmer_counts_sort(cp_kmer_counts *t, int64_t min_count, void *stream, cp_kmer_sorted **out);
void    cp_kmer_sorted_destroy(cp_kmer_sorted *s);
int64_t cp_kmer_sorted_size(const cp_kmer_sorted *s);       /* host values: nothing is waited for */
int64_t cp_kmer_sorted_bytes(const cp_kmer_sorted *s);
/* Device pointers to size() words each, valid until destroy; the words are written when the call that made `s` has returned. */
int     cp_kmer_sorted_arrays(const cp_kmer_sorted *s, const uint64_t **d_hi, const uint64_t **d_lo,
                              const uint64_t **d_cnt);
int     cp_kmer_sorted_ktab(cp_kmer_sorted *s, int64_t first, int64_t n, uint8_t *d_records, int64_t *d_index,
                            void *stream);
int     cp_ktab_ibyte(int K);
int     cp_ktab_tile(void);

/* ------------------------------------------------------------------------------------------
 * Sorted k-mers of a label table (class2ktab): the same snapshot taken of a cp_kmer_table, one consensus class per
 * call, so that the classes of the k-mers themselves become FASTK k-mer tables (the haploid k-mers as hap-mers, the
 * repeat k-mers as a mask), and the FASTK histogram of each class.
 *
 *   Per key    total = the sum of the four label counts, in 64 bits (below 2^34); max = the largest of the four;
 *              cls = the consensus label of "Per-k-mer label table": the largest count, a tie R > D > H > E.
 *   Selected   a key for which all three hold: label == -1 or cls == label (label 0..3 is E, H, D, R; -1 is every
 *              key); total >= min_total; 100 * max >= min_pct * total, in integers.  So min_pct = 100 keeps exactly
 *              the unanimous keys, counts (2, 1, 0, 0) pass 66 and fail 67, and (1, 1, 0, 0) is class H, passes 50
 *              and fails 51.
 *   Result     an ordinary cp_kmer_sorted: the selected keys ascending by hi << 63 | lo, d_cnt the exact total;
 *              cp_kmer_sorted_size, _bytes, _arrays, _ktab and _destroy work on it unchanged, a record carries
 *              min(total, CP_MAX_KMER_CNT), and cp_kmer_sorted_ktab stays CP_EINVAL for K < 5.  An empty selection is
 *              size 0 with null arrays and is no error.
 *   Arguments  label in [-1, 3], min_total in [1, 32767], min_pct in [0, 100]; anything else is CP_EINVAL, and so is a
 *              NULL t or out.  The table is untouched.
 *   Table      only read: cp_kmer_table_stats and cp_kmer_table_export give the same before and after, and a snapshot
 *              does not follow later adds.  Forward and canonical tables are both legal; the key order is the same.
 *              Neither call reports or clears the table's deferred error (a caller that wants it asks
 *              cp_kmer_table_stats first).  cp_kmer_table_sort synchronises `stream`, and the stream of the table's
 *              last add first when the two differ.  An allocation that fails is CP_ENOMEM with the byte count in the
 *              message, nothing leaked.
 *   Histogram  cp_kmer_table_class_hist, for each class l in the order E, H, D, R: hist[l][c-1] = distinct keys with
 *              cls == l and total == c for c < 32767, hist[l][32766] = those with total >= 32767, ilowcnt[l] =
 *              hist[l][0], ihighcnt[l] = the sum of total over the keys with total >= 32767: the contract of
 *              cp_kmer_counts_hist, four times.  No min_total and no min_pct.  Runs on and waits for the stream of the
 *              last add or consensus on the table.
 * On a canonical table the four class snapshots at min_total = 1, min_pct = 0 partition the label = -1 snapshot, which
 * is cp_kmer_counts_sort(min_count 1) of a count table fed the same reads (keys, counts, records, index), and the
 * four class histograms sum cell for cell to that table's cp_kmer_counts_hist.
 */
int     cp_kmer_table_sort(cp_kmer_table *t, int label, int64_t min_total, int min_pct, void *stream,
                           cp_kmer_sorted **out);
int     cp_kmer_table_class_hist(cp_kmer_table *t, int64_t *hist /* [4][32767] */, int64_t *ilowcnt /* [4] */,
                                 int64_t *ihighcnt /* [4] */);

/* ------------------------------------------------------------------------------------------
 * Sorted k-mers as input (tab2prof): a snapshot loaded from the payload of a FASTK k-mer table, and the two queries that
 * every snapshot answers -- what libfastk.c's Load_Kmer_Table, Find_Kmer and `FastK -p:<table>` do with a .ktab.
 *
 *   Load       the exact inverse of cp_kmer_sorted_ktab, in three steps.
 *              load_begin    `index` is the stub's HOST array of 1 << 8*ibyte int64, ibyte = cp_ktab_ibyte(K).  K must lie
 *                            in [5, 63] and the index must be non-negative and non-decreasing, otherwise CP_EINVAL.  n =
 *                            the last index cell.  Allocates the 24 n bytes and the bucket starts (start[0] = 0,
 *                            start[p+1] = index[p]); an allocation that fails is CP_ENOMEM with the byte count in the
 *                            message, nothing leaked.  Synchronous (one copy of the starts).
 *              load_records  appends the next n entries from device bytes of any alignment, n * pbyte of them, in file
 *                            order (so there is no `first`); n = 0 is legal, an append past the end is CP_EINVAL and
 *                            appends nothing.  An entry's prefix is the bucket whose range of the index holds its
 *                            ordinal; the key is prefix and the record's hbyte bytes with the pad bits of the last byte
 *                            dropped; the count is the little-endian uint16.  Asynchronous on `stream`; the bytes may be
 *                            reused once the stream has passed the call.
 *              load_end      CP_EINVAL unless all n entries were appended.  Then checks key[i-1] < key[i] for every i:
 *                            a key that repeats or steps back is CP_EINVAL with the first offending ordinal i in the
 *                            message (the snapshot stays unready).  Synchronises `stream`.
 *   Ready      only after a successful load_end is a loaded snapshot ready; the snapshots of cp_kmer_counts_sort and
 *              cp_kmer_table_sort are born ready.  On a snapshot that is not ready cp_kmer_sorted_find, _profiles,
 *              _ktab and _arrays are CP_EINVAL; _size, _bytes and _destroy are always legal.  load_records and load_end
 *              on a ready snapshot are CP_EINVAL.  A loaded snapshot is an ordinary cp_kmer_sorted: its _ktab gives back
 *              the bytes it was loaded from (records whose pad bits were 0) and the index.
 *   Find       d_pos[i] = the ordinal of the key d_hi[i] << 63 | d_lo[i] in the snapshot, or -1 when it is absent (so is a
 *              key that no k-mer of this K can have): Find_Kmer's return value (libfastk.c:662-709) for a key that is
 *              canonical already.  Works for every K a snapshot can have, K < 5 included (a bucket is the whole key).
 *   Profiles   the cell layout of cp_kmer_counts_profiles: d_prof[d_prof_off[r] + i] = min(cnt, 32767) of the key of the
 *              k-mer at positions [i, i+K) of read r, or 0 when that key is absent.  With `canonical` non-zero the key is
 *              min(forward, reverse complement), the key of a count table; with 0 it is the forward k-mer, for the
 *              snapshots of a forward cp_kmer_table.  A k-mer that holds a byte other than upper-case A C G T gives 0.
 *              An absent key is never an error.  d_tally, when not NULL, is int64 [3] on the device and is ADDED TO:
 *              cells present, cells absent, cells with other bytes.  Reads shorter than K and empty reads are legal.
 *   Lookup     bucket = the key's top 8*ibyte bits (the whole key for K < 5), then a binary search over
 *              [start[bucket], start[bucket+1]) clamped to [0, n], at most 64 probes: no content of a snapshot can make
 *              a lookup run on or read outside the arrays (the first two probes may be placed by interpolation on the
 *              key's suffix instead of at the middle; the result is the same).  When 2K-63 <= 8*ibyte (K <= 43 with three prefix bytes, every
 *              K <= 31) the bucket fixes hi: only lo is compared and hi[] is never read.
 * The snapshot is only read by both queries; both are asynchronous on `stream`.
 */
int     cp_kmer_sorted_load_begin(int K, const int64_t *index, cp_kmer_sorted **out);
int     cp_kmer_sorted_load_records(cp_kmer_sorted *s, int64_t n, const uint8_t *d_records, void *stream);
int     cp_kmer_sorted_load_end(cp_kmer_sorted *s, void *stream);
int     cp_kmer_sorted_find(const cp_kmer_sorted *s, const uint64_t *d_hi, const uint64_t *d_lo, int64_t m,
                            int64_t *d_pos, void *stream);
int     cp_kmer_sorted_profiles(const cp_kmer_sorted *s, int canonical, const char *d_seq, const int64_t *d_seq_off,
                                const int64_t *d_prof_off, int nreads, int64_t total_bases, uint16_t *d_prof,
                                int64_t *d_tally, void *stream);

/* ------------------------------------------------------------------------------------------
 * Set algebra on sorted k-mers (tabop): two snapshots combined into a third by a streaming merge on the device -- what
 * FASTK's Logex does with two k-mer tables -- and the FASTK histogram of a snapshot.  Everything is in integers and
 * independent of tile size and scheduling.
 *
 *   Presence   a key is IN A when A holds it and a_min <= cntA <= a_max, cntA being the snapshot's own d_cnt (the exact
 *              64-bit count of a snapshot sorted here, at most 32767 for a loaded one); IN B likewise.  `range` is a
 *              HOST array a_min a_max b_min b_max; NULL means [1, INT64_MAX] for both.  An entry outside its range is
 *              treated exactly as if it were absent.
 *   Kept       CP_SET_AND a key in A and in B; CP_SET_OR in either; CP_SET_SUB in A and not in B; CP_SET_XOR in exactly
 *              one.
 *   Count      of a kept key: CP_CNT_LEFT is cntA when in A, otherwise cntB; CP_CNT_SUM the sum over the sides it is in;
 *              CP_CNT_MIN and CP_CNT_MAX over the sides it is in.  Under SUB and XOR one side is in, so all four give
 *              that side's count.  Sums are exact in 64 bits; a record clamps at CP_MAX_KMER_CNT, as everywhere.
 *   Result     an ordinary cp_kmer_sorted, born ready, keys ascending, with memory of its own (it survives destroying a
 *              and b) and its bucket starts rebuilt: cp_kmer_sorted_size, _bytes, _arrays, _ktab, _find, _profiles and
 *              _destroy work on it unchanged.  An empty result is size 0 with null arrays and is no error.
 *   Tally      a HOST array: keys in A only, in B only, in both (each after the ranges), and the result's size.  With
 *              out == NULL only the tally is computed and nothing of result size is allocated.
 *   Operands   both ready and of the same K; a == b is legal; K < 5 is legal.  Both are only read: their _ktab gives
 *              the same bytes before and after.
 *   Errors     CP_EINVAL for a NULL a or b, for out and tally both NULL, an unready operand, differing K, a set_op or
 *              cnt_op outside the enums, a range with min < 1 or max < min.  An allocation that fails is CP_ENOMEM with
 *              the byte count in the message, nothing leaked.  Synchronises `stream`: the result's size must be known
 *              to allocate it.
 *   Memory     on top of the result (24 bytes per entry and the bucket starts) 24 bytes per tile of cp_ktab_tile()
 *              entries of the two operands together, never 24 bytes per operand entry.
 *   Histogram  cp_kmer_sorted_hist, the contract of cp_kmer_counts_hist over a snapshot's d_cnt: hist[c-1] = entries with
 *              count c for c < 32767, hist[32766] = those with count >= 32767, ilowcnt = hist[0], ihighcnt = the sum of
 *              the counts >= 32767.  CP_EINVAL on an unready snapshot.  It takes no stream: a snapshot is complete when the
 *              call that made it has returned, so there is nothing to wait for but the call's own sweep, which runs on
 *              the null stream and is waited for.  For cp_kmer_counts_sort(t, 1) it equals cp_kmer_counts_hist(t) cell
 *              for cell.
 */
enum { CP_SET_AND = 0, CP_SET_OR = 1, CP_SET_SUB = 2, CP_SET_XOR = 3 };
enum { CP_CNT_LEFT = 0, CP_CNT_SUM = 1, CP_CNT_MIN = 2, CP_CNT_MAX = 3 };
int     cp_kmer_sorted_combine(const cp_kmer_sorted *a, const cp_kmer_sorted *b, int set_op, int cnt_op,
                               const int64_t *range /* host [4]: a_min a_max b_min b_max, or NULL */,
                               int64_t *tally /* host [4], or NULL */, void *stream,
                               cp_kmer_sorted **out /* or NULL: tally only */);
int     cp_kmer_sorted_hist(const cp_kmer_sorted *s, int64_t *hist /* host [32767] */, int64_t *ilowcnt, int64_t *ihighcnt);

/* ------------------------------------------------------------------------------------------
 * Read hits in two sorted k-mer sets (tabbin): per read of a batch in the flat layout above, how many of its k-mer
 * positions carry a key that only A holds, that only B holds, that both hold, and how often the A and B markers switch
 * sides along the read -- what trio binning asks of two parental marker sets, and what a switch error or a chimeric read
 * looks like.  One pass over the bases; every key is rolled once and looked up in both snapshots.  Everything is in
 * integers.
 *
 *   Presence   exactly as in cp_kmer_sorted_combine: a key is IN A when A holds it and a_min <= cntA <= a_max with the
 *              snapshot's own d_cnt; IN B likewise.  `range` is a HOST array a_min a_max b_min b_max; NULL means
 *              [1, INT64_MAX] for both.
 *   Marker     of a k-mer position.  The key is chosen as in cp_kmer_sorted_profiles: min(forward, reverse complement)
 *              with `canonical` non-zero, the forward k-mer with 0.  The marker is A for a key in A and not in B, B for a
 *              key in B and not in A, BOTH for a key in both, and none otherwise.  A k-mer that holds a byte other than
 *              upper-case A C G T is OTHER.  The snapshots need not be disjoint: two raw parental tables give the A and B
 *              markers that their two differences (CP_SET_SUB either way) would give.
 *   Row        d_hits[r*CP_HIT_WIDTH + ...] of read r: CP_HIT_A, CP_HIT_B, CP_HIT_BOTH and CP_HIT_OTHER are the numbers of
 *              its positions with that marker.  CP_HIT_SWITCHES: take the positions marked A or B in read order, ignoring
 *              every other position; it is the number of adjacent pairs of that subsequence whose markers differ.  Reads
 *              shorter than K and empty reads give a row of zeros.  Every row is written, never added to.
 *   Fixed      a row is a function of the read and the two snapshots alone: not of what else is in the batch, of the order
 *              of the reads, or of the block and chunk sizes of the kernels.
 *   Operands   both ready and of the same K; a == b is legal (every hit is BOTH), so is a snapshot of size 0.  Both are
 *              only read.  Lookups are those of "Sorted k-mers as input": clamped ranges, at most 64 probes.
 *   Errors     all before any launch: CP_EINVAL for a NULL a or b, an unready snapshot, differing K, a range with
 *              min < 1 or max < min, a negative nreads or total_bases, a null device pointer when there is work
 *              (nreads == 0 is no work and no error).  Scratch, 32 bytes per 16384 bases of the batch, is allocated and
 *              freed in stream order per call; when that fails it is CP_ENOMEM with the byte count in the message.
 * Asynchronous on `stream`.
 *
 * cp_bin_call is the one rule by which a row becomes a call; host only, no device involved.  It returns 'U' when
 * nA + nB < min_markers; otherwise 'A' when nA * wB > nB * wA, 'B' when nB * wA > nA * wB, and 'U' for a tie, the products
 * taken in 128 bits.  wA = only_a and wB = only_b when `normalise` is non-zero and both are positive, otherwise both are
 * 1: only_a and only_b are the numbers of distinct keys only in A and only in B (tally[0] and tally[1] of
 * cp_kmer_sorted_combine with out == NULL and the same ranges), and dividing a read's hits by the sizes of the two marker
 * sets is how trio binning scores it.  CP_EINVAL for a NULL hit.
 */
enum { CP_HIT_A = 0, CP_HIT_B = 1, CP_HIT_BOTH = 2, CP_HIT_OTHER = 3, CP_HIT_SWITCHES = 4, CP_HIT_WIDTH = 5 };
int     cp_kmer_sorted_read_hits(const cp_kmer_sorted *a, const cp_kmer_sorted *b, int canonical,
                                 const int64_t *range /* host [4]: a_min a_max b_min b_max, or NULL */,
                                 const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases,
                                 int64_t *d_hits /* device [nreads][CP_HIT_WIDTH], overwritten */, void *stream);
int     cp_bin_call(const int64_t *hit /* [CP_HIT_WIDTH] */, int64_t only_a, int64_t only_b, int64_t min_markers,
                    int normalise);

/* ------------------------------------------------------------------------------------------
 * Runs of k-mer states along reads (tabtrack): the k-mer positions of a batch in the flat layout above, looked up in one
 * or two snapshots and reduced to runs of equal state on the device -- WHERE along a read or a contig the k-mers are that
 * a table does not hold (the intervals of an assembly that the reads do not support, the errors of a read), and where the
 * A and B markers of "Read hits in two sorted k-mer sets" form phase blocks.  Only the runs come down, never a value per
 * base.  Every key is rolled once and looked up once per snapshot.  Everything is in integers.
 *
 *   State      of a k-mer position: the marker of cp_kmer_sorted_read_hits, with the same key choice (`canonical`), the
 *              same presence rule and the same HOST `range` a_min a_max b_min b_max (NULL: [1, INT64_MAX] for both).
 *              CP_RUN_NONE a key in neither, CP_RUN_A in A and not in B, CP_RUN_B in B and not in A, CP_RUN_BOTH in both,
 *              CP_RUN_OTHER a k-mer that holds a byte other than upper-case A C G T.  b == NULL means no second table:
 *              the states are NONE, A and OTHER only, and a key is looked up once.
 *   Run        `skip` and `emit` are masks over the states, bit 1 << state.  A position whose state is in `skip` is
 *              transparent: it neither breaks nor extends anything.  Of the other positions of ONE read, in order, a run is
 *              a maximal stretch of equal state.  Its record: `first` and `last` the ordinals in the read of its first and
 *              last position (k-mer i covers the bases [i, i+K) of the read), `n` the number of its positions (with
 *              skip == 0, n == last-first+1), `read` the read's index in the batch, `state`.  A run whose state is not in
 *              `emit` is not written, but still separates its neighbours.
 *   Output     d_run_off[r] .. d_run_off[r+1] are the records of read r in d_runs, ascending in `first`; all nreads+1
 *              offsets are overwritten, and *total (HOST) = d_run_off[nreads].  Reads shorter than K, empty reads and
 *              nreads == 0 give no runs and are no error.
 *   Capacity   d_runs holds `capacity` records.  With *total > capacity the call returns CP_EOVERFLOW; d_run_off and
 *              *total are exact all the same, the records below `capacity` are written and nothing beyond them is touched.
 *              d_runs == NULL with capacity == 0 is the counting call.
 *   Fixed      the records of a read are a function of the read, the snapshots, the ranges and the masks alone: not of what
 *              else is in the batch, of the order of the reads, or of the grid, block and chunk sizes of the kernels.
 *   Operands   ready and of the same K; a == b is legal, so is a snapshot of size 0.  Both are only read.  Lookups are
 *              those of "Sorted k-mers as input": clamped ranges, at most 64 probes.
 *   Errors     all before any launch: CP_EINVAL for a NULL a or total, an unready snapshot, differing K, a range with
 *              min < 1 or max < min, emit == 0, emit & skip != 0, a mask above 0x1f, a negative nreads, total_bases or
 *              capacity, a null device pointer where there is work (d_runs with capacity > 0, d_run_off and d_seq_off
 *              with nreads > 0, d_seq with total_bases > 0).
 *   Memory     scratch of one byte per base of the batch and 32 bytes per 16384 bases, allocated and freed in stream
 *              order per call; when that fails it is CP_ENOMEM with the byte count in the message.
 *              Nothing is queued on `stream` before that allocation has succeeded.
 *   Cost       one pass of lookups and two light passes over the state bytes.  The offsets of a stretch of reads without a
 *              k-mer position (shorter than K, or empty) are stored one after the other by the one lane that meets the
 *              next read, and a read's last run is closed by one binary search over d_seq_off: nothing for reads and
 *              contigs, but a batch of millions of reads shorter than K is serialised in single lanes.
 * Synchronises `stream`: the total must be known to return it.
 *
 * cp_run_blocks is the one rule by which the runs of ONE read -- every state that is not skipped emitted -- become blocks;
 * host only, no device involved.  The runs with n < min_n are dropped; of those that are left, neighbours of equal state
 * are merged into one block: `first` of the first, `last` of the last, n summed, `read` and `state` of the first.  It
 * writes the blocks in order (at most nruns; `blocks` may be `runs`), sets *dropped to the number of dropped runs and
 * returns the number of blocks.  The rule is this library's own, not Merqury's, which tolerates switches within a
 * distance.  CP_EINVAL for a NULL runs, blocks or dropped, min_n < 1 or a negative nruns.
 */
enum { CP_RUN_NONE = 0, CP_RUN_A = 1, CP_RUN_B = 2, CP_RUN_BOTH = 3, CP_RUN_OTHER = 4 };
typedef struct cp_kmer_run { int64_t first, last, n; int32_t read, state; } cp_kmer_run;
int     cp_kmer_sorted_read_runs(const cp_kmer_sorted *a, const cp_kmer_sorted *b /* or NULL */, int canonical,
                                 const int64_t *range /* host [4]: a_min a_max b_min b_max, or NULL */,
                                 unsigned int skip, unsigned int emit,
                                 const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases,
                                 cp_kmer_run *d_runs /* device [capacity], or NULL */, int64_t capacity,
                                 int64_t *d_run_off /* device [nreads+1], overwritten */, int64_t *total /* host */,
                                 void *stream);
int64_t cp_run_blocks(const cp_kmer_run *runs, int64_t nruns, int64_t min_n, cp_kmer_run *blocks, int64_t *dropped);

/* ------------------------------------------------------------------------------------------
 * Fixing reads from a k-mer table (tabfix): error correction against solid k-mers.  The runs of absent k-mers of "Runs of
 * k-mer states along reads" are the errors of a read, about K positions per substitution; here such a run is turned into
 * the ONE edit of the read that makes every k-mer around it present, where there is exactly one, and the edits are applied
 * on the device.  The rule is this library's own.  Everything is in integers and is a function of the read and the
 * snapshot alone.
 *
 *   Positions  a sequence s of n bases has P = n-K+1 k-mer positions, position p covering the bases [p, p+K).  The state of
 *              a position is the one cp_kmer_sorted_read_runs gives with one table (b == NULL): present (CP_RUN_A),
 *              CP_RUN_NONE or CP_RUN_OTHER, with the same `canonical` switch and the same count range a_min a_max (HOST
 *              `range`, NULL: [1, INT64_MAX]).
 *   Gap        a maximal run [i, j] of NONE positions.  It is CLOSED when i >= 1, j <= P-2 and both neighbouring positions
 *              are present, and OPEN otherwise: at an end of the sequence, or beside an OTHER position.  For a closed gap
 *              L = j-i+1, e = i+K-1, f = j, g = f-e+1 = L-K+1 and t = -g.  Base e is the first base a left-to-right
 *              reading cannot explain, base f the last base a right-to-left reading cannot explain: one substitution gives
 *              L = K and e == f, an insertion of g bases gives L = K+g-1, a lost base L = K-1, and a change inside a
 *              repeat a shorter gap still (t > 0), because the k-mers that lie inside the repeat do not see it.
 *   Candidates with D = max_indel in [0, 4], every candidate (del, ins) replaces s[e, e+del) by the string ins.  In this order:
 *                g >= 1   (d, "") for d = g .. D: the read had an insertion.  When g == 1 also (1, c) for the three bases
 *                         c != s[e], in the order A C G T: a substitution.
 *                g <= 0   (d, "") for d = 1 .. D.  When D >= 1, (0, c) for the four bases c in the order A C G T: the read
 *                         lost a base.  Then (0, s[e-d, e)) for d = 2 .. min(D, t): the read lost a copy of a tandem unit.
 *              A candidate with e+del > n does not exist.  There are at most 2D+3 candidates for one gap, and all of them
 *              give different strings.
 *   Accepted   let c be the sequence after the edit.  The checked positions q run from e-K+1 = i to e+|ins|-1, for a pure
 *              removal from i to e-1, both ends clipped to [0, len(c)-K]: K-1+|ins| k-mers at most.  The candidate is
 *              accepted when that range is not empty and every k-mer in it is present under the same presence rule (a
 *              k-mer with a byte other than A C G T is not present).
 *   Status     CP_FIX_NONE candidates were tried and none was accepted; CP_FIX_ONE exactly one was accepted, it is the fix;
 *              CP_FIX_MANY more than one was accepted, the gap is left alone; CP_FIX_OPEN the gap is open and was not
 *              tried; CP_FIX_NOCAND a closed gap with no candidate (g > D and g != 1, or D == 0 and g <= 0);
 *              CP_FIX_CLASH, below.
 *   Clash      a ONE fix becomes CLASH in two cases, both taken on the statuses before any clash is decided: e < e'+del'
 *              for the gap just before it in the same sequence when that gap is ONE, and e+del > e'' for the gap just
 *              after it when that gap is ONE.  Both partners go.  Gaps that are not neighbours cannot overlap: the next
 *              gap begins at i'' >= j+2, so e'' >= j+K+1; its j'' >= j+2, so the next but one has e''' >= j+K+3; and
 *              e+del <= j+K-1+D <= j+K+3 with D <= 4.
 *   So         the applied edits of a sequence are disjoint and ascending, and after ONE edit every k-mer outside its checked
 *              window is the same string as before.  An edit takes the positions [i, max(e+del, e)-1] of the sequence away and
 *              puts its window, all present, in their place; the window reads the bases [i, e+del+K-2].  Where every applied
 *              fix stands alone -- the next gap begins behind e+del-1 and the next applied fix has e'' >= e+del+K-1 -- the
 *              NONE positions of the corrected sequence number exactly the NONE positions before less the sum of L over the
 *              applied gaps.  Where fixes stand closer (two errors within about K bases) the windows were checked without
 *              the neighbour's edit, and a removal of more than g+1 bases takes positions of the next gap with it: the
 *              identity is no theorem there.  The result does not depend on batching, read order, grid or chunk sizes.
 *   Scope      one error per gap.  Two errors closer than K give one gap with g >= 2 and stay; a deletion of two or more
 *              bases outside a repeat stays (4^d candidates).  Where repeats reach K, gaps stay ambiguous.
 *
 * cp_kmer_sorted_read_fixes: one record per gap of the batch (the flat layout above), a cp_kmer_fix of 32 bytes.
 *   Record     `first` = i and `last` = j as in a cp_kmer_run, `read` the read's index in the batch, `status`, `nacc` the
 *              number of accepted candidates; `del`, `nins` and `ins` (upper-case bases, zero padded) are the edit when the
 *              status is ONE or CLASH and zero otherwise.  The records correspond one to one, offsets included, with the
 *              NONE runs of cp_kmer_sorted_read_runs(s, NULL, ..., skip 0, emit 1 << CP_RUN_NONE).
 *   Output     d_fix_off[r] .. d_fix_off[r+1] are the records of read r, ascending in `first`; all nreads+1 offsets are
 *              overwritten and *total (HOST) = d_fix_off[nreads].  Reads shorter than K, empty reads and nreads == 0 give
 *              no records and are no error.  d_tally, a DEVICE int64 [CP_FIX_WIDTH] or NULL, is ADDED TO: one cell per
 *              status.
 *   Capacity   d_fixes holds `capacity` records.  With *total > capacity the call returns CP_EOVERFLOW; d_fix_off and
 *              *total are exact all the same.  A fix needs the records of its neighbours, so a call that overflows writes
 *              no record at all and adds nothing to d_tally.  d_fixes == NULL with capacity == 0 is the counting call.
 *   Passes     the state bytes, block summaries, scan and write pass of the runs; then one wave per gap tries the
 *              candidates, lane l looking up the k-mer at checked position i+l; then two passes of one lane
 *              per record apply the clash rule, the first deciding from what the second alone stores.  Lookups are those of "Sorted k-mers as input": clamped ranges, at most 64 probes.
 *   Errors     all before any launch: CP_EINVAL for a NULL s or total, an unready snapshot, a snapshot of K < 5 (a candidate
 *              reads the five bases s[e-4 .. e]), a range with min < 1 or max < min, max_indel outside [0, 4], a negative nreads, total_bases or capacity, a null device pointer
 *              where there is work (as in cp_kmer_sorted_read_runs).  Scratch as there, but allocated and freed
 *              outside the stream's order; CP_ENOMEM with the byte count in the message and nothing queued before it.
 *              A batch with more than 2^24 gaps is CP_EINVAL once their number is known, with *total set and no record
 *              written: that is what cp_apply_fixes takes in one call, so what one call gives the other takes.
 *              The snapshot and the batch are only read.  Synchronises `stream`.
 *
 * cp_apply_fixes: the batch with the records of status CP_FIX_ONE applied and nothing else, as a batch of the same layout.
 *   K          the k of the snapshot that made the records: e = first+K-1.
 *   Output     d_out_off [nreads+1] is overwritten with the new offsets and *out_total (HOST) = d_out_off[nreads];
 *              d_out[d_out_off[r] .. d_out_off[r+1]) is read r with its edits.  With *out_total > out_capacity the call
 *              returns CP_EOVERFLOW with exact offsets and total and d_out untouched.  total_bases + 4 * records always
 *              suffices.
 *   Clamped    everything read from d_fixes is checked: a record is an edit only when its status is ONE, del and nins are at
 *              most 4, its `read` is the read whose records hold it, 0 <= first, e < n and e+del <= n; anything else is
 *              treated as "no edit".  Offsets read from d_fix_off are clamped to [0, d_fix_off[nreads]], every store is
 *              checked against the read's new extent and out_capacity.  Records that are not ascending in `first` give
 *              unspecified bases, but no content of the records makes a lane read or write outside the arrays.
 *   Passes     the signed length change per record, its scan over all records, the offsets, then a copy in which a lane owns
 *              64 consecutive input bases: it finds their read, the last edit at or before them by a binary search in the
 *              read's records, and walks.  No lane is serial over a sequence: a contig of many blocks is copied by many.
 *   Errors     CP_EINVAL before any launch for K outside [5, 63], negative sizes, a NULL out_total, null device pointers
 *              where there is work; the number of records (d_fix_off[nreads]) is read first, and at most 2^24 records are
 *              taken per call.  Scratch of 8 bytes per record, CP_ENOMEM with the byte count in the message.  The batch and
 *              the records are only read.  Synchronises `stream`.
 */
enum { CP_FIX_NONE = 0, CP_FIX_ONE = 1, CP_FIX_MANY = 2, CP_FIX_OPEN = 3, CP_FIX_NOCAND = 4, CP_FIX_CLASH = 5, CP_FIX_WIDTH = 6 };
typedef struct cp_kmer_fix { int64_t first, last; int32_t read; uint8_t status, del, nins, nacc; char ins[8]; } cp_kmer_fix;
int     cp_kmer_sorted_read_fixes(const cp_kmer_sorted *s, int canonical, const int64_t *range /* host [2], or NULL */,
                                  int max_indel, const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases,
                                  cp_kmer_fix *d_fixes /* device [capacity], or NULL */, int64_t capacity,
                                  int64_t *d_fix_off /* device [nreads+1], overwritten */, int64_t *total /* host */,
                                  int64_t *d_tally /* device [CP_FIX_WIDTH], added to, or NULL */, void *stream);
int     cp_apply_fixes(const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases, int K,
                       const cp_kmer_fix *d_fixes, const int64_t *d_fix_off /* device [nreads+1] */,
                       char *d_out /* device [out_capacity] */, int64_t out_capacity,
                       int64_t *d_out_off /* device [nreads+1], overwritten */, int64_t *out_total /* host */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Count comparison of sorted k-mers (tabcmp): the joint distribution of the counts that two snapshots give one key -- the
 * matrix of KAT's comp and the spectra-cn of Merqury (the read-count spectrum split by the copy number in an assembly) --
 * by the streaming merge of "Set algebra on sorted k-mers", and the k-mer QV that follows from it.  Everything on the
 * device is in integers and independent of tile size, grid and scheduling.
 *
 *   Presence   exactly as in cp_kmer_sorted_combine: a key is IN A when A holds it and a_min <= cntA <= a_max with the
 *              snapshot's own d_cnt; IN B likewise.  `range` is a HOST array a_min a_max b_min b_max; NULL means
 *              [1, INT64_MAX] for both.  An entry outside its range is treated exactly as if it were absent.
 *   Cell       a key that is in A or in B has x = min(cntA, xmax), 0 when it is not in A, and y = min(cntB, ymax), 0 when
 *              it is not in B.  The counts are the exact 64-bit d_cnt, so a snapshot sorted here may hold counts above
 *              32767.  mat[x*(ymax+1)+y] receives 1 under CP_CMP_KEYS, cntA under CP_CMP_A and cntB under CP_CMP_B, the
 *              count of a side the key is not in being 0.  A key in neither is not counted, so mat[0] is always 0.  Row
 *              xmax and column ymax are the "at least" cells.
 *   Sums       exact in 64 bits (taken modulo 2^64).  `mat` is a HOST array and is overwritten.
 *   Operands   both ready and of the same K; a == b is legal (only cells (min(c, xmax), min(c, ymax)) are non-zero), so
 *              are size 0 (two empty operands give a matrix of zeros) and K < 5.  Both are only read.
 *   Errors     all before any launch: CP_EINVAL for a NULL a, b or mat, an unready operand, differing K, a range with
 *              min < 1 or max < min, a weight outside the enum, xmax or ymax outside [1, 32767], and
 *              (xmax+1)*(ymax+1) > 2^22.  An allocation that fails is CP_ENOMEM with the byte count in the message,
 *              nothing leaked.  Synchronises `stream`.
 *   Memory     16 bytes per tile of cp_ktab_tile() entries of the two operands together, and the matrix; never anything
 *              per entry.
 *   Knobs      read per call from the environment, for measurements and tests: CLASSPRO_CMP_GRID=<n> sets the number of
 *              blocks, clamped to [1, the default]; CLASSPRO_CMP_LDS=0 sends every cell straight to the matrix in device
 *              memory instead of summing the low corner on chip.  Neither changes a result.
 *
 * cp_kmer_qv is Merqury's rule; host only, no device involved.  a_only and a_total are the CP_CMP_A sums over column
 * y = 0 and over the whole matrix: the k-mers of A (an assembly) that B (the reads) does not hold, and all of A's.
 * err = 1 - pow(1 - (double)a_only / a_total, 1.0 / K), qv = -10 * log10(err), and qv = +inf when a_only == 0.  CP_EINVAL
 * for a_total <= 0, a_only < 0, a_only > a_total, K < 1 or a NULL qv or err.
 */
enum { CP_CMP_KEYS = 0, CP_CMP_A = 1, CP_CMP_B = 2 };
int     cp_kmer_sorted_compare_hist(const cp_kmer_sorted *a, const cp_kmer_sorted *b,
                                    const int64_t *range /* host [4]: a_min a_max b_min b_max, or NULL */,
                                    int weight, int xmax, int ymax,
                                    int64_t *mat /* host [(xmax+1)*(ymax+1)], overwritten */, void *stream);
int     cp_kmer_qv(int K, int64_t a_only, int64_t a_total, double *qv, double *err);

/* ------------------------------------------------------------------------------------------
 * Heterozygous pairs of sorted k-mers (tabhet): every key of ONE snapshot paired with the keys that differ from it only at
 * the centre base, and the 2-D histogram of the two counts of such pairs -- the first step of Smudgeplot and of FASTK's
 * PloidyPlot, which gives ploidy and heterozygosity from the reads alone.  The pairing rule for even K is this library's
 * own, chosen to be strand-symmetric.  Everything is in integers and independent of grid, block size and scheduling.
 *
 *   In         a key is IN when lo <= cnt <= hi with the snapshot's own d_cnt; `range` is a HOST array lo hi, NULL means
 *              [1, INT64_MAX].  A key outside the range is treated exactly as if it were absent.
 *   Siblings   positions are 0-based from the first (most significant) base; m = K/2 rounded down and m' = K-1-m (m' = m
 *              for odd K, m-1 for even K).  The candidates of an in key X are the canonical forms (the minimum of a k-mer
 *              and its reverse complement) of X with one base replaced at position m or at position m', X itself and
 *              repeats removed: at most 3 for odd K, at most 6 for even K.  Y is a sibling of X when it is a candidate of X
 *              and is in.  Equivalently some orientation of X and some orientation of Y differ at position m and nowhere
 *              else; the relation is symmetric.  The keys are taken to be canonical, as every table of `kprof -t` is.
 *   Degree     deg(X) = the number of siblings of X, 0 for a key that is not in.
 *   Pair       an unordered {X, Y} of siblings, counted once; UNIQUE when deg(X) = deg(Y) = 1.  For even K a component
 *              need not be a clique: AACA ~ AAAA ~ ACAA at K = 4, but AACA and ACAA are no siblings.
 *   Cell       a counted pair has a = min(cntX, cntY) and b = max(cntX, cntY) of the exact 64-bit d_cnt and adds 1 to
 *              mat[min(a, xmax)*(ymax+1) + min(b, ymax)].  Row 0 and column 0 stay 0.  `unique` non-zero counts the
 *              unique pairs only (Smudgeplot's choice), 0 every pair.  `mat` is a HOST array and is overwritten.
 *   Tally      HOST int64 [CP_HET_WIDTH]: CP_HET_KEYS the in keys, CP_HET_PAIRED the keys with deg >= 1, CP_HET_MULTI
 *              those with deg >= 2, CP_HET_PAIRS all pairs (the sum of the degrees / 2), CP_HET_UNIQUE the unique pairs,
 *              CP_HET_OUT the size of the result under the mode.  The first five do not depend on `unique`.
 *   d_deg      a DEVICE array of `size` bytes, overwritten with the degrees (at most 6).
 *   out        an ordinary ready cp_kmer_sorted of the keys that are members of a counted pair under the mode, ascending,
 *              each with its own count.  It owns its memory and its bucket starts are rebuilt, so every query and
 *              cp_kmer_sorted_combine take it; an empty result has size 0 and null arrays.  To be destroyed by the caller.
 *   Operand    ready, any K a snapshot can have (2..63), any size.  It is only read.  Lookups are those of "Sorted k-mers
 *              as input": clamped ranges, at most 64 probes.
 *   Errors     all before any launch: CP_EINVAL for a NULL s, an unready snapshot, mat, tally, d_deg and out all NULL, a
 *              range with lo < 1 or hi < lo, and -- when mat is given -- xmax or ymax outside [1, 32767] or
 *              (xmax+1)*(ymax+1) > 2^22, and -- when out is given -- a snapshot of more than 2^24 tiles of
 *              cp_ktab_tile() entries.  An allocation that fails is CP_ENOMEM with the byte count in the message,
 *              nothing leaked.  After any error the contents of mat, tally and d_deg are unspecified.  Synchronises
 *              `stream`.
 *   Memory     one byte per entry (none when d_deg is given: it serves as that scratch), the matrix, and with `out` 8
 *              bytes per tile of cp_ktab_tile() entries; then the result itself.
 *   Knobs      read per call from the environment, for measurements and tests: CLASSPRO_HET_LDS=0 sends every cell
 *              straight to the matrix in device memory instead of summing the low corner on chip; CLASSPRO_HET_STAGE=1
 *              (0) selects (deselects) the staged form, in which a block holds its tile of cp_ktab_tile() consecutive
 *              entries on chip and resolves the candidates that fall inside the tile there.  Neither changes a result.
 */
enum { CP_HET_KEYS = 0, CP_HET_PAIRED = 1, CP_HET_MULTI = 2, CP_HET_PAIRS = 3, CP_HET_UNIQUE = 4, CP_HET_OUT = 5, CP_HET_WIDTH = 6 };
int     cp_kmer_sorted_het_pairs(const cp_kmer_sorted *s, const int64_t *range /* host [2]: lo hi, or NULL */,
                                 int unique, int xmax, int ymax,
                                 int64_t *mat /* host [(xmax+1)*(ymax+1)], overwritten, or NULL */,
                                 int64_t *tally /* host [CP_HET_WIDTH], or NULL */,
                                 uint8_t *d_deg /* device [size], overwritten, or NULL */,
                                 void *stream, cp_kmer_sorted **out /* or NULL */);

/* ------------------------------------------------------------------------------------------
 * Phasing heterozygous sites from reads (tabphase): the two members of a unique heterozygous pair are the two alleles of a
 * SITE; reads that carry two sites say whether the smaller k-mers of the two lie on one haplotype or on two; a maximum
 * spanning forest over those votes gives every site a block and a side, and the k-mers split into two marker tables A and
 * B that need no parents.  The definitions are this library's own.  Everything is in integers and nothing depends on grid,
 * block size, batching, read order or scheduling.
 *
 *   Sites      P is a ready snapshot of canonical keys; its counts are not looked at.  Siblings and deg are those of
 *              "Heterozygous pairs of sorted k-mers", taken inside P with no range.  mate[i] is the ordinal of entry i's only
 *              sibling when deg(i) = 1 and that sibling's degree is 1, otherwise -1.  A mated entry is the LOW member when
 *              i < mate[i]; site(i) = the number of low members below min(i, mate[i]), so site ids are dense, 0 .. S-1;
 *              allele(i) is 0 for the low member and 1 for the high one; mark[i] = site << 1 | allele (int32) for a mated
 *              entry, -1 otherwise.  On the result of cp_kmer_sorted_het_pairs(unique = 1, out) every entry is mated: a
 *              second sibling inside P would be a second sibling in the table.  S < 2^30, otherwise CP_EINVAL: a mark is a
 *              non-negative int32.
 *   Markers    a k-mer position of a read is a marker (site, allele) when its key -- chosen as in cp_kmer_sorted_profiles,
 *              by `canonical` -- is in P and that entry is mated.  Every other position is transparent: absent keys,
 *              unmated entries and k-mers holding a byte other than upper-case A C G T, exactly as for the switches of
 *              cp_bin_call.
 *   Links      take the markers of one read in order.  Every adjacent pair (s,a), (s',a') with s != s' is a link with the
 *              key min(s,s') << 32 | max(s,s') << 1 | (a ^ a'), a 63-bit number; a pair with s == s' is counted as `self`
 *              and gives no link.  The links of a batch are emitted in batch order -- reads ascending, positions ascending
 *              -- so the array itself is deterministic.  A marker is never compared across a read boundary.
 *   Edges      after all reads every site pair s < t has cis, the occurrences of the key (s,t,0), and trans, those of
 *              (s,t,1).  With w = max, l = min and margin = w - l an edge is WEAK when w < min_support, otherwise TIED when
 *              margin == 0, otherwise KEPT with sign = (trans > cis).
 *   Forest     kept edge e comes before f when min(margin_e, 65535) > min(margin_f, 65535), or these are equal and
 *              (s_e, t_e) is lexicographically smaller: a strict total order, held by one 64-bit word (the clamped margin in
 *              the top 16 bits, then 2^48-1 minus an ordinal that ascends with (s,t)).  F is the maximum spanning forest
 *              under that order -- Kruskal taking the edges from first to last and adding an edge when it joins two trees.
 *              F is unique.
 *   Blocks     block[s] is the smallest site of s's tree; side[s] is the XOR of the signs along F's path from block[s] to s,
 *              0 for the block's own site.  A site without a kept edge is SINGLE: block[s] = s, side[s] = 0.  A kept edge
 *              with sign != side[s] ^ side[t] is a CONFLICT; it is never in F.
 *   Split      entry i of P goes to table A when it is mated, its site is not SINGLE and side[site] ^ allele == 0, to B
 *              when that value is 1.  Both are ordinary snapshots that keep the entries' own counts, bucket starts rebuilt.
 *   Between    the phase of one block relative to another is arbitrary -- no method that sees only reads can know it.  A
 *   blocks     and B mean something INSIDE a block, which is what the blocks and switches of "Runs of k-mer states" need.
 *
 * cp_kmer_counts_add_keys adds n explicit keys hi << 63 | lo to a count table, +1 each (d_hi NULL: every hi is 0); failed
 * inserts, growth and replay work as for bases.  CP_EINVAL for a filtered table.  A key that does not fit 2K bits or whose
 * lo exceeds 2^63-1 is found on the device: it is left out and counted, the other keys of the call ARE added, and the call
 * returns CP_EINVAL after the pass -- the table is not repaired.  Synchronises.  The links are accumulated in a table of
 * K = 32, whose cp_kmer_counts_sort(t, 1) hands the edges over ascending, cis and trans of a pair adjacent.
 *
 * cp_kmer_sorted_het_sites fills d_mark (int32 [size]) and, when given, d_mate (int64 [size]); *nsites = S; tally (host
 * [2], or NULL) = mated and unmated entries.  CP_EINVAL for a NULL p or nsites, an unready snapshot, a NULL d_mark where
 * there are entries.  Scratch: 8 bytes per entry (16 without d_mate) and 8 per tile.  Synchronises.
 *
 * cp_kmer_sorted_read_links emits the links of a batch.  Capacity, the counting call (d_links NULL, capacity 0) and
 * CP_EOVERFLOW with the exact *total work as in cp_kmer_sorted_read_runs; a call that overflows writes no link and adds
 * nothing to the tally.  d_tally (device int64 [3], or NULL) is ADDED TO: markers, links, self.  Errors before any launch:
 * CP_EINVAL for a NULL p or total, an unready snapshot, negative sizes, null pointers where there is work.  Scratch, by
 * plain allocation: 16 bytes per marker -- the first pass has room for one marker per 64 bases and is repeated once at the
 * exact size when the batch holds more -- 16 bytes per block of 8192 positions and 8 per 256 markers.  Synchronises.
 * Knob, read per call from the environment, for tests: CLASSPRO_PHASE_GUESS=<n> gives the first staging array room for n
 * markers (at least 1) instead of one per 64 bases, so that the repeated pass can be forced.  It changes no result.
 *
 * cp_phase_forest takes the sorted link keys with their counts.  The two counts of a pair are read from adjacent entries; a
 * pair with only one of its keys present has the other count 0.  A key with a bit above 62, with s >= t or with
 * t >= nsites is ignored and counted, per key, in CP_PH_BAD; nothing read from the arrays leads outside an array.  tally
 * (host [CP_PH_WIDTH], or NULL): EDGES the site pairs, KEPT, TIED, WEAK, FOREST the edges of F, CONFLICTS, BLOCKS the trees
 * of two or more sites, SINGLE, LARGEST the sites of the largest block (0 without a block), ROUNDS the Boruvka rounds that
 * joined trees, BAD.  Errors before any launch: CP_EINVAL for a NULL or unready snapshot or one whose K is not 32,
 * min_support < 1, nsites outside [0, 2^31), 2^48 keys or more, a NULL d_block or d_side with nsites > 0.  Scratch: 9 bytes
 * per key and 24 per site.  Synchronises.
 *
 * cp_kmer_sorted_phase_split builds table A (which = 0) or B (which = 1).  It takes nsites, the length of d_block and
 * d_side: whether a site is SINGLE is read from d_block (no other site names it and it names itself), which needs a byte
 * per site.  A mark that names a site >= nsites keeps its entry out.  CP_EINVAL for a NULL p or out, an unready snapshot,
 * which outside {0, 1}, nsites outside [0, 2^31), null pointers where there is work.  The result is the caller's.
 */
enum { CP_PH_EDGES = 0, CP_PH_KEPT = 1, CP_PH_TIED = 2, CP_PH_WEAK = 3, CP_PH_FOREST = 4, CP_PH_CONFLICTS = 5, CP_PH_BLOCKS = 6,
       CP_PH_SINGLE = 7, CP_PH_LARGEST = 8, CP_PH_ROUNDS = 9, CP_PH_BAD = 10, CP_PH_WIDTH = 11 };
int     cp_kmer_counts_add_keys(cp_kmer_counts *t, const uint64_t *d_hi /* or NULL: all zero */, const uint64_t *d_lo,
                                int64_t n, void *stream);
int     cp_kmer_sorted_het_sites(const cp_kmer_sorted *p, int64_t *d_mate /* int64 [size], or NULL */,
                                 int32_t *d_mark /* int32 [size] */, int64_t *nsites /* host */,
                                 int64_t *tally /* host [2]: mated, unmated; or NULL */, void *stream);
int     cp_kmer_sorted_read_links(const cp_kmer_sorted *p, const int32_t *d_mark, int canonical, const char *d_seq,
                                  const int64_t *d_seq_off, int nreads, int64_t total_bases,
                                  uint64_t *d_links /* uint64 [capacity], or NULL */, int64_t capacity,
                                  int64_t *total /* host */, int64_t *d_tally /* device int64 [3], added to; or NULL */,
                                  void *stream);
int     cp_phase_forest(const cp_kmer_sorted *edges, int64_t nsites, int64_t min_support,
                        int64_t *d_block /* int64 [nsites] */, uint8_t *d_side /* uint8 [nsites] */,
                        int64_t *tally /* host [CP_PH_WIDTH], or NULL */, void *stream);
int     cp_kmer_sorted_phase_split(const cp_kmer_sorted *p, const int32_t *d_mark, const int64_t *d_block,
                                   const uint8_t *d_side, int64_t nsites, int which /* 0: A, 1: B */, void *stream,
                                   cp_kmer_sorted **out);

/* ------------------------------------------------------------------------------------------
 * Unitigs of sorted k-mers (tabunitig): the de Bruijn graph that ONE snapshot of canonical k-mers implies -- which k-mers
 * follow which -- and its compaction: the maximal non-branching chains spelled as sequences, what BCALM and GGCAT produce
 * and what every de Bruijn assembler builds on.  The definitions are this library's own.  Everything is in integers and
 * independent of grid, block size and scheduling.
 *
 *   In         a key is IN when lo <= cnt <= hi with the snapshot's own d_cnt; `range` is a HOST array lo hi, NULL means
 *              [1, INT64_MAX].  A key outside the range is treated exactly as if it were absent.  A key is the bases as a
 *              2K-bit number, first base most significant, A C G T = 0 1 2 3; the keys are taken to be canonical.
 *   State      the in entry with ordinal i has two states: 2i spells the key X, 2i+1 spells rc(X); flip(s) = s ^ 1.
 *   Successor  for a state spelling w the successors are the strings w[1:]+c, c in A C G T, whose canonical form is in.
 *              The successor STATE of such a string is 2j when the string equals key j and 2j+1 when it is key j's
 *              reverse complement.  out(s) is the set of such c.  The predecessors of s are the flips of the successors
 *              of flip(s).
 *   d_adj      a DEVICE array of `size` bytes, overwritten: bit c of byte i is set iff c is in out(2i), bit 4+c iff c is in
 *              out(2i+1); 0 for an entry that is not in.  For a palindromic key (X = rc(X), even K) the nibbles are equal.
 *   Link       s -> t exists when out(s) has exactly one member and t is its state, out(flip(t)) has exactly one member
 *              (which is then flip(s)), the node of t is not the node of s (no homopolymer loop t = s, no hairpin
 *              t = flip(s)), and neither node is palindromic.  Every state has at most one link out and one in, and
 *              s -> t exists iff flip(t) -> flip(s) does.
 *   Unitig     a maximal chain of links, taken once for the chain and its mirror image; a chain never meets its own
 *              mirror, so every in key lies in exactly one unitig, exactly once.
 *   Spelling   of a path of n nodes: the first state's K bases, then the last base of each further state, n+K-1 bases.
 *              With h the first state and e the last, the other strand starts at flip(e); the unitig is spelled from the
 *              smaller of the states h and flip(e), that is from the end node with the smaller key; for n = 1 that is
 *              state 2i, the canonical k-mer itself.  A closed chain (CIRCULAR) starts at its smallest node in the forward
 *              state 2i, follows the links once round and is spelled open with n+K-1 bases.
 *   Order      unitigs are numbered by ascending first state: the output is a function of the table and the range alone.
 *   out        a cp_unitigs: count unitigs, d_off[count+1] the offsets of their sequences in d_seq (upper-case A C G T;
 *              bases = d_off[count]; nodes of u = d_off[u+1]-d_off[u]-K+1), d_kc[u] the exact 64-bit sum of the counts of
 *              its nodes, d_flag[u] bit 0 = circular.  All DEVICE arrays owned by the object, null when count = 0.  To be
 *              destroyed by the caller; it keeps no reference to the snapshot.
 *   d_utg d_at DEVICE arrays of `size` int64, overwritten: the unitig of entry i and 2*(its node index within the spelled
 *              unitig) + (1 when the unitig spells the key's reverse complement); both -1 for an entry that is not in.
 *   Tally      HOST int64 [CP_UTG_WIDTH]: CP_UTG_KEYS the in keys, CP_UTG_UNITIGS, CP_UTG_BASES, CP_UTG_CIRCULAR the closed
 *              ones, CP_UTG_LONGEST the longest unitig in bases, CP_UTG_ISOLATED the in keys with adjacency byte 0,
 *              CP_UTG_TIPS those with one empty nibble and one non-empty, CP_UTG_BRANCHING those with a nibble of two or
 *              more bits, CP_UTG_ARCS the sum of the popcounts of all bytes.  Two fields are measurements and the only ones
 *              that may depend on scheduling: CP_UTG_ROUNDS, the jump rounds of the ranking, and CP_UTG_JUMP_NS, the
 *              nanoseconds of the host's clock that those rounds took, each waited for.
 *   Passes     with out, d_utg and d_at all NULL only the adjacency pass runs (tally and/or d_adj); the UNITIGS, BASES,
 *              CIRCULAR, LONGEST, ROUNDS and JUMP_NS fields are then 0.  With d_utg or d_at and no out the chains are ranked and
 *              numbered and no sequence is written.
 *   Operand    ready, any K a snapshot can have (2..63).  It is only read.  Lookups are those of "Sorted k-mers as input":
 *              clamped ranges, at most 64 probes.  An empty table, or one with every key out of range, gives zero unitigs
 *              and null arrays and is no error.
 *   Errors     all before any launch: CP_EINVAL for a NULL s, an unready snapshot, tally, d_adj, d_utg, d_at and out all
 *              NULL, a range with lo < 1 or hi < lo, and -- when unitigs are wanted -- a snapshot of more than 2^30 entries
 *              (a state and a distance share one 64-bit word).  An allocation that fails is CP_ENOMEM with the byte count
 *              in the message, nothing leaked.  After any error the contents of the outputs are unspecified.
 *              Synchronises `stream`.
 *   Memory     the adjacency pass alone: one byte per entry (none when d_adj is given).  With unitigs 33 bytes per entry
 *              beside that byte: a 64-bit ranking word (resolved bit, distance, state) and a 32-bit link per state, a
 *              64-bit ordinal and a head byte per entry; 8 bytes per tile of cp_ktab_tile() entries and per 4096 entries;
 *              32 bytes per state on a closed chain, on the device and on the host, where closed chains are finished;
 *              then the result: bases + 17 bytes per unitig.
 *
 * cp_unitig_n50: host only, no device involved.  The largest L such that the unitigs of at least L bases hold at least half
 * of all bases; 0 for n = 0; CP_EINVAL for n < 0, a NULL len with n > 0 or a negative length.
 */
enum { CP_UTG_KEYS = 0, CP_UTG_UNITIGS = 1, CP_UTG_BASES = 2, CP_UTG_CIRCULAR = 3, CP_UTG_LONGEST = 4, CP_UTG_ISOLATED = 5,
       CP_UTG_TIPS = 6, CP_UTG_BRANCHING = 7, CP_UTG_ARCS = 8, CP_UTG_ROUNDS = 9, CP_UTG_JUMP_NS = 10, CP_UTG_WIDTH = 11 };
typedef struct cp_unitigs cp_unitigs;
int     cp_kmer_sorted_unitigs(const cp_kmer_sorted *s, const int64_t *range /* host [2]: lo hi, or NULL */,
                               int64_t *tally /* host [CP_UTG_WIDTH], or NULL */,
                               uint8_t *d_adj /* device [size], overwritten, or NULL */,
                               int64_t *d_utg, int64_t *d_at /* device [size] each, overwritten, or NULL */,
                               void *stream, cp_unitigs **out /* or NULL */);
/* The getters of a cp_unitigs and of a cp_unitig_graph return host values and device pointers to arrays that are written
 * when the call that made the object has returned: nothing is waited for. */
int64_t cp_unitigs_count(const cp_unitigs *u);
int64_t cp_unitigs_bases(const cp_unitigs *u);
int     cp_unitigs_arrays(const cp_unitigs *u, const char **d_seq, const int64_t **d_off /* [count+1] */,
                          const int64_t **d_kc, const uint8_t **d_flag);
void    cp_unitigs_destroy(cp_unitigs *u);
int64_t cp_unitig_n50(const int64_t *len, int64_t n);

/* ------------------------------------------------------------------------------------------
 * Links between unitigs (tabgraph): which unitig follows which, in which orientation, and the connected components of
 * the graph they form -- the edges that BCALM ships as L:+:id:- header fields and that GFA writes as L lines.  Builds on
 * "Unitigs of sorted k-mers" and uses its words State, out(s), Successor, flip and path.  Everything is in integers and,
 * but for CP_UGL_ROUNDS, independent of grid, block size and scheduling.
 *
 *   Oriented   x = 2u + o: o = 0 ('+') is unitig u as spelled, o = 1 ('-') its reverse complement; x ^ 1 is the other
 *              strand.
 *   Ends       with p[0..n-1] the states of u's spelled path: end(2u) = p[n-1], end(2u+1) = flip(p[0]) and
 *              start(x) = flip(end(x ^ 1)), so start(2u) = p[0] and start(2u+1) = flip(p[n-1]).  For a one-node unitig
 *              with path [s] the two starts are s and flip(s).
 *   Arc        x -> y with base c exists iff c is in out(end(x)) and the successor state of that string is start(y).
 *              Every successor state of an end state is the start of exactly one oriented unitig (this follows from
 *              Link): with the successor state t = 2j + b and r = d_at[j] & 1, y = 2 * d_utg[j] + (b ^ r); the node index
 *              d_at[j] >> 1 is 0 when b == r and n-1 otherwise.  The overlap of every arc is K-1 bases.
 *   Hence      a circular unitig has exactly the two arcs 2u -> 2u and 2u+1 -> 2u+1.  A homopolymer node has self arcs, a
 *              hairpin gives 2u -> 2u+1.  A palindromic node is a one-node unitig spelled in state 2i: both orientations
 *              carry the same out-arcs and every arc into it lands on '+'.  Off palindromic nodes x -> y exists iff
 *              y^1 -> x^1 does.  LINKS == CP_UTG_ARCS - 2 * (CP_UTG_KEYS - CP_UTG_UNITIGS).
 *   Order      arcs are sorted by source x ascending, then by c ascending: a function of the table and the range alone.
 *   Component  comp[u] is the smallest unitig ordinal in u's connected component, arcs taken as undirected and
 *              orientation ignored.
 *   Arguments  `range` is the one given to cp_kmer_sorted_unitigs; u, d_utg and d_at are the object and the where arrays
 *              of THAT call on THIS snapshot (device, `size` int64 each).  Arrays of another call give unspecified arcs
 *              but never an access outside the arrays: a unitig read from them is clamped to [0, count).  The snapshot,
 *              u and the two arrays are only read.
 *   out        a cp_unitig_graph: d_loff[2*count+1] the offsets of the arcs of every oriented unitig, d_link[links] the
 *              target y and d_base[links] the base c (0..3) of every arc, d_comp[count] the components (null without
 *              want_comp).  DEVICE arrays owned by the object, all null when count = 0 (zero unitigs give zero links and
 *              are no error), d_link and d_base also when links = 0.  To be destroyed by the caller; it keeps no
 *              reference to the snapshot or to u.
 *   Tally      HOST int64 [CP_UGL_WIDTH]: CP_UGL_LINKS; CP_UGL_DEAD_ENDS the oriented unitigs without an arc;
 *              CP_UGL_TIP_UNITIGS the unitigs with exactly one of their two orientations dead; CP_UGL_ISOLATED_UNITIGS
 *              those with both dead; CP_UGL_SELF the arcs whose target unitig is the source's; CP_UGL_COMPONENTS and
 *              CP_UGL_LARGEST_BASES, the largest sum of unitig bases over a component, both 0 without want_comp;
 *              CP_UGL_ROUNDS, a measurement and the only field that may depend on scheduling: the label rounds, the
 *              last, which changes nothing, included (0 without want_comp or without links).
 *   Passes     one lane per oriented unitig reads the K bases at its end and makes its four look-ups, one search after
 *              the other, by the bounded search of "Sorted k-mers as input": 8 look-ups per unitig, not per k-mer.  The
 *              components are label rounds -- a 64-bit atomic minimum of agent scope per arc, then every label replaced
 *              by its label's label to a fixed point -- until a round lowers nothing, at most count rounds and no
 *              smaller cap; the result is the component's minimum whatever the scheduling (kmer_unitig_graph.hip).
 *   Errors     all before any launch: CP_EINVAL for a NULL s or u, NULL d_utg or d_at with count > 0, an unready
 *              snapshot, a u whose K differs from the snapshot's, a range with lo < 1 or hi < lo, tally and out both
 *              NULL.  An allocation that fails is CP_ENOMEM with the byte count in the message, nothing leaked.  A given
 *              `out` is cleared on every error.  Synchronises `stream`.
 *   Memory     scratch: 64 bytes per unitig (four staged targets per orientation), 8 more with want_comp, 8 bytes per
 *              4096 oriented unitigs and under 200 bytes of counters.  Result: 16 bytes per unitig + 8, 9 bytes per link, and 8
 *              bytes per unitig with want_comp.
 */
enum { CP_UGL_LINKS = 0, CP_UGL_DEAD_ENDS = 1, CP_UGL_TIP_UNITIGS = 2, CP_UGL_ISOLATED_UNITIGS = 3, CP_UGL_SELF = 4,
       CP_UGL_COMPONENTS = 5, CP_UGL_LARGEST_BASES = 6, CP_UGL_ROUNDS = 7, CP_UGL_WIDTH = 8 };
typedef struct cp_unitig_graph cp_unitig_graph;
int     cp_kmer_sorted_unitig_links(const cp_kmer_sorted *s, const int64_t *range /* host [2] or NULL, the one given to _unitigs */,
                                    const cp_unitigs *u, const int64_t *d_utg, const int64_t *d_at /* device [size], of the call that made u */,
                                    int64_t *tally /* host [CP_UGL_WIDTH], or NULL */, int want_comp,
                                    void *stream, cp_unitig_graph **out /* or NULL */);
int64_t cp_unitig_graph_links(const cp_unitig_graph *g);
int     cp_unitig_graph_arrays(const cp_unitig_graph *g, const int64_t **d_loff /* [2*count+1] */, const int64_t **d_link /* [links]: y */,
                               const uint8_t **d_base /* [links]: c */, const int64_t **d_comp /* [count], null without want_comp */);
void    cp_unitig_graph_destroy(cp_unitig_graph *g);

/* ------------------------------------------------------------------------------------------
 * Reads through the unitig graph (tabpath): the k-mer positions of a batch in the flat layout above, looked up in ONE
 * snapshot and located in its unitigs, reduced on the device to the stretches that run along one oriented unitig -- which
 * way a read or a contig runs through the compacted de Bruijn graph, the read coverage of every unitig and the read
 * support of every arc.  Builds on "Unitigs of sorted k-mers" and "Links between unitigs" and uses their words State,
 * Link, Oriented, Ends and Arc.  Only the segments come down, never a value per base.  Every key is rolled once and looked
 * up once.  Everything is in integers.
 *
 *   Step       of k-mer position i of a read (k-mer i covers the bases [i, i+K)), with w the forward k-mer and
 *              X = min(w, rc(w)): OTHER when w holds a byte other than upper-case A C G T; ABSENT when X is not found, or is
 *              found at entry e with d_utg[e] < 0 -- an entry outside the range given to cp_kmer_sorted_unitigs is absent
 *              in this way, so this call needs no range of its own; otherwise the step is (x, q): with b = (w != X),
 *              u = d_utg[e], k = d_at[e] >> 1, r = d_at[e] & 1 and n the nodes of u, x = 2u + (b ^ r), and q = k when
 *              b == r, else n-1-k.  q is the place of the position in the oriented unitig x.  A palindromic key has b = 0.
 *   Segment    a maximal stretch of consecutive positions of one read, with no position between them, whose steps are
 *              (x, q), (x, q+1), ...  Its record: `first` the ordinal in the read of its first position, `n` the number
 *              of its positions, `x`, `q` of the first position, `read` the read's index in the batch, `flags`.  Bit 0 of
 *              flags (CP_PATH_JOINED_FLAG) is JOINED: the position first-1 of the same read is a step as well.  A closed unitig run
 *              round twice gives two segments, the second joined (the self arc 2u -> 2u); nothing is special-cased.
 *   Joins      a joined segment follows a segment that ends at the last place of its unitig, starts at place 0, and the arc
 *              x_prev -> x whose base is the read's base at first+K-1 exists: this follows from Link and Arc.
 *   Spelling   read[first : first+n+K-1] equals the sequence of the oriented unitig x at [q : q+n+K-1].
 *   Mirror     the segments of rc(read) are those of the read in reverse order with first' = nk-first-n (nk the k-mer
 *              positions of the read), q' = nodes-q-n and x' = x ^ 1, but x' = x for the one-node unitig of a palindromic
 *              key.
 *   Walk       a maximal chain of a read's segments in which every segment but the first is joined (host side: GAF).
 *   Output     d_seg_off[r] .. d_seg_off[r+1] are the records of read r in d_segs, ascending in `first`; all nreads+1
 *              offsets are overwritten, and *total (HOST) = d_seg_off[nreads].  Reads shorter than K, empty reads and
 *              nreads == 0 give no segments and are no error.  n and q fit 32 bits, because unitigs exist only for
 *              snapshots of at most 2^30 entries.
 *   Capacity   d_segs holds `capacity` records.  With *total > capacity the call returns CP_EOVERFLOW; d_seg_off, *total and
 *              the tally are exact all the same, the records below `capacity` are written and nothing beyond them is
 *              touched.  d_segs == NULL with capacity == 0 is the counting call.
 *   Sums       d_cov[u] += n per segment of unitig u; d_support[a] += 1 per joined segment, a the arc in
 *              d_loff[x_prev] .. d_loff[x_prev+1] of g whose base is the read's.  Both are ADDED TO, so a caller
 *              accumulates over batches, and only by a call that returns CP_OK: a call that overflows adds nothing, so the
 *              call that is made again at the exact size does not add twice.  Exact 64-bit integer sums, independent of
 *              batching, read order, grid and scheduling.  d_support counts the direction the reads were given in; the
 *              strand-free support of an edge is its own plus its mirror arc's.
 *   Tally      HOST int64 [CP_PATH_WIDTH], overwritten: CP_PATH_POSITIONS the k-mer positions, CP_PATH_PRESENT those that
 *              are steps, CP_PATH_ABSENT, CP_PATH_OTHER, CP_PATH_SEGMENTS (= *total), CP_PATH_JOINED, CP_PATH_WALKS
 *              (= SEGMENTS - JOINED).
 *   Fixed      the records of a read are a function of the read, the snapshot and the unitigs alone: not of what else is in
 *              the batch, of the order of the reads, or of the grid, block and chunk sizes of the kernels.
 *   Arguments  u, d_utg and d_at are the object and the where arrays (device, `size` int64 each) of ONE call of
 *              cp_kmer_sorted_unitigs on THIS snapshot, g the graph made from them (or NULL; needed for d_support).  Where
 *              arrays or a g of another call give unspecified records and sums but never an access outside an array: a
 *              unitig, an oriented unitig and an arc read from them are clamped.  Everything passed in is only read, but
 *              d_cov (`count` int64) and d_support (`links` int64).
 *   Errors     all before any launch: CP_EINVAL for a NULL s, u or total, an unready snapshot, a u of another K, NULL where
 *              arrays with count > 0, d_support without g, a negative nreads, total_bases or capacity, a null device pointer
 *              where there is work (d_segs with capacity > 0, d_seg_off and d_seq_off with nreads > 0, d_seq with
 *              total_bases > 0).
 *   Memory     scratch of 8 bytes per base of the batch, 32 bytes per 16384 bases and 64 bytes more, allocated and freed in
 *              stream order per call; when that fails it is CP_ENOMEM with the byte count in the message.  Nothing is
 *              queued on `stream` before that allocation has succeeded.
 *   Cost       one pass of lookups that stores a 64-bit word per base, and two passes over those words.  Reads without a
 *              k-mer position are serialised in single lanes as in "Runs of k-mer states along reads".  One 64-bit atomic
 *              per segment: reads that pile on one repeat unitig add to one address.
 * Synchronises `stream`: the total must be known to return it.
 *
 * cp_count_nonzero: *count (HOST) = the number of values of the DEVICE array d_v[0..n) that are not zero -- the unitigs
 * touched of a d_cov, the arcs crossed of a d_support -- so that only the number comes down.  CP_EINVAL for a NULL count,
 * n < 0 or a NULL d_v with n > 0.  Synchronises `stream`.
 */
enum { CP_PATH_POSITIONS = 0, CP_PATH_PRESENT = 1, CP_PATH_ABSENT = 2, CP_PATH_OTHER = 3, CP_PATH_SEGMENTS = 4,
       CP_PATH_JOINED = 5, CP_PATH_WALKS = 6, CP_PATH_WIDTH = 7 };
enum { CP_PATH_JOINED_FLAG = 1 };
typedef struct cp_path_seg { int64_t first, x; int32_t n, q, read, flags; } cp_path_seg;   /* 32 bytes */
int     cp_kmer_sorted_read_paths(const cp_kmer_sorted *s, const cp_unitigs *u,
                                  const int64_t *d_utg, const int64_t *d_at /* device [size], of the call that made u */,
                                  const cp_unitig_graph *g /* or NULL; needed for d_support */,
                                  const char *d_seq, const int64_t *d_seq_off, int nreads, int64_t total_bases,
                                  cp_path_seg *d_segs /* device [capacity], or NULL */, int64_t capacity,
                                  int64_t *d_seg_off /* device [nreads+1], overwritten */,
                                  int64_t *d_cov /* device [count], added to, or NULL */,
                                  int64_t *d_support /* device [links], added to, or NULL */,
                                  int64_t *tally /* host [CP_PATH_WIDTH], or NULL */, int64_t *total /* host */, void *stream);
int     cp_count_nonzero(const int64_t *d_v, int64_t n, int64_t *count /* host */, void *stream);

/* ------------------------------------------------------------------------------------------
 * Pruning the unitig graph (tabclean): the structural cleaning that every de Bruijn tool chain makes after compaction --
 * short dead-end branches clipped, simple bubbles popped, short islands dropped -- as marks per unitig and as the snapshot
 * without the k-mers of the marked unitigs, an ordinary cp_kmer_sorted that every other call takes.  Builds on "Unitigs of
 * sorted k-mers" and "Links between unitigs" and uses their words Oriented and Arc.  Everything is in integers.  Every mark
 * is a function of the input graph of ONE call alone, never of another mark of that call, so the result is independent of
 * grid, block size and scheduling.
 *
 *   Words      for an oriented unitig x: deg(x) = d_loff[x+1] - d_loff[x], T(x) the targets d_link[d_loff[x] .. d_loff[x+1]).
 *              For a unitig u: bases(u) = d_off[u+1] - d_off[u], nodes(u) = bases(u) - K + 1, circ(u) bit 0 of d_flag[u],
 *              w(u) its weight: d_weight[u] when d_weight is given, else d_kc[u]; a negative weight counts as 0.
 *   Limits     a HOST array max_island, max_tip, max_bubble, in bases; 0 switches a rule off.
 *   why[u]     0 kept, 1 island, 2 tip, 3 bubble.  The three cases exclude each other by their degrees.
 *   Island     deg(2u) == 0, deg(2u+1) == 0 and bases(u) <= max_island.
 *   TC(u)      a tip CANDIDATE: exactly one of deg(2u), deg(2u+1) is 0 and bases(u) <= max_tip.  x is then the orientation of
 *              u that has arcs: it walks from the dead end into the graph.
 *   Tip        TC(u), and there is an arc x -> y with y >> 1 != u and an arc y^1 -> t such that v = (t^1) >> 1 satisfies
 *              v != u and v BEATS u: !TC(v), or (nodes(v), w(v)) > (nodes(u), w(u)) lexicographically, or the pairs are
 *              equal and v < u.  v is another unitig that enters the junction u enters.  A tip with no competitor at its
 *              junction stays; among competing candidates at one junction the order is strict and total, so the best stays.
 *   Bubble     the ARM condition: !circ(u), deg(2u) == 1, deg(2u+1) == 1, bases(u) <= max_bubble, and with y = T(2u)[0] and
 *              t = T(2u+1)[0] neither y >> 1 nor t >> 1 is u.  With p = t^1, every z in T(p) (at most 4) names v = z >> 1,
 *              an ALTERNATIVE when v != u, !circ(v), bases(v) <= max_bubble, deg(z) == 1, T(z)[0] == y, deg(z^1) == 1 and
 *              T(z^1)[0] == t.  u goes when some alternative v has w(v) * nodes(u) > w(u) * nodes(v), or the products are
 *              equal and v < u; the products are exact (128 bits: a weight may reach 2^62, nodes 2^30).  The arm of highest
 *              mean weight always stays.
 *   As it is   the rule is written on d_loff and d_link as they are: nothing is special-cased at palindromic nodes, hairpins
 *              or self arcs (a closed chain, a homopolymer node, a hairpin and a palindromic node all stay).
 *   Limit      a bubble whose other side is split by a further junction is not simple and is not popped: that is what two
 *              error sites closer than K give.  A caller's rounds (tabclean, SortedKmers.clean) resolve what other removals
 *              uncover; two interleaved bubbles stay.
 *   d_why      a DEVICE array of `count` bytes, overwritten with why[u].
 *   out        a ready cp_kmer_sorted of the entries with d_utg[i] >= 0 and why[d_utg[i]] == 0, with their own counts, in
 *              ascending order, its bucket starts rebuilt: cp_kmer_sorted_ktab, _find, _profiles, _combine and _unitigs work
 *              on it.  An entry outside the range of the unitigs call (d_utg[i] < 0) is not in it.  To be destroyed by the
 *              caller; it keeps no reference to anything passed in.
 *   Tally      HOST int64 [CP_PRUNE_WIDTH]: CP_PRUNE_UNITIGS the unitigs looked at, CP_PRUNE_ISLANDS, CP_PRUNE_TIPS and
 *              CP_PRUNE_BUBBLES those marked, CP_PRUNE_REMOVED_BASES their bases, CP_PRUNE_REMOVED_KEYS the entries of
 *              marked unitigs, CP_PRUNE_KEPT_KEYS the entries of `out`.  KEPT_KEYS + REMOVED_KEYS == CP_UTG_KEYS of the call
 *              that made u.
 *   Arguments  u and d_utg are the object and the where array (device, `size` int64) of ONE call of cp_kmer_sorted_unitigs on
 *              THIS snapshot, g the graph made from them, d_weight `count` int64 on the device.  Arrays of another call give
 *              unspecified marks but never an access outside an array: a unitig, an oriented unitig and an offset read from
 *              them are clamped.  Everything passed in is only read.
 *   Passes     one lane per unitig applies the rule, its loads issued in groups (kn_rule.h); one pass over the entries
 *              turns d_utg and why into tile counts; the scan; a pass that writes the kept entries (neither when out is
 *              NULL; the pass over the entries only when tally or out is given).  The sums are taken per wave before any
 *              atomic.
 *   Errors     all before any launch: CP_EINVAL for a NULL s, u, g or limits, an unready snapshot, a u of another K, a g of
 *              another number of unitigs, a NULL d_utg with count > 0, a negative limit, d_why, tally and out all NULL.  An
 *              allocation that fails is CP_ENOMEM with the byte count in the message, nothing leaked.  A given `out` is
 *              cleared on every error.  Zero unitigs give an empty `out` and are no error.  Synchronises `stream`.
 *   Memory     scratch: 8 bytes per tile of cp_ktab_tile() entries, 8 bytes per 4096 tiles or buckets, 64 bytes of counters
 *              and one byte per unitig (none when d_why is given).  Result: 24 bytes per kept entry and 8 per bucket.
 */
enum { CP_PRUNE_UNITIGS, CP_PRUNE_ISLANDS, CP_PRUNE_TIPS, CP_PRUNE_BUBBLES, CP_PRUNE_REMOVED_KEYS,
       CP_PRUNE_REMOVED_BASES, CP_PRUNE_KEPT_KEYS, CP_PRUNE_WIDTH };
int     cp_kmer_sorted_unitig_prune(const cp_kmer_sorted *s, const cp_unitigs *u,
                                    const int64_t *d_utg /* device [size], of the call that made u */, const cp_unitig_graph *g,
                                    const int64_t *d_weight /* device [count] or NULL: d_kc */, const int64_t *limits /* host [3] */,
                                    uint8_t *d_why /* device [count], overwritten, or NULL */, int64_t *tally /* host, or NULL */,
                                    void *stream, cp_kmer_sorted **out /* or NULL */);

/* ------------------------------------------------------------------------------------------
 * Global-threshold labels (ClassGS): replaces the per-read loop of src/ClassGS.c:228-248, the GenomeScope-style
 * baseline the reference compares ClassPro against, for a batch in the flat layout above.
 *
 *   Label     of a count c: E if c < thres[0], else H if c < thres[1], else D if c < thres[2], else R.  This is the
 *             reference's chain, so unsorted thresholds have a defined result (with 30 10 50 no k-mer is H).  Any
 *             int32_t value is legal (the host clamps to [0, 65536]); counts are the full uint16_t range.
 *   Read r    gets 'N' on its first min(K-1, rlen_r) positions, then one label per count.  Unlike cp_classify_batch,
 *             reads shorter than K are allowed: they have no counts (prof_off[r+1] = prof_off[r]) and get only 'N'.
 *   Outputs   each optional (NULL = not wanted, at least one required):
 *             d_labels  [total_bases]  the characters;
 *             d_packed  + d_pack_off [nreads+1]: the 2-bit layout of cp_pack_labels, written directly;
 *             d_counts  int64 [4] on the device, order E, H, D, R, ADDED TO, so several batches accumulate.
 * Offsets are 64-bit throughout: a batch may hold more than 2^31 bases.  Asynchronous on `stream`.
 */
int cp_threshold_labels(int K, const int32_t *thres, const uint16_t *d_prof, const int64_t *d_prof_off,
                        const int64_t *d_seq_off, int nreads, int64_t total_bases, char *d_labels,
                        uint8_t *d_packed, const int64_t *d_pack_off, int64_t *d_counts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Label accuracy: replaces the counting of src/class2acc.c:141-316 (default report) for an estimate and a truth label
 * string that are already on the device, both in the layout of `labels` above.  An accumulator, so batches add up.
 *
 *   Per read  over positions i >= K-1: rtot = rlen-(K-1), rcor = equal labels, rfne = truth E and estimate not E,
 *             rcomp[4] = truth composition.  Reads with rlen < K contribute nothing.
 *   cfm       [truth][estimate], order E, R, H, D as class2acc prints it (its stoc); counts every read.
 *   Filter    a read with (double)rcomp[E]/rtot*100 > max_e_pct (class2acc -f, default 100) is left out of all nine
 *             totals and counted in n_reads_filtered.  Otherwise it goes to "repeat" when
 *             (double)rcomp[R]/rtot*100 > rep_pct (-r, default 0), else to "normal".  The device evaluates exactly
 *             these double expressions (divide, then multiply, no contraction), so the decisions are the host tool's.
 *   Invalid   a character other than E H D R at a position >= K-1 of either string is tallied in n_invalid, counted
 *             nowhere else, and makes every later cp_acc_read return CP_EINVAL (deferred; `stats` is still filled).
 * All sums are integers: the result is the same bit for bit whatever the batching or the read order.
 */
typedef struct cp_acc cp_acc;
typedef struct
  { int64_t cfm[4][4];
    int64_t ntot, ncor, nfne;                            /* reads that passed the filter */
    int64_t ntot_normal, ncor_normal, nfne_normal;
    int64_t ntot_repeat, ncor_repeat, nfne_repeat;
    int64_t n_reads, n_reads_filtered, n_invalid;
  } cp_acc_stats;
int  cp_acc_create(int K, double max_e_pct, double rep_pct, cp_acc **out);
void cp_acc_destroy(cp_acc *a);
/* Asynchronous on `stream`. */
int  cp_acc_add(cp_acc *a, const char *d_est, const char *d_truth, const int64_t *d_seq_off, int nreads,
                int64_t total_bases, void *stream);
/* Waits for the stream of the last cp_acc_add on `a` (the null stream before the first), then reads the totals back. */
int  cp_acc_read(cp_acc *a, cp_acc_stats *out);

#ifdef __cplusplus
}
#endif
#endif

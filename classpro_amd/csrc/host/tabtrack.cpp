// tabtrack.cpp -- WHERE along the sequences of a source the k-mers of one or two FASTK k-mer tables lie: the runs of k-mer
// states of "Runs of k-mer states along reads" (include/classpro_amd.h), reduced on the device; only the runs come down.
//
//   tabtrack [-v] [-m<int(1)>] [-b<int(67108864)>] [-o<out_root>]
//            <A>[.ktab][:<lo>-<hi>] [<B>[.ktab][:<lo>-<hi>]] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// ONE table, the absence track: where the k-mers of a sequence are that the table does not hold.  With the table of the
// reads (`kprof -t`) and an assembly as the source that is the QV of every contig and the intervals the reads do not
// support, what Merqury writes next to its QV; with the reads themselves as the source (`:2-`) the runs are the sequencing
// errors, about K positions per substitution.  One line per sequence on stdout, in source order, tab-separated:
//   <ordinal from 1> <length> <valid k-mers> <missing k-mers> <missing runs> <QV> <the .class header without its '@'>
// valid = k-mers of upper-case A C G T, missing = those of them not in the table, QV = cp_kmer_qv(K, missing, valid) as
// %.4f, "inf" when nothing is missing and "-" without a valid k-mer.  And one line on stderr:
//   tabtrack: <n> sequences, <k> k-mers, <m> missing in <r> runs, QV <qv>          k the valid k-mers, QV over them all
// -o writes <out_root>.missing.bed: <name> <first> <last+K> <n> per missing run, first and last the ordinals of the run's
// first and last k-mer, so that [first, last+K) are its bases; <name> is the header up to its first blank.
//
// TWO tables, phase blocks: A and B are two marker sets (hap-mers of tabop), positions with a key in neither or in both
// and positions with other bytes are transparent, and the runs of A and B markers are taken.  Per sequence the blocks are
// cp_run_blocks(runs, -m): runs of fewer than -m markers are dropped, neighbours of equal side merged.  This rule is this
// project's own, not Merqury's, which tolerates switches within a distance.  One line per sequence:
//   <ordinal> <length> <nA> <nB> <runs> <dropped runs> <blocks> <bases in blocks> <header>
// bases in blocks = the sum of last+K-first.  With -m1, runs - 1 is tabbin's `switches`.  And one line on stderr:
//   tabtrack: <n> sequences, <a> A and <b> B markers, <r> runs, <d> dropped, <k> blocks, block N50 <x>
// x = the largest span s such that the blocks of span >= s hold at least half of all block bases, 0 without blocks.
// -o writes <out_root>.blocks.bed: <name> <first> <last+K> <A|B> <n> per block.
//
//   :<lo>-<hi>  the count range of an operand, as tabop takes it (ktab_range.h).
//   -m  the least number of markers of a run that is kept (two tables only).
//   -b  bases per device batch, whole sequences per batch: a batch goes out once it holds that many bases.
//   -v  one more line on stderr: the entries of the tables, bases, batches, runs brought down.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabtrack <usage line>                                                  wrong number of arguments
//   tabtrack: -<c> is an illegal option
//   tabtrack: -<c> '<text>' argument is not an integer
//   tabtrack: Minimum number of markers must be positive (<n>)                    -m below 1
//   tabtrack: Bases per device batch must be positive (<n>)                       -b below 1
//   tabtrack: -m needs two tables                                                 -m with one table
//   tabtrack: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    either table
//   tabtrack: K of <A stub> (<k>) and <B stub> (<k>) differ
//   tabtrack: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file           the source
//   tabtrack: Cannot open <path> for 'w'                                          the file of -o
#include <algorithm>
#include <cmath>
#include "gpu_tool.h"
#include "read_source.h"
#include "ktab_upload.h"
#include "ktab_range.h"

static const char *USAGE = "[-v] [-m<int(1)>] [-b<int(67108864)>] [-o<out_root>]\n"
                           "                <A>[.ktab][:<lo>-<hi>] [<B>[.ktab][:<lo>-<hi>]] <source>[.db|.dam|.f[ast][aq][.gz]]";

struct Batch
  { std::vector<std::string> headers;
    std::vector<char> seq;
    std::vector<int64_t> soff{0};
    void clear() { headers.clear(); seq.clear(); soff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

static void print_qv(FILE *f, int K, int64_t missing, int64_t valid)
{ if (valid <= 0) { fputc('-',f); return; }
  double qv, err;
  const int rc = cp_kmer_qv(K,missing,valid,&qv,&err);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_qv");
  fprintf(f,"%.4f",qv);
}

int main(int argc, char **argv)
{ PROG = "tabtrack";
  bool verbose = false, have_m = false;
  int min_n = 1, batch_bases = 64 << 20;
  std::string out_root;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-')
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'm': min_n = arg_int(a,"Minimum number of markers",true); have_m = true; break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'o': out_root = a+2; break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2 && pos.size() != 3)
    die("Usage: %s %s\n",PROG,USAGE);
  const bool two = pos.size() == 3;
  if (have_m && !two) die("%s: -m needs two tables\n",PROG);
  int64_t range[4] = { 1, INT64_MAX, 1, INT64_MAX };
  const std::string name_a = split_range(pos[0],range);
  std::string name_b;
  if (two) name_b = split_range(pos[1],range+2);
  KtabReader A, B;
  A.open(name_a);
  if (two)
    { B.open(name_b);
      if (A.K != B.K) die("%s: K of %s (%d) and %s (%d) differ\n",PROG,A.stub.c_str(),A.K,B.stub.c_str(),B.K);
    }
  const int K = A.K;
  Source S;
  std::string dir, root;
  if (!S.find(pos.back(),&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos.back().c_str());
  FILE *bed = nullptr;
  const std::string bed_path = out_root+(two ? ".blocks.bed" : ".missing.bed");
  if (!out_root.empty() && !(bed = fopen(bed_path.c_str(),"w")))
    die("%s: Cannot open %s for 'w'\n",PROG,bed_path.c_str());
  S.open();

  // ---- the tables up ----
  HCHK(hipSetDevice(0));
  cp_kmer_sorted *TA, *TB = nullptr;
  { DevBuf<uint8_t> d_rec;
    TA = upload_ktab(A,d_rec);
    if (two) TB = upload_ktab(B,d_rec);
    d_rec.release();
  }
  const unsigned int skip = two ? (1u << CP_RUN_NONE) | (1u << CP_RUN_BOTH) | (1u << CP_RUN_OTHER) : 0u;
  const unsigned int emit = 0x1fu & ~skip;

  // ---- the sequences ----
  DevBuf<char> d_seq;
  DevBuf<int64_t> d_soff, d_roff;
  DevBuf<cp_kmer_run> d_runs;
  std::vector<int64_t> h_roff, spans;
  std::vector<cp_kmer_run> h_runs, blocks;
  std::vector<char> obuf((size_t)1 << 20);
  setvbuf(stdout,obuf.data(),_IOFBF,obuf.size());
  Batch R;
  int64_t nseqs = 0, nbases = 0, nbatches = 0, ndown = 0;
  int64_t nvalid = 0, nmissing = 0, nmruns = 0;            // one table
  int64_t tot_a = 0, tot_b = 0, nruns = 0, ndropped = 0, nblocks = 0, block_bases = 0;   // two tables
  auto flush = [&]()
    { const int n = R.n();
      if (n == 0) return;
      const int64_t bases = R.soff.back();
      d_seq.need(R.seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,R.seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(R.soff);
      d_roff.need((size_t)n+1);
      d_runs.need(std::max<size_t>(1024,(size_t)(bases/16)));         // a guess: a run per 16 bases
      int64_t total = 0;
      int rc = cp_kmer_sorted_read_runs(TA,TB,1,range,skip,emit,d_seq.p,d_soff.p,n,bases,d_runs.p,(int64_t)d_runs.cap,d_roff.p,
                                        &total,nullptr);
      if (rc == CP_EOVERFLOW)                              // the total is exact: once more at that size
        { d_runs.need((size_t)total);
          rc = cp_kmer_sorted_read_runs(TA,TB,1,range,skip,emit,d_seq.p,d_soff.p,n,bases,d_runs.p,(int64_t)d_runs.cap,d_roff.p,
                                        &total,nullptr);
        }
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_read_runs");
      h_roff.resize((size_t)n+1);
      h_runs.resize((size_t)total);
      HCHK(hipMemcpy(h_roff.data(),d_roff.p,((size_t)n+1)*sizeof(int64_t),hipMemcpyDeviceToHost));
      if (total > 0) HCHK(hipMemcpy(h_runs.data(),d_runs.p,(size_t)total*sizeof(cp_kmer_run),hipMemcpyDeviceToHost));
      ndown += total;
      for (int r = 0; r < n; r++)
        { const int64_t len = R.soff[(size_t)r+1]-R.soff[(size_t)r];
          const char *header = R.headers[(size_t)r].c_str()+(R.headers[(size_t)r].empty() ? 0 : 1);
          const int name_len = (int)strcspn(header," \t");
          const cp_kmer_run *run = h_runs.data()+h_roff[(size_t)r];
          const int64_t nr = h_roff[(size_t)r+1]-h_roff[(size_t)r];
          const long long ordinal = (long long)(nseqs-n+r+1);
          if (!two)
            { int64_t valid = 0, missing = 0, mruns = 0;
              for (int64_t i = 0; i < nr; i++)
                { if (run[i].state != CP_RUN_OTHER) valid += run[i].n;
                  if (run[i].state != CP_RUN_NONE) continue;
                  missing += run[i].n;
                  mruns++;
                  if (bed)
                    fprintf(bed,"%.*s\t%lld\t%lld\t%lld\n",name_len,header,(long long)run[i].first,(long long)(run[i].last+K),
                            (long long)run[i].n);
                }
              printf("%lld\t%lld\t%lld\t%lld\t%lld\t",ordinal,(long long)len,(long long)valid,(long long)missing,(long long)mruns);
              print_qv(stdout,K,missing,valid);
              printf("\t%s\n",header);
              nvalid += valid; nmissing += missing; nmruns += mruns;
              continue;
            }
          int64_t na = 0, nb = 0, dropped = 0, bb = 0;
          for (int64_t i = 0; i < nr; i++) (run[i].state == CP_RUN_A ? na : nb) += run[i].n;
          blocks.resize((size_t)nr+1);
          const int64_t nblk = cp_run_blocks(nr ? run : blocks.data(),nr,min_n,blocks.data(),&dropped);
          if (nblk < 0) cp_die((int)nblk,"cp_run_blocks");
          for (int64_t i = 0; i < nblk; i++)
            { const int64_t span = blocks[(size_t)i].last+K-blocks[(size_t)i].first;
              bb += span;
              spans.push_back(span);
              if (bed)
                fprintf(bed,"%.*s\t%lld\t%lld\t%c\t%lld\n",name_len,header,(long long)blocks[(size_t)i].first,
                        (long long)(blocks[(size_t)i].last+K),blocks[(size_t)i].state == CP_RUN_A ? 'A' : 'B',
                        (long long)blocks[(size_t)i].n);
            }
          printf("%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%s\n",ordinal,(long long)len,(long long)na,(long long)nb,
                 (long long)nr,(long long)dropped,(long long)nblk,(long long)bb,header);
          tot_a += na; tot_b += nb; nruns += nr; ndropped += dropped; nblocks += nblk; block_bases += bb;
        }
      nbatches++;
      R.clear();
    };
  while (S.next())
    { const int64_t rlen = (int64_t)S.seq.size();
      R.headers.push_back(S.header);
      R.seq.insert(R.seq.end(),S.seq.begin(),S.seq.end());
      R.soff.push_back(R.soff.back()+rlen);
      nseqs++;
      nbases += rlen;
      if (R.soff.back() >= batch_bases || R.n() == INT32_MAX) flush();
    }
  flush();
  fflush(stdout);
  if (ferror(stdout)) die("%s: Cannot write the standard output\n",PROG);
  if (bed && fclose(bed) != 0) die("%s: Cannot write %s\n",PROG,bed_path.c_str());

  if (!two)
    { fprintf(stderr,"%s: %lld sequences, %lld k-mers, %lld missing in %lld runs, QV ",PROG,(long long)nseqs,(long long)nvalid,
              (long long)nmissing,(long long)nmruns);
      print_qv(stderr,K,nmissing,nvalid);
      fputc('\n',stderr);
    }
  else
    { std::sort(spans.begin(),spans.end(),[](int64_t x, int64_t y) { return x > y; });
      int64_t n50 = 0, held = 0;
      for (const int64_t s : spans)
        { held += s;
          if (2*(unsigned __int128)held >= (unsigned __int128)block_bases) { n50 = s; break; }
        }
      fprintf(stderr,"%s: %lld sequences, %lld A and %lld B markers, %lld runs, %lld dropped, %lld blocks, block N50 %lld\n",PROG,
              (long long)nseqs,(long long)tot_a,(long long)tot_b,(long long)nruns,(long long)ndropped,(long long)nblocks,
              (long long)n50);
    }
  if (verbose)
    { if (two)
        fprintf(stderr,"A %lld entries, B %lld entries, %lld bases, %lld batches, %lld runs brought down\n",(long long)A.entries,
                (long long)B.entries,(long long)nbases,(long long)nbatches,(long long)ndown);
      else
        fprintf(stderr,"A %lld entries, %lld bases, %lld batches, %lld runs brought down\n",(long long)A.entries,(long long)nbases,
                (long long)nbatches,(long long)ndown);
    }
  cp_kmer_sorted_destroy(TA);
  if (TB) cp_kmer_sorted_destroy(TB);
  return 0;
}

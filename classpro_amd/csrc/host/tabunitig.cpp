// tabunitig.cpp -- the unitigs of the de Bruijn graph of one FASTK k-mer table: which canonical k-mers follow which, and
// the maximal non-branching chains of that graph spelled as sequences, on the GPU -- the compacted graph that BCALM and
// GGCAT produce.
//
//   tabunitig [-v] <table>[.ktab][:<lo>-<hi>] [<out_root>]
//
// Prints one line on stdout, always, and nothing else there:
//   tabunitig: <keys> k-mers, <u> unitigs, <bases> bases, <c> circular, longest <L>, N50 <n>
// the k-mers in range, their unitigs, the bases of all sequences, the closed chains, the longest sequence and the N50 of
// the sequences (cp_kmer_sorted_unitigs, cp_unitig_n50; "Unitigs of sorted k-mers" in include/classpro_amd.h).  With
// <out_root> writes <out_root>.unitigs.fa: per unitig, in the library's order, the header
//   ><ordinal> LN:i:<bases> KC:i:<count sum>[ CL:Z:circular]
// and the sequence on one line.  The sequences, count sums and flags come down in ranges through buffers of a fixed size;
// the offsets (8 bytes per unitig) are held whole, because the N50 needs every length.  Without <out_root> no file is
// created.  The output is created before the GPU is touched, so that a name that cannot be written costs no GPU work; a
// failure on the device after that leaves it behind, empty.  The table may be FastK's own, a Logex product, `kprof -t`, a
// class table of class2ktab or a tabop result; its k-mers are taken to be canonical.
//   :<lo>-<hi>  the count range, exactly as tabop takes it: k-mers outside it count as absent.
//   -v  one line on stderr: K, the entries of the table, tips, branching and isolated k-mers, the jump rounds of the
//       ranking and the seconds of the device call.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabunitig <usage line>                                                 wrong number of arguments
//   tabunitig: -<c> is an illegal option
//   tabunitig: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    the table
//   tabunitig: Cannot open <path> for 'w'                                         <out_root>.unitigs.fa
#include <chrono>
#include "gpu_tool.h"
#include "ktab_upload.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] <table>[.ktab][:<lo>-<hi>] [<out_root>]";
static const int64_t SEQ_BUF = 1 << 24;    // bases held on the host at a time
static const int64_t UTG_BUF = 1 << 20;    // count sums and flags held on the host at a time

int main(int argc, char **argv)
{ PROG = "tabunitig";
  bool verbose = false;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-' && a[1] != '\0')                         // a bare "-" is an operand like any other name
        for (int k = 1; a[k]; k++)
          { if (a[k] == 'v') verbose = true;
            else die("%s: -%c is an illegal option\n",PROG,a[k]);
          }
      else
        pos.push_back(a);
    }
  if (pos.size() != 1 && pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  int64_t range[2];
  const std::string name = split_range(pos[0],range);
  KtabReader A;
  A.open(name);
  const int K = A.K;

  // the output is created before the GPU is touched
  FILE *fa = nullptr;
  std::string fa_path;
  if (pos.size() == 2)
    { fa_path = path_to(pos[1])+"/"+root_of(pos[1],"")+".unitigs.fa";
      const bool fresh = access(fa_path.c_str(),F_OK) != 0;
      const int fd = open(fa_path.c_str(),O_WRONLY|O_CREAT,0666);
      if (fd >= 0 && (ftruncate(fd,0) != 0 || !(fa = fdopen(fd,"wb")))) close(fd);
      if (!fa)
        { if (fd >= 0 && fresh) unlink(fa_path.c_str());
          die("%s: Cannot open %s for 'w'\n",PROG,fa_path.c_str());
        }
    }

  // ---- the table up, then the graph ----
  HCHK(hipSetDevice(0));
  cp_kmer_sorted *T;
  { DevBuf<uint8_t> d_rec;
    T = upload_ktab(A,d_rec);
    d_rec.release();
  }
  int64_t tally[CP_UTG_WIDTH];
  cp_unitigs *U = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = cp_kmer_sorted_unitigs(T,range,tally,nullptr,nullptr,nullptr,nullptr,&U);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitigs");
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now()-t0).count();
  cp_kmer_sorted_destroy(T);

  const int64_t count = cp_unitigs_count(U);
  const char *d_seq;
  const int64_t *d_off, *d_kc;
  const uint8_t *d_flag;
  if (cp_unitigs_arrays(U,&d_seq,&d_off,&d_kc,&d_flag) != CP_OK) cp_die(CP_EINVAL,"cp_unitigs_arrays");
  std::vector<int64_t> off((size_t)count+1,0), len((size_t)count);
  if (count > 0) HCHK(hipMemcpy(off.data(),d_off,(size_t)(count+1)*8,hipMemcpyDeviceToHost));
  for (int64_t u = 0; u < count; u++) len[(size_t)u] = off[(size_t)u+1]-off[(size_t)u];
  const int64_t n50 = cp_unitig_n50(len.data(),count);
  if (n50 < 0) cp_die((int)n50,"cp_unitig_n50");
  printf("%s: %lld k-mers, %lld unitigs, %lld bases, %lld circular, longest %lld, N50 %lld\n",PROG,(long long)tally[CP_UTG_KEYS],
         (long long)tally[CP_UTG_UNITIGS],(long long)tally[CP_UTG_BASES],(long long)tally[CP_UTG_CIRCULAR],
         (long long)tally[CP_UTG_LONGEST],(long long)n50);
  fflush(stdout);

  if (fa)
    { std::vector<char> seq((size_t)SEQ_BUF);
      std::vector<int64_t> kc((size_t)UTG_BUF);
      std::vector<uint8_t> flag((size_t)UTG_BUF);
      int64_t have0 = 0, have1 = 0;                            // seq holds the bases [have0, have1)
      bool ok = true;
      for (int64_t u0 = 0; u0 < count; u0 += UTG_BUF)
        { const int64_t nu = std::min(UTG_BUF,count-u0);
          HCHK(hipMemcpy(kc.data(),d_kc+u0,(size_t)nu*8,hipMemcpyDeviceToHost));
          HCHK(hipMemcpy(flag.data(),d_flag+u0,(size_t)nu,hipMemcpyDeviceToHost));
          for (int64_t u = u0; u < u0+nu; u++)
            { ok = fprintf(fa,">%lld LN:i:%lld KC:i:%lld%s\n",(long long)u,(long long)len[(size_t)u],(long long)kc[(size_t)(u-u0)],
                           (flag[(size_t)(u-u0)] & 1) ? " CL:Z:circular" : "") > 0 && ok;
              for (int64_t p = off[(size_t)u]; p < off[(size_t)u+1]; )
                { if (p >= have1)                              // the next range of bases, from p on
                    { have0 = p;
                      have1 = std::min(p+SEQ_BUF,off[(size_t)count]);
                      HCHK(hipMemcpy(seq.data(),d_seq+have0,(size_t)(have1-have0),hipMemcpyDeviceToHost));
                    }
                  const int64_t e = std::min(have1,off[(size_t)u+1]);
                  ok = fwrite(seq.data()+(p-have0),1,(size_t)(e-p),fa) == (size_t)(e-p) && ok;
                  p = e;
                }
              ok = fputc('\n',fa) != EOF && ok;
            }
        }
      if (fclose(fa) != 0 || !ok) die("%s: Cannot write %s\n",PROG,fa_path.c_str());
    }
  cp_unitigs_destroy(U);
  if (verbose)
    fprintf(stderr,"K %d: %lld entries; %lld tips, %lld branching, %lld isolated; %lld jump rounds; %.3f s on the device\n",K,
            (long long)A.entries,(long long)tally[CP_UTG_TIPS],(long long)tally[CP_UTG_BRANCHING],
            (long long)tally[CP_UTG_ISOLATED],(long long)tally[CP_UTG_ROUNDS],secs);
  return 0;
}

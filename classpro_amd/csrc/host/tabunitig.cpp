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
#include "tab_out.h"
#include "unitig_dump.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] <table>[.ktab][:<lo>-<hi>] [<out_root>]";

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
  Outputs outs;
  FILE *fa = nullptr;
  std::string fa_path;
  if (pos.size() == 2)
    { fa_path = path_to(pos[1])+"/"+root_of(pos[1],"")+".unitigs.fa";
      fa = outs.create(fa_path);
    }

  // ---- the table up, then the graph ----
  cp_kmer_sorted *T = upload_table(A);
  int64_t tally[CP_UTG_WIDTH];
  cp_unitigs *U = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = cp_kmer_sorted_unitigs(T,range,tally,nullptr,nullptr,nullptr,nullptr,&U);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitigs");
  const double secs = since(t0);
  cp_kmer_sorted_destroy(T);

  std::vector<int64_t> off, len;
  unitig_lengths(U,off,len);
  print_unitig_line(len,tally);
  fflush(stdout);

  if (fa)
    { const bool ok = write_unitig_fasta(fa,U,off);
      if (fclose(fa) != 0 || !ok) die("%s: Cannot write %s\n",PROG,fa_path.c_str());
    }
  cp_unitigs_destroy(U);
  if (verbose)
    fprintf(stderr,"K %d: %lld entries; %lld tips, %lld branching, %lld isolated; %lld jump rounds; %.3f s on the device\n",K,
            (long long)A.entries,(long long)tally[CP_UTG_TIPS],(long long)tally[CP_UTG_BRANCHING],
            (long long)tally[CP_UTG_ISOLATED],(long long)tally[CP_UTG_ROUNDS],secs);
  return 0;
}

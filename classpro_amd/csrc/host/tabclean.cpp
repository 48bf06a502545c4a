// tabclean.cpp -- structural cleaning of the de Bruijn graph of one FASTK k-mer table, on the GPU: short dead-end branches
// clipped, simple bubbles popped, short islands dropped, in rounds, and the k-mers that are left as a table of their own --
// the step every de Bruijn tool chain makes after compaction, which a count range cannot stand in for.
//
//   tabclean [-v] [-i<int(0)>] [-t<int(2K)>] [-b<int(0)>] [-r<int(10)>] [-T<int(4)>] <table>[.ktab][:<lo>-<hi>] [<out_root>]
//
// A round is cp_kmer_sorted_unitigs (where arrays), cp_kmer_sorted_unitig_links (no components) and
// cp_kmer_sorted_unitig_prune ("Pruning the unitig graph" in include/classpro_amd.h).  Round 1 takes the count range; the
// later rounds run on the previous result with no range.  The loop ends after a round that removes nothing, or after -r
// rounds.  Prints on stdout, always, and nothing else there:
//   tabclean: <keys> k-mers, <u> unitigs, <bases> bases, <c> circular, longest <L>, N50 <n>      tabunitig's line, the input graph
//   tabclean: round <r>: <u> unitigs, <i> islands, <t> tips, <b> bubbles, <k> k-mers removed      per round
//   tabclean: <keys> k-mers, <u> unitigs, <bases> bases, <c> circular, longest <L>, N50 <n>      the graph of the result
//   tabclean: <in> k-mers in, <out> out, <r> rounds
// With <out_root> writes <out_root>.ktab with its parts and <out_root>.hist in kprof's layout (ktab_writer.h), as tabop does;
// the stub's minval is the input's.  Without it no file is created.  The table may be FastK's own, a Logex product,
// `kprof -t`, a class table of class2ktab or a tabop result; its k-mers are taken to be canonical.
//   :<lo>-<hi>  the count range, exactly as tabop takes it: k-mers outside it count as absent and are not in the result.
//   -i  islands: a unitig with no arc of at most so many bases goes (0: none).
//   -t  tips: a dead-end unitig of at most so many bases goes when a better branch enters its junction (0: none; 2K).
//   -b  bubbles: of the arms of at most so many bases between one pair of junctions only the one of highest mean count
//       stays (0: none, the default, because the arms of a heterozygous site are the H k-mers this project labels).
//   -r  rounds at most.
//   -T  table parts of the result.
//   -v  one line on stderr per round with the wall seconds of its three library calls (allocations and waits included), and
//       one with K, the entries and the parts.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabclean <usage line>                                                  wrong number of arguments
//   tabclean: -<c> is an illegal option
//   tabclean: -<c> '<text>' argument is not an integer
//   tabclean: Island limit must be non-negative (<n>)                              -i; Tip limit, Bubble limit: -t, -b
//   tabclean: Number of rounds must be positive (<n>)                              -r
//   tabclean: Number of threads must be positive (<n>)                             -T
//   tabclean: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    the table
//   tabclean: <out_root>.ktab is the operand: the result needs a name of its own
//   tabclean: Cannot open <path> for 'w'                                          <out_root>.ktab, <out_root>.hist
#include "tab_out.h"
#include "unitig_dump.h"                   // print_unitig_line: tabunitig's line
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] [-i<int(0)>] [-t<int(2K)>] [-b<int(0)>] [-r<int(10)>] [-T<int(4)>]\n"
                           "                <table>[.ktab][:<lo>-<hi>] [<out_root>]";

int main(int argc, char **argv)
{ PROG = "tabclean";
  bool verbose = false;
  int nthreads = 4, islands = 0, tips = -1, bubbles = 0, rounds = 10;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-' && a[1] != '\0')                         // a bare "-" is an operand like any other name
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'i': islands = arg_int(a,"Island limit",false); break;
          case 't': tips = arg_int(a,"Tip limit",false); break;
          case 'b': bubbles = arg_int(a,"Bubble limit",false); break;
          case 'r': rounds = arg_int(a,"Number of rounds",true); break;
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
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
  const bool build = pos.size() == 2;
  const int64_t limits[3] = { islands, tips < 0 ? 2*K : tips, bubbles };

  // the stub and the histogram: both are created before the GPU is touched, or neither is left behind
  std::string odir, oname, tab_path, hist_path;
  Outputs outs;
  FILE *ft = nullptr, *fh = nullptr;
  if (build)
    { odir = path_to(pos[1]);
      oname = root_of(pos[1],"");
      tab_path = odir+"/"+oname+".ktab";
      hist_path = odir+"/"+oname+".hist";
      die_if_operand(tab_path,A.stub,"is the operand");
      ft = outs.create(tab_path);
      fh = outs.create(hist_path);
    }

  // ---- the table up, then the rounds ----
  cp_kmer_sorted *T = upload_table(A);
  DevBuf<int64_t> d_utg, d_at;
  int64_t keys_in = 0, done = 0, removed = 1;
  for (int r = 0; r < rounds && removed > 0; r++)
    { const int64_t size = cp_kmer_sorted_size(T);
      d_utg.need((size_t)size+1);
      d_at.need((size_t)size+1);
      int64_t ut[CP_UTG_WIDTH], pt[CP_PRUNE_WIDTH];
      cp_unitigs *U = nullptr;
      cp_unitig_graph *G = nullptr;
      cp_kmer_sorted *R = nullptr;
      const int64_t *rng = r == 0 ? range : nullptr;
      const auto t0 = std::chrono::steady_clock::now();
      int rc = cp_kmer_sorted_unitigs(T,rng,ut,nullptr,size ? d_utg.p : nullptr,size ? d_at.p : nullptr,nullptr,&U);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitigs");
      rc = cp_kmer_sorted_unitig_links(T,rng,U,d_utg.p,d_at.p,nullptr,0,nullptr,&G);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitig_links");
      rc = cp_kmer_sorted_unitig_prune(T,U,d_utg.p,G,nullptr,limits,nullptr,pt,nullptr,&R);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitig_prune");
      const double secs = since(t0);
      if (r == 0)
        { print_unitig_line(U,ut);
          keys_in = ut[CP_UTG_KEYS];
        }
      printf("%s: round %d: %lld unitigs, %lld islands, %lld tips, %lld bubbles, %lld k-mers removed\n",PROG,r+1,
             (long long)pt[CP_PRUNE_UNITIGS],(long long)pt[CP_PRUNE_ISLANDS],(long long)pt[CP_PRUNE_TIPS],
             (long long)pt[CP_PRUNE_BUBBLES],(long long)pt[CP_PRUNE_REMOVED_KEYS]);
      if (verbose) fprintf(stderr,"round %d: %lld entries; %.3f s wall\n",r+1,(long long)size,secs);
      removed = pt[CP_PRUNE_REMOVED_KEYS];
      done = r+1;
      if (removed == 0) print_unitig_line(U,ut);                      // the result's graph is this round's
      cp_unitig_graph_destroy(G);
      cp_unitigs_destroy(U);
      cp_kmer_sorted_destroy(T);
      T = R;
    }
  if (removed > 0)                                             // the rounds ran out: the graph of the result is not known yet
    { int64_t ut[CP_UTG_WIDTH];
      cp_unitigs *U = nullptr;
      const int rc = cp_kmer_sorted_unitigs(T,nullptr,ut,nullptr,nullptr,nullptr,nullptr,&U);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitigs");
      print_unitig_line(U,ut);
      cp_unitigs_destroy(U);
    }
  d_utg.release();
  d_at.release();
  const int64_t keys_out = cp_kmer_sorted_size(T);
  printf("%s: %lld k-mers in, %lld out, %lld rounds\n",PROG,(long long)keys_in,(long long)keys_out,(long long)done);
  fflush(stdout);

  int nparts = 0;
  if (build)
    { std::vector<int64_t> hist((size_t)CP_MAX_KMER_CNT);
      int64_t ilow, ihigh;
      const int rc = cp_kmer_sorted_hist(T,hist.data(),&ilow,&ihigh);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_hist");
      write_hist(fh,hist_path,K,ilow,ihigh,hist.data());
      KtabWriter W;
      W.write(T,K,A.minval,nthreads,ft,tab_path,odir,oname);
      W.release();
      nparts = W.nparts;
    }
  cp_kmer_sorted_destroy(T);
  if (verbose)
    fprintf(stderr,"K %d: %lld entries, minval %d, %d parts; result %lld entries, %d parts\n",K,(long long)A.entries,A.minval,
            A.nparts,(long long)keys_out,nparts);
  return 0;
}

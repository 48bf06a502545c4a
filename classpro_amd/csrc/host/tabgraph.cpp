// tabgraph.cpp -- the compacted de Bruijn graph of one FASTK k-mer table as a GFA file: the unitigs that tabunitig spells,
// which of them follows which and in which orientation, and the connected components of that graph, on the GPU -- what
// Bandage, the GFA tool chain and bubble or tip analysis read.
//
//   tabgraph [-v] <table>[.ktab][:<lo>-<hi>] <out_root>
//
// Prints two lines on stdout, always, and nothing else there:
//   tabgraph: <keys> k-mers, <u> unitigs, <bases> bases, <c> circular, longest <L>, N50 <n>
//   tabgraph: <links> links, <dead> dead ends, <tips> tip unitigs, <comps> components, largest <bases> bases
// the first is tabunitig's line (cp_kmer_sorted_unitigs, cp_unitig_n50), the second the tally of
// cp_kmer_sorted_unitig_links ("Links between unitigs" in include/classpro_amd.h): the arcs between oriented unitigs, the
// oriented unitigs without one, the unitigs with exactly one such orientation, the connected components and the bases of
// the unitigs of the largest.  Writes <out_root>.gfa, in this order:
//   H\tVN:Z:1.0
//   S\t<u>\t<sequence>\tLN:i:<bases>\tKC:i:<count sum>\tco:i:<component>        per unitig, in the library's order
//   L\t<u>\t<+|->\t<v>\t<+|->\t<K-1>M                                           per arc, in the library's order
// Both arcs of a mirror pair are written, as BCALM's converter does; a circular unitig shows through its two self links.
// The sequences, count sums, components and links come down in ranges through buffers of a fixed size; the offsets (8
// bytes per unitig) are held whole, because the N50 needs every length.  The output is created before the GPU is
// touched, so that a name that cannot be written costs no GPU work; a failure on the device after that leaves it behind,
// empty.  The table and the range are tabunitig's.
//   -v  one line on stderr: tabunitig's, then the label rounds of the components and the seconds of the link pass and of
//       the component pass (the link pass is run once more on its own to time it).
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabgraph <usage line>                                                  wrong number of arguments
//   tabgraph: -<c> is an illegal option
//   tabgraph: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    the table
//   tabgraph: Cannot open <path> for 'w'                                          <out_root>.gfa
#include "tab_out.h"
#include "unitig_dump.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] <table>[.ktab][:<lo>-<hi>] <out_root>";

int main(int argc, char **argv)
{ PROG = "tabgraph";
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
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  int64_t range[2];
  const std::string name = split_range(pos[0],range);
  KtabReader A;
  A.open(name);
  const int K = A.K;

  // the output is created before the GPU is touched
  const std::string gfa_path = path_to(pos[1])+"/"+root_of(pos[1],"")+".gfa";
  Outputs outs;
  FILE *gfa = outs.create(gfa_path);

  // ---- the table up, then the unitigs, then their links ----
  cp_kmer_sorted *T = upload_table(A);
  const int64_t size = cp_kmer_sorted_size(T);
  DevBuf<int64_t> d_utg, d_at;
  d_utg.need((size_t)size+1);
  d_at.need((size_t)size+1);
  int64_t tally[CP_UTG_WIDTH], lt[CP_UGL_WIDTH];
  cp_unitigs *U = nullptr;
  cp_unitig_graph *G = nullptr;
  auto t0 = std::chrono::steady_clock::now();
  int rc = cp_kmer_sorted_unitigs(T,range,tally,nullptr,size ? d_utg.p : nullptr,size ? d_at.p : nullptr,nullptr,&U);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitigs");
  const double secs = since(t0);
  double link_secs = 0;
  if (verbose)                                                 // the link pass alone, only to time it
    { t0 = std::chrono::steady_clock::now();
      rc = cp_kmer_sorted_unitig_links(T,range,U,d_utg.p,d_at.p,lt,0,nullptr,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitig_links");
      link_secs = since(t0);
    }
  t0 = std::chrono::steady_clock::now();
  rc = cp_kmer_sorted_unitig_links(T,range,U,d_utg.p,d_at.p,lt,1,nullptr,&G);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitig_links");
  const double comp_secs = std::max(since(t0)-link_secs,0.0);
  cp_kmer_sorted_destroy(T);
  d_utg.release();
  d_at.release();

  std::vector<int64_t> off, len;
  unitig_lengths(U,off,len);
  print_unitig_line(len,tally);
  printf("%s: %lld links, %lld dead ends, %lld tip unitigs, %lld components, largest %lld bases\n",PROG,(long long)lt[CP_UGL_LINKS],
         (long long)lt[CP_UGL_DEAD_ENDS],(long long)lt[CP_UGL_TIP_UNITIGS],(long long)lt[CP_UGL_COMPONENTS],
         (long long)lt[CP_UGL_LARGEST_BASES]);
  fflush(stdout);

  const bool ok = write_gfa(gfa,U,G,K,off,nullptr,nullptr);
  if (fclose(gfa) != 0 || !ok) die("%s: Cannot write %s\n",PROG,gfa_path.c_str());
  cp_unitig_graph_destroy(G);
  cp_unitigs_destroy(U);
  if (verbose)
    fprintf(stderr,"K %d: %lld entries; %lld tips, %lld branching, %lld isolated; %lld jump rounds; %.3f s on the device; "
                   "%lld label rounds; %.3f s links, %.3f s components\n",K,(long long)A.entries,(long long)tally[CP_UTG_TIPS],
            (long long)tally[CP_UTG_BRANCHING],(long long)tally[CP_UTG_ISOLATED],(long long)tally[CP_UTG_ROUNDS],secs,
            (long long)lt[CP_UGL_ROUNDS],link_secs,comp_secs);
  return 0;
}

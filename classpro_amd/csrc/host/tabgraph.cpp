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
#include <chrono>
#include "gpu_tool.h"
#include "ktab_upload.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] <table>[.ktab][:<lo>-<hi>] <out_root>";
static const int64_t SEQ_BUF = 1 << 24;    // bases held on the host at a time
static const int64_t UTG_BUF = 1 << 20;    // unitigs whose count sums, components and link offsets are held at a time
static const int64_t LNK_BUF = 1 << 22;    // links held on the host at a time

static double since(std::chrono::steady_clock::time_point t0)
{ return std::chrono::duration<double>(std::chrono::steady_clock::now()-t0).count(); }

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
  FILE *gfa = nullptr;
  { const bool fresh = access(gfa_path.c_str(),F_OK) != 0;
    const int fd = open(gfa_path.c_str(),O_WRONLY|O_CREAT,0666);
    if (fd >= 0 && (ftruncate(fd,0) != 0 || !(gfa = fdopen(fd,"wb")))) close(fd);
    if (!gfa)
      { if (fd >= 0 && fresh) unlink(gfa_path.c_str());
        die("%s: Cannot open %s for 'w'\n",PROG,gfa_path.c_str());
      }
  }

  // ---- the table up, then the unitigs, then their links ----
  HCHK(hipSetDevice(0));
  cp_kmer_sorted *T;
  { DevBuf<uint8_t> d_rec;
    T = upload_ktab(A,d_rec);
    d_rec.release();
  }
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

  const int64_t count = cp_unitigs_count(U), links = cp_unitig_graph_links(G);
  const char *d_seq;
  const int64_t *d_off, *d_kc, *d_loff, *d_link, *d_comp;
  const uint8_t *d_flag;
  if (cp_unitigs_arrays(U,&d_seq,&d_off,&d_kc,&d_flag) != CP_OK) cp_die(CP_EINVAL,"cp_unitigs_arrays");
  if (cp_unitig_graph_arrays(G,&d_loff,&d_link,nullptr,&d_comp) != CP_OK) cp_die(CP_EINVAL,"cp_unitig_graph_arrays");
  std::vector<int64_t> off((size_t)count+1,0), len((size_t)count);
  if (count > 0) HCHK(hipMemcpy(off.data(),d_off,(size_t)(count+1)*8,hipMemcpyDeviceToHost));
  for (int64_t u = 0; u < count; u++) len[(size_t)u] = off[(size_t)u+1]-off[(size_t)u];
  const int64_t n50 = cp_unitig_n50(len.data(),count);
  if (n50 < 0) cp_die((int)n50,"cp_unitig_n50");
  printf("%s: %lld k-mers, %lld unitigs, %lld bases, %lld circular, longest %lld, N50 %lld\n",PROG,(long long)tally[CP_UTG_KEYS],
         (long long)tally[CP_UTG_UNITIGS],(long long)tally[CP_UTG_BASES],(long long)tally[CP_UTG_CIRCULAR],
         (long long)tally[CP_UTG_LONGEST],(long long)n50);
  printf("%s: %lld links, %lld dead ends, %lld tip unitigs, %lld components, largest %lld bases\n",PROG,(long long)lt[CP_UGL_LINKS],
         (long long)lt[CP_UGL_DEAD_ENDS],(long long)lt[CP_UGL_TIP_UNITIGS],(long long)lt[CP_UGL_COMPONENTS],
         (long long)lt[CP_UGL_LARGEST_BASES]);
  fflush(stdout);

  bool ok = fputs("H\tVN:Z:1.0\n",gfa) != EOF;
  { std::vector<char> seq((size_t)SEQ_BUF);
    std::vector<int64_t> kc((size_t)UTG_BUF), comp((size_t)UTG_BUF);
    int64_t have0 = 0, have1 = 0;                              // seq holds the bases [have0, have1)
    for (int64_t u0 = 0; u0 < count; u0 += UTG_BUF)
      { const int64_t nu = std::min(UTG_BUF,count-u0);
        HCHK(hipMemcpy(kc.data(),d_kc+u0,(size_t)nu*8,hipMemcpyDeviceToHost));
        HCHK(hipMemcpy(comp.data(),d_comp+u0,(size_t)nu*8,hipMemcpyDeviceToHost));
        for (int64_t u = u0; u < u0+nu; u++)
          { ok = fprintf(gfa,"S\t%lld\t",(long long)u) > 0 && ok;
            for (int64_t p = off[(size_t)u]; p < off[(size_t)u+1]; )
              { if (p >= have1)                                // the next range of bases, from p on
                  { have0 = p;
                    have1 = std::min(p+SEQ_BUF,off[(size_t)count]);
                    HCHK(hipMemcpy(seq.data(),d_seq+have0,(size_t)(have1-have0),hipMemcpyDeviceToHost));
                  }
                const int64_t e = std::min(have1,off[(size_t)u+1]);
                ok = fwrite(seq.data()+(p-have0),1,(size_t)(e-p),gfa) == (size_t)(e-p) && ok;
                p = e;
              }
            ok = fprintf(gfa,"\tLN:i:%lld\tKC:i:%lld\tco:i:%lld\n",(long long)len[(size_t)u],(long long)kc[(size_t)(u-u0)],
                         (long long)comp[(size_t)(u-u0)]) > 0 && ok;
          }
      }
  }
  { std::vector<int64_t> loff((size_t)2*UTG_BUF+1), link((size_t)LNK_BUF);
    int64_t have0 = 0, have1 = 0;                              // link holds the links [have0, have1)
    for (int64_t u0 = 0; u0 < count; u0 += UTG_BUF)
      { const int64_t nu = std::min(UTG_BUF,count-u0);
        HCHK(hipMemcpy(loff.data(),d_loff+2*u0,(size_t)(2*nu+1)*8,hipMemcpyDeviceToHost));
        for (int64_t x = 2*u0; x < 2*(u0+nu); x++)
          for (int64_t k = loff[(size_t)(x-2*u0)]; k < loff[(size_t)(x-2*u0)+1] && k < links; k++)
            { if (k >= have1)                                  // the next range of links, from k on
                { have0 = k;
                  have1 = std::min(k+LNK_BUF,links);
                  HCHK(hipMemcpy(link.data(),d_link+have0,(size_t)(have1-have0)*8,hipMemcpyDeviceToHost));
                }
              const int64_t y = link[(size_t)(k-have0)];
              ok = fprintf(gfa,"L\t%lld\t%c\t%lld\t%c\t%dM\n",(long long)(x >> 1),(x & 1) ? '-' : '+',(long long)(y >> 1),
                           (y & 1) ? '-' : '+',K-1) > 0 && ok;
            }
      }
  }
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

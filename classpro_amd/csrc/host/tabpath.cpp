// tabpath.cpp -- which way the sequences of a source run through the compacted de Bruijn graph of one FASTK k-mer table:
// the segments of "Reads through the unitig graph" (include/classpro_amd.h), reduced on the device, chained to walks on the
// host and written as GAF; the read coverage of every unitig and the read support of every arc, as tags of tabgraph's GFA.
//
//   tabpath [-v] [-g] [-b<int(67108864)>] [-o<out_root>] <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// The table is loaded, its unitigs made with the range and the where arrays (cp_kmer_sorted_unitigs), their links found
// (cp_kmer_sorted_unitig_links), and the source run through cp_kmer_sorted_read_paths in batches of whole sequences.
// Prints two lines on stdout, always, and nothing else there:
//   tabpath: <keys> k-mers, <u> unitigs, <bases> bases, <c> circular, longest <L>, N50 <n>
//   tabpath: <reads> sequences, <positions> k-mers, <present> on the graph, <segments> segments, <walks> walks,
//            <t> of <u> unitigs touched, <c> of <links> links crossed                                  (one line)
// the first is tabunitig's line; touched = unitigs with coverage, crossed = arcs with support, both counted on the device.
// -o writes <out_root>.gaf, one line per walk in source order, tab-separated:
//   <name> <length> <first> <end> + <path> <path length> <q> <q+end-first> <end-first> <end-first> 255
// <name> is the header up to its first blank, as tabtrack's BED names it; [first, end) are the bases of the sequence that
// the walk covers, end = first+n+K-1 of its last segment; <path> is >u or <u per segment; path length is the sum of the
// unitigs' bases less K-1 per join; q is the place of the first segment, which in bases is where the walk starts on the path.
//   -g  (needs -o) also writes <out_root>.gfa: tabgraph's file with RC:i:<coverage> appended to every S line and
//       RC:i:<support> to every L line.  Support counts the direction the sequences were given in.
//   :<lo>-<hi>  the count range of the table, as tabunitig takes it (ktab_range.h).
//   -b  bases per device batch, whole sequences per batch: a batch goes out once it holds that many bases.
//   -v  one more line on stderr: entries, bases, batches, segments brought down and the seconds on the device.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabpath <usage line>                                                   wrong number of arguments
//   tabpath: -<c> is an illegal option
//   tabpath: -<c> '<text>' argument is not an integer
//   tabpath: Bases per device batch must be positive (<n>)                        -b below 1
//   tabpath: -g needs -o
//   tabpath: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    the table
//   tabpath: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file            the source
//   tabpath: Cannot open <path> for 'w'                                           <out_root>.gaf, <out_root>.gfa
#include <algorithm>
#include "tab_out.h"
#include "unitig_dump.h"
#include "read_source.h"
#include "ktab_range.h"

static const char *USAGE = "[-v] [-g] [-b<int(67108864)>] [-o<out_root>] <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]";

struct Batch
  { std::vector<std::string> headers;
    std::vector<char> seq;
    std::vector<int64_t> soff{0};
    void clear() { headers.clear(); seq.clear(); soff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

int main(int argc, char **argv)
{ PROG = "tabpath";
  bool verbose = false, want_gfa = false;
  int batch_bases = 64 << 20;
  std::string out_root;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-' && a[1] != '\0')
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else if (a[k] == 'g') want_gfa = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'o': out_root = a+2; break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  if (want_gfa && out_root.empty()) die("%s: -g needs -o\n",PROG);
  int64_t range[2];
  const std::string name = split_range(pos[0],range);
  KtabReader A;
  A.open(name);
  const int K = A.K;
  Source S;
  std::string dir, root;
  if (!S.find(pos[1],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[1].c_str());
  S.open();

  // the outputs are created before the GPU is touched
  Outputs outs;
  const std::string gaf_path = out_root+".gaf", gfa_path = out_root+".gfa";
  FILE *gaf = out_root.empty() ? nullptr : outs.create(gaf_path), *gfa = want_gfa ? outs.create(gfa_path) : nullptr;
  std::vector<char> gbuf((size_t)1 << 20);
  if (gaf) setvbuf(gaf,gbuf.data(),_IOFBF,gbuf.size());

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
  rc = cp_kmer_sorted_unitig_links(T,range,U,d_utg.p,d_at.p,lt,want_gfa ? 1 : 0,nullptr,&G);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_unitig_links");
  const double graph_secs = since(t0);

  const int64_t count = cp_unitigs_count(U), links = cp_unitig_graph_links(G);
  std::vector<int64_t> off, len;
  unitig_lengths(U,off,len);
  print_unitig_line(len,tally);
  DevBuf<int64_t> d_cov, d_sup;
  d_cov.need((size_t)count+1);
  d_sup.need((size_t)links+1);
  HCHK(hipMemset(d_cov.p,0,((size_t)count+1)*8));
  HCHK(hipMemset(d_sup.p,0,((size_t)links+1)*8));

  // ---- the sequences ----
  DevBuf<char> d_seq;
  DevBuf<int64_t> d_soff, d_goff;
  DevBuf<cp_path_seg> d_segs;
  std::vector<int64_t> h_goff;
  std::vector<cp_path_seg> h_segs;
  Batch R;
  int64_t nseqs = 0, nbases = 0, nbatches = 0, ndown = 0, sum[CP_PATH_WIDTH] = { 0, 0, 0, 0, 0, 0, 0 };
  double path_secs = 0;
  bool ok = true;
  auto flush = [&]()
    { const int n = R.n();
      if (n == 0) return;
      const int64_t bases = R.soff.back();
      d_seq.need(R.seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,R.seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(R.soff);
      d_goff.need((size_t)n+1);
      d_segs.need(std::max<size_t>(1024,(size_t)(bases/16)));         // a guess: a segment per 16 bases
      int64_t total = 0, pt[CP_PATH_WIDTH];
      const auto b0 = std::chrono::steady_clock::now();
      int prc = cp_kmer_sorted_read_paths(T,U,d_utg.p,d_at.p,G,d_seq.p,d_soff.p,n,bases,d_segs.p,(int64_t)d_segs.cap,d_goff.p,
                                          d_cov.p,d_sup.p,pt,&total,nullptr);
      if (prc == CP_EOVERFLOW)                             // the total is exact and nothing was added: once more at that size
        { d_segs.need((size_t)total);
          prc = cp_kmer_sorted_read_paths(T,U,d_utg.p,d_at.p,G,d_seq.p,d_soff.p,n,bases,d_segs.p,(int64_t)d_segs.cap,d_goff.p,
                                          d_cov.p,d_sup.p,pt,&total,nullptr);
        }
      if (prc != CP_OK) cp_die(prc,"cp_kmer_sorted_read_paths");
      path_secs += since(b0);
      for (int k = 0; k < CP_PATH_WIDTH; k++) sum[k] += pt[k];
      ndown += total;
      if (gaf)
        { h_goff.resize((size_t)n+1);
          h_segs.resize((size_t)total);
          HCHK(hipMemcpy(h_goff.data(),d_goff.p,((size_t)n+1)*sizeof(int64_t),hipMemcpyDeviceToHost));
          if (total > 0) HCHK(hipMemcpy(h_segs.data(),d_segs.p,(size_t)total*sizeof(cp_path_seg),hipMemcpyDeviceToHost));
          std::string path;
          for (int r = 0; r < n; r++)
            { const int64_t rlen = R.soff[(size_t)r+1]-R.soff[(size_t)r];
              const char *header = R.headers[(size_t)r].c_str()+(R.headers[(size_t)r].empty() ? 0 : 1);
              const int name_len = (int)strcspn(header," \t");
              const int64_t s1 = h_goff[(size_t)r+1];
              for (int64_t i = h_goff[(size_t)r]; i < s1; )
                { const cp_path_seg &h = h_segs[(size_t)i];
                  const int64_t i0 = i;
                  int64_t end = h.first+h.n+K-1, plen = 0;
                  path.clear();
                  do                                       // the segments of one walk
                    { const cp_path_seg &g = h_segs[(size_t)i];
                      const int64_t u = std::min(std::max(g.x >> 1,(int64_t)0),count-1);
                      path += (g.x & 1) ? '<' : '>';
                      path += std::to_string((long long)(g.x >> 1));
                      plen += len[(size_t)u]-(i > i0 ? K-1 : 0);
                      end = g.first+g.n+K-1;
                      i++;
                    }
                  while (i < s1 && (h_segs[(size_t)i].flags & CP_PATH_JOINED_FLAG));
                  const long long span = (long long)(end-h.first);
                  ok = fprintf(gaf,"%.*s\t%lld\t%lld\t%lld\t+\t%s\t%lld\t%d\t%lld\t%lld\t%lld\t255\n",name_len,header,(long long)rlen,
                               (long long)h.first,(long long)end,path.c_str(),(long long)plen,(int)h.q,(long long)h.q+span,span,
                               span) > 0 && ok;
                }
            }
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
  if (gaf && (fclose(gaf) != 0 || !ok)) die("%s: Cannot write %s\n",PROG,gaf_path.c_str());
  int64_t touched = 0, crossed = 0;
  rc = cp_count_nonzero(d_cov.p,count,&touched,nullptr);
  if (rc == CP_OK) rc = cp_count_nonzero(d_sup.p,links,&crossed,nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_count_nonzero");
  printf("%s: %lld sequences, %lld k-mers, %lld on the graph, %lld segments, %lld walks, %lld of %lld unitigs touched, "
         "%lld of %lld links crossed\n",PROG,(long long)nseqs,(long long)sum[CP_PATH_POSITIONS],(long long)sum[CP_PATH_PRESENT],
         (long long)sum[CP_PATH_SEGMENTS],(long long)sum[CP_PATH_WALKS],(long long)touched,(long long)count,(long long)crossed,
         (long long)links);
  fflush(stdout);
  if (ferror(stdout)) die("%s: Cannot write the standard output\n",PROG);
  cp_kmer_sorted_destroy(T);
  d_utg.release();
  d_at.release();

  if (gfa)                                                     // tabgraph's file with the two RC tags
    { ok = write_gfa(gfa,U,G,K,off,d_cov.p,d_sup.p);
      if (fclose(gfa) != 0 || !ok) die("%s: Cannot write %s\n",PROG,gfa_path.c_str());
    }
  cp_unitig_graph_destroy(G);
  cp_unitigs_destroy(U);
  if (verbose)
    fprintf(stderr,"K %d: %lld entries, %lld bases, %lld batches, %lld segments brought down; %.3f s on the device for the graph, "
                   "%.3f s for the paths\n",K,(long long)A.entries,(long long)nbases,(long long)nbatches,(long long)ndown,
            graph_secs,path_secs);
  return 0;
}

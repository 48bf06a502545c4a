// tabphase.cpp -- the heterozygous k-mer pairs of a FASTK k-mer table phased from reads, on the GPU: the unique pairs of the
// table (tabhet's, under the count range) are the two alleles of a site; every sequence of the source that carries two
// sites votes for the two smaller k-mers lying on one haplotype or on two; a maximum spanning forest over the votes gives
// every site a block and a side ("Phasing heterozygous sites from reads" in include/classpro_amd.h).  The result is two
// marker tables A and B that need no parents:
//   kprof -t2 reads && tabphase reads:5- reads.fasta reads.ph && tabtrack reads.ph.A reads.ph.B asm.fasta
// The phase of one block relative to another is arbitrary: A and B mean something inside a block, which is what tabtrack's
// blocks and switches need.
//
//   tabphase [-v] [-m<int(2)>] [-b<int(67108864)>] [-T<int(4)>] <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]
//            [<out_root>]
//
// Prints two lines on stdout, always, and nothing else there:
//   tabphase: <keys> k-mers, <sites> sites, <n> sequences, <markers> markers, <links> links, <self> self
//   tabphase: <edges> edges, <kept> kept, <tied> tied, <weak> weak, <conflicts> conflicts, <blocks> blocks, largest <L> sites,
//             <single> unlinked sites                                                                      (one line)
// keys the k-mers of the unique pairs.  With <out_root> writes
//   <out_root>.A.ktab, <out_root>.B.ktab   with their parts and <out_root>.A.hist, <out_root>.B.hist as tabop writes its own;
//                                          every k-mer keeps its count and the stub's minval is the input's
//   <out_root>.sites.tsv                   one line per site in site order, tab-separated:
//                                          site block side low_kmer high_kmer low_count high_count
//                                          block = -1 for an unlinked site; side says which table the LOW k-mer went to
//                                          (0: A), the high one went to the other
// Without <out_root> no file is created.  Every output is created before the GPU is touched.
//   :<lo>-<hi>  the count range of the table, as tabhet takes it: k-mers outside it count as absent.
//   -m  the support an edge needs: the larger of its two counts must reach it.
//   -b  bases per device batch, whole sequences per batch.
//   -T  table parts of each result.
//   -v  one more line on stderr: the Boruvka rounds, the batches and the seconds on the device.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabphase <usage line>                                                  wrong number of arguments
//   tabphase: -<c> is an illegal option
//   tabphase: -<c> '<text>' argument is not an integer
//   tabphase: Support of an edge must be positive (<n>)                           -m below 1
//   tabphase: Bases per device batch must be positive (<n>)                       -b below 1
//   tabphase: Number of threads must be positive (<n>)                            -T below 1
//   tabphase: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    the table (K < 5 among them)
//   tabphase: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file           the source
//   tabphase: <out_root>.A.ktab is the operand: the result needs a name of its own
//   tabphase: Cannot open <path> for 'w'                                          the outputs
#include <algorithm>
#include "tab_out.h"
#include "read_source.h"
#include "ktab_range.h"

static const char *USAGE = "[-v] [-m<int(2)>] [-b<int(67108864)>] [-T<int(4)>]\n"
                           "                <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]] [<out_root>]";

static std::string kmer_text(uint64_t hi, uint64_t lo, int K)
{ const unsigned __int128 key = (((unsigned __int128)hi) << 63) | (unsigned __int128)lo;
  std::string s((size_t)K,'A');
  for (int p = 0; p < K; p++) s[(size_t)p] = "ACGT"[(int)(key >> (2*(K-1-p))) & 3];
  return s;
}

template <class T>
static std::vector<T> down(const T *d, size_t n)
{ std::vector<T> h(n);
  if (n) HCHK(hipMemcpy(h.data(),d,n*sizeof(T),hipMemcpyDeviceToHost));
  return h;
}

int main(int argc, char **argv)
{ PROG = "tabphase";
  bool verbose = false;
  int min_support = 2, batch_bases = 64 << 20, nthreads = 4;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-' && a[1] != '\0')
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'm': min_support = arg_int(a,"Support of an edge",true); break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2 && pos.size() != 3)
    die("Usage: %s %s\n",PROG,USAGE);
  int64_t range[2];
  const std::string name = split_range(pos[0],range);
  KtabReader A;
  A.open(name);
  const int K = A.K;
  Source S;
  std::string dir, root;
  if (!S.find(pos[1],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[1].c_str());

  // every output is created before the GPU is touched, or none is left behind
  Outputs outs;
  std::string odir, oname[2], tab_path[2], hist_path[2], tsv_path;
  FILE *ft[2] = { nullptr, nullptr }, *fh[2] = { nullptr, nullptr }, *tsv = nullptr;
  if (pos.size() == 3)
    { odir = path_to(pos[2]);
      for (int w = 0; w < 2; w++)
        { oname[w] = root_of(pos[2],"")+(w ? ".B" : ".A");
          tab_path[w] = odir+"/"+oname[w]+".ktab";
          hist_path[w] = odir+"/"+oname[w]+".hist";
          die_if_operand(tab_path[w],A.stub,"is the operand");
        }
      tsv_path = odir+"/"+root_of(pos[2],"")+".sites.tsv";
      for (int w = 0; w < 2; w++)
        { ft[w] = outs.create(tab_path[w]);
          fh[w] = outs.create(hist_path[w]);
        }
      tsv = outs.create(tsv_path);
    }
  S.open();

  // ---- the table up, its unique pairs, their sites ----
  cp_kmer_sorted *T = upload_table(A), *P = nullptr;
  int64_t het[CP_HET_WIDTH];
  double dev_s = 0;
  auto t0 = std::chrono::steady_clock::now();
  int rc = cp_kmer_sorted_het_pairs(T,range,1,1,1,nullptr,het,nullptr,nullptr,&P);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_het_pairs");
  cp_kmer_sorted_destroy(T);
  const int64_t nkeys = cp_kmer_sorted_size(P);
  DevBuf<int64_t> d_mate, d_block, d_tally, d_soff;
  DevBuf<int32_t> d_mark;
  DevBuf<uint8_t> d_side;
  DevBuf<uint64_t> d_links;
  DevBuf<char> d_seq;
  d_mate.need((size_t)nkeys+1);
  d_mark.need((size_t)nkeys+1);
  int64_t nsites = 0;
  rc = cp_kmer_sorted_het_sites(P,d_mate.p,d_mark.p,&nsites,nullptr,nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_het_sites");
  dev_s += since(t0);

  // ---- the links of every batch into a count table of K = 32 ----
  cp_kmer_counts *acc = nullptr;
  rc = cp_kmer_counts_create(32,0,&acc);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_create");
  d_tally.need(4);
  HCHK(hipMemset(d_tally.p,0,3*sizeof(int64_t)));
  std::vector<char> seq;
  std::vector<int64_t> soff{0};
  int64_t nseqs = 0, nbatches = 0;
  auto flush = [&]()
    { const int n = (int)soff.size()-1;
      if (n == 0) return;
      const int64_t bases = soff.back();
      d_seq.need(seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(soff);
      const auto b0 = std::chrono::steady_clock::now();
      int64_t total = 0;
      d_links.need(std::max<size_t>(1024,(size_t)(bases/256)));       // a guess: a link per 256 bases
      int rcb = cp_kmer_sorted_read_links(P,d_mark.p,1,d_seq.p,d_soff.p,n,bases,d_links.p,(int64_t)d_links.cap,&total,d_tally.p,nullptr);
      if (rcb == CP_EOVERFLOW)                             // the total is exact and the tally untouched: once more at that size
        { d_links.need((size_t)total);
          rcb = cp_kmer_sorted_read_links(P,d_mark.p,1,d_seq.p,d_soff.p,n,bases,d_links.p,(int64_t)d_links.cap,&total,d_tally.p,nullptr);
        }
      if (rcb != CP_OK) cp_die(rcb,"cp_kmer_sorted_read_links");
      rcb = cp_kmer_counts_add_keys(acc,nullptr,d_links.p,total,nullptr);
      if (rcb != CP_OK) cp_die(rcb,"cp_kmer_counts_add_keys");
      dev_s += since(b0);
      nbatches++;
      seq.clear();
      soff.assign(1,0);
    };
  while (S.next())
    { seq.insert(seq.end(),S.seq.begin(),S.seq.end());
      soff.push_back(soff.back()+(int64_t)S.seq.size());
      nseqs++;
      if (soff.back() >= batch_bases || soff.size()-1 == (size_t)INT32_MAX) flush();
    }
  flush();
  int64_t lt[3];
  HCHK(hipMemcpy(lt,d_tally.p,sizeof(lt),hipMemcpyDeviceToHost));
  printf("%s: %lld k-mers, %lld sites, %lld sequences, %lld markers, %lld links, %lld self\n",PROG,(long long)nkeys,
         (long long)nsites,(long long)nseqs,(long long)lt[0],(long long)lt[1],(long long)lt[2]);

  // ---- the edges, the forest, the two tables ----
  t0 = std::chrono::steady_clock::now();
  cp_kmer_sorted *E = nullptr, *R[2] = { nullptr, nullptr };
  rc = cp_kmer_counts_sort(acc,1,nullptr,&E);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_sort");
  cp_kmer_counts_destroy(acc);
  d_block.need((size_t)nsites+1);
  d_side.need((size_t)nsites+1);
  int64_t ph[CP_PH_WIDTH];
  rc = cp_phase_forest(E,nsites,min_support,d_block.p,d_side.p,ph,nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_phase_forest");
  cp_kmer_sorted_destroy(E);
  if (tsv)
    for (int w = 0; w < 2; w++)
      { rc = cp_kmer_sorted_phase_split(P,d_mark.p,d_block.p,d_side.p,nsites,w,nullptr,&R[w]);
        if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_phase_split");
      }
  dev_s += since(t0);
  printf("%s: %lld edges, %lld kept, %lld tied, %lld weak, %lld conflicts, %lld blocks, largest %lld sites, %lld unlinked sites\n",
         PROG,(long long)ph[CP_PH_EDGES],(long long)ph[CP_PH_KEPT],(long long)ph[CP_PH_TIED],(long long)ph[CP_PH_WEAK],
         (long long)ph[CP_PH_CONFLICTS],(long long)ph[CP_PH_BLOCKS],(long long)ph[CP_PH_LARGEST],(long long)ph[CP_PH_SINGLE]);
  fflush(stdout);

  if (tsv)
    { const uint64_t *p_hi, *p_lo, *p_cnt;
      rc = cp_kmer_sorted_arrays(P,&p_hi,&p_lo,&p_cnt);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_arrays");
      const std::vector<uint64_t> hi = down(p_hi,(size_t)nkeys), lo = down(p_lo,(size_t)nkeys), cnt = down(p_cnt,(size_t)nkeys);
      const std::vector<int64_t> mate = down(d_mate.p,(size_t)nkeys), block = down(d_block.p,(size_t)nsites);
      const std::vector<uint8_t> side = down(d_side.p,(size_t)nsites);
      std::vector<uint8_t> linked((size_t)nsites,0);
      for (int64_t s = 0; s < nsites; s++)
        if (block[(size_t)s] != s) linked[(size_t)s] = linked[(size_t)block[(size_t)s]] = 1;
      bool ok = true;
      int64_t s = 0;
      for (int64_t i = 0; i < nkeys && s < nsites; i++)
        { const int64_t m = mate[(size_t)i];
          if (m <= i || m >= nkeys) continue;
          ok = fprintf(tsv,"%lld\t%lld\t%d\t%s\t%s\t%llu\t%llu\n",(long long)s,linked[(size_t)s] ? (long long)block[(size_t)s] : -1LL,
                       (int)side[(size_t)s],kmer_text(hi[(size_t)i],lo[(size_t)i],K).c_str(),
                       kmer_text(hi[(size_t)m],lo[(size_t)m],K).c_str(),(unsigned long long)cnt[(size_t)i],
                       (unsigned long long)cnt[(size_t)m]) > 0 && ok;
          s++;
        }
      if (fclose(tsv) != 0 || !ok) die("%s: Cannot write %s\n",PROG,tsv_path.c_str());
      for (int w = 0; w < 2; w++)
        { std::vector<int64_t> hist((size_t)CP_MAX_KMER_CNT);
          int64_t ilow, ihigh;
          rc = cp_kmer_sorted_hist(R[w],hist.data(),&ilow,&ihigh);
          if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_hist");
          write_hist(fh[w],hist_path[w],K,ilow,ihigh,hist.data());
          KtabWriter W;
          W.write(R[w],K,A.minval,nthreads,ft[w],tab_path[w],odir,oname[w]);
          W.release();
          cp_kmer_sorted_destroy(R[w]);
        }
    }
  if (verbose)
    fprintf(stderr,"K %d: %lld entries; %lld rounds, %lld forest edges, %lld bad keys; %lld batches, %.3f s on the device\n",K,
            (long long)A.entries,(long long)ph[CP_PH_ROUNDS],(long long)ph[CP_PH_FOREST],(long long)ph[CP_PH_BAD],
            (long long)nbatches,dev_s);
  cp_kmer_sorted_destroy(P);
  return 0;
}

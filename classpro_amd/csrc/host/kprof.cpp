// kprof.cpp -- k-mer count profiles and histogram from reads alone: what `FastK -k<K> -t1 -p` leaves for ClassPro,
// counted on the GPU.
//
//   kprof [-v] [-k<int(40)>] [-T<int(4)>] [-f<int>] [-t<int>] [-N<out_root>] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// Writes <root>.hist, <root>.prof, .<root>.pidx.1..n and .<root>.prof.1..n (layout: classpro_amd/fastk.py), <root> being
// the source's path without its extension, or -N.  The source is found as ClassPro finds it: the first of .db .dam
// .fastq .fasta .fq .fa and their .gz forms that exists.  Usage errors, a source that cannot be read and an output
// directory that cannot be written are reported before the GPU is touched.
// Two passes over the reads in device batches on GPU 0 (cp_kmer_counts_*, semantics in include/classpro_amd.h):
//   1. bases up, added to the count table;
//   2. bases up again, uint16 counts down, and the -T host threads encode them with cp_encode_profile.  Part p of
//      nparts = min(T, reads) holds the reads [reads*p/nparts, reads*(p+1)/nparts).
// -f<MiB> puts a singleton filter of that many MiB (rounded up to a power of two, at most 131072) in front of the table
// ("Filtered count table" in include/classpro_amd.h): the k-mers seen once then take no slot, at the price of a third
// pass over the reads -- mark, count, profile.  The files written are byte for byte those written without -f; absent or
// 0 means no filter and the two passes above.
// -t<m> also writes the k-mer table of `FastK -t<m>`, <root>.ktab and .<root>.ktab.1..n: the distinct canonical k-mers
// that occur at least m times (m in [1, 32767]; with -f at least 2, the k-mers seen once hold no slot), in ascending
// order, with a prefix index -- what libfastk.c's Open_Kmer_Stream, Load_Kmer_Table and Find_Kmer read (layout:
// classpro_amd/fastk.py).  Between the count and the profile pass the table is sorted on the device
// (cp_kmer_counts_sort, "Sorted k-mers" in include/classpro_amd.h) and its records, encoded there, come down in ranges
// of TAB_RANGE entries through one buffer; the host only writes them (ktab_writer.h).  Part p of nparts =
// max(1, min(T, entries)) holds the entries [entries*p/nparts, entries*(p+1)/nparts).  The snapshot is destroyed before
// the profile pass starts.
// Without -t every file is what it was.  K < 5 has no .ktab (the reader decodes one to three prefix bytes).
// A k-mer with a byte other than upper-case A C G T is not counted and gets count 0; how many there were is always said
// on stderr.  FastK's own treatment of such bases is not reproduced.
#include "gpu_tool.h"
#include "read_source.h"
#include "prof_writer.h"
#include "ktab_writer.h"
#include "thread_pool.h"

static const char *USAGE = "[-v] [-k<int(40)>] [-T<int(4)>] [-N<out_root>] <source>[.db|.dam|.f[ast][aq][.gz]]";

static const long long MAX_FILTER_MIB = 1ll << 17;           // 2^40 bits, the library's limit
static const int64_t BATCH_BASES = (int64_t)64 << 20;        // bases per device batch

struct Batch
  { std::vector<char> seq;
    std::vector<int64_t> soff{0}, poff{0};
    void clear() { seq.clear(); soff.assign(1,0); poff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

int main(int argc, char **argv)
{ PROG = "kprof";
  bool verbose = false;
  int K = 40, nthreads = 4;
  int64_t filter_mib = 0;
  int tab_min = 0;                                                  // -t: 0 = no k-mer table
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
          case 'k': K = arg_int(a,"K-mer length",true); break;
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
          case 'N': out_root = a+2; break;
          case 't': tab_min = (int)arg_range(a,"Table cutoff",1,CP_MAX_KMER_CNT); break;
          case 'f': filter_mib = arg_range(a,"Filter size",0,MAX_FILTER_MIB," MiB"); break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 1)
    die("Usage: %s %s\n",PROG,USAGE);
  if (K < 2 || K > 63)
    die("%s: K-mer length must lie in [2, 63] (%d)\n",PROG,K);
  if (tab_min == 1 && filter_mib)
    die("%s: -t1 needs the k-mers seen once, which -f keeps out of the table: give -t2 or more, or drop -f\n",PROG);
  if (tab_min && cp_ktab_ibyte(K) == 0)
    die("%s: -t needs a K-mer length of at least 5 (%d): a k-mer table has one to three prefix bytes\n",PROG,K);

  Source S;
  std::string path, root;
  if (!S.find(pos[0],&path,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[0].c_str());
  if (out_root.empty()) out_root = path+"/"+root;
  const std::string odir = path_to(out_root), oname = root_of(out_root,"");
  const std::string hist_path = odir+"/"+oname+".hist", stub_path = odir+"/"+oname+".prof";
  FILE *fh = fopen(hist_path.c_str(),"wb");
  if (!fh) die("%s: Cannot open %s for 'w'\n",PROG,hist_path.c_str());
  FILE *fs = fopen(stub_path.c_str(),"wb");
  if (!fs) die("%s: Cannot open %s for 'w'\n",PROG,stub_path.c_str());
  const std::string tab_path = odir+"/"+oname+".ktab";
  FILE *ft = nullptr;
  if (tab_min && !(ft = fopen(tab_path.c_str(),"wb")))
    die("%s: Cannot open %s for 'w'\n",PROG,tab_path.c_str());
  S.open();
  if (verbose)
    fprintf(stderr,"Input = %s, K = %d, outputs = %s.hist, %s.prof, %s/.%s.{pidx,prof}.*\n",S.path.c_str(),K,
            (odir+"/"+oname).c_str(),(odir+"/"+oname).c_str(),odir.c_str(),oname.c_str());

  // ---- pass 1: count (with -f: mark, then count) ----
  const int Km1 = K-1;
  cp_kmer_counts *T = nullptr;
  DevBuf<char> d_seq;
  DevBuf<int64_t> d_soff, d_poff;
  DevBuf<uint16_t> d_prof;
  Batch B;
  int64_t nreads = 0, nbases = 0;
  auto device_up = [&]()                                            // the first device work of the process
    { if (T) return;
      HCHK(hipSetDevice(0));
      const int rc = filter_mib ? cp_kmer_counts_create_filtered(K,0,filter_mib << 23,&T)
                                : cp_kmer_counts_create(K,0,&T);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_create");
    };
  auto push = [&]()
    { const size_t len = S.seq.size();
      B.seq.insert(B.seq.end(),S.seq.begin(),S.seq.end());
      B.soff.push_back(B.soff.back()+(int64_t)len);
      B.poff.push_back(B.poff.back()+((int64_t)len > Km1 ? (int64_t)len-Km1 : 0));
    };
  auto upload = [&]()
    { device_up();
      d_seq.need(B.seq.size()+1);
      if (!B.seq.empty()) HCHK(hipMemcpy(d_seq.p,B.seq.data(),B.seq.size(),hipMemcpyHostToDevice));
      d_soff.up(B.soff);
    };
  bool marking = filter_mib != 0;                                   // with -f: the mark pass comes first
  auto add = [&]()
    { if (B.n() == 0) return;
      upload();
      const int rc = marking ? cp_kmer_counts_mark(T,d_seq.p,d_soff.p,B.n(),B.soff.back(),nullptr)
                             : cp_kmer_counts_add(T,d_seq.p,d_soff.p,B.n(),B.soff.back(),nullptr);
      if (rc != CP_OK) cp_die(rc,marking ? "cp_kmer_counts_mark" : "cp_kmer_counts_add");
      B.clear();
    };
  // One pass over the reads: each is pushed, and `batch` takes what has gathered at BATCH_BASES and at the end.  The
  // first pass counts the reads and bases; a later one starts the source again and has to meet the same reads.
  auto pass = [&](bool first, const auto &batch)
    { if (!first) S.rewind();
      int64_t seen = 0;
      while (S.next())
        { if (!first && seen >= nreads) die("%s: %s changed while it was read\n",PROG,S.path.c_str());
          push();
          seen++;
          if (first) nbases += (int64_t)S.seq.size();
          if (B.soff.back() >= BATCH_BASES) batch();
        }
      batch();
      if (first) nreads = seen;
      else if (seen != nreads) die("%s: %s changed while it was read\n",PROG,S.path.c_str());
    };
  pass(true,add);
  device_up();
  if (marking)                                                      // the same reads again, counted
    { marking = false;
      pass(false,add);
    }

  cp_kmer_count_stats st;
  int rc = cp_kmer_counts_stats(T,&st);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_stats");
  { std::vector<int64_t> hist((size_t)CP_MAX_KMER_CNT);
    int64_t ilow = 0, ihigh = 0;
    rc = cp_kmer_counts_hist(T,hist.data(),&ilow,&ihigh);
    if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_hist");
    write_hist(fh,hist_path,K,ilow,ihigh,hist.data());
  }

  // ---- -t: the sorted table, between the passes ----
  std::string tabled;                                               // what -t adds to the -v line
  if (tab_min)
    { cp_kmer_sorted *sorted = nullptr;
      rc = cp_kmer_counts_sort(T,tab_min,nullptr,&sorted);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_sort");
      KtabWriter TW;
      TW.write(sorted,K,tab_min,nthreads,ft,tab_path,odir,oname);
      TW.release();
      const int64_t entries = TW.entries;
      const int ibyte = TW.ibyte, tparts = TW.nparts;
      cp_kmer_sorted_destroy(sorted);
      char m[160];
      snprintf(m,sizeof(m),", %lld table entries, minval %d, ibyte %d, %d table parts",(long long)entries,tab_min,ibyte,tparts);
      tabled = m;
    }

  // ---- pass 2: profiles ----
  const int nparts = (int)std::min<int64_t>(nthreads,nreads);
  ProfWriter W;
  W.open(fs,stub_path,K,nparts,nreads,odir,oname);
  ThreadPool pool(nthreads);
  std::vector<uint16_t> h_prof;
  std::vector<std::vector<uint8_t>> code((size_t)nthreads);          // per thread: the codes of its reads of the batch
  auto profile = [&]()
    { const int n = B.n();
      if (n == 0) return;
      upload();
      d_poff.up(B.poff);
      const int64_t cells = B.poff.back();
      d_prof.need((size_t)cells+8);
      rc = cp_kmer_counts_profiles(T,d_seq.p,d_soff.p,d_poff.p,n,B.soff.back(),d_prof.p,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_profiles");
      h_prof.resize((size_t)cells+1);
      if (cells > 0) HCHK(hipMemcpy(h_prof.data(),d_prof.p,(size_t)cells*2,hipMemcpyDeviceToHost));
      else HCHK(hipDeviceSynchronize());
      W.clen.assign((size_t)n,0);
      const int nt = std::min(nthreads,n);
      pool.parallel_for(nt,[&](int64_t t)                            // thread t: a contiguous range of the batch's reads
        { const int r0 = (int)((int64_t)n*t/nt), r1 = (int)((int64_t)n*(t+1)/nt);
          std::vector<uint8_t> &c = code[(size_t)t];
          c.resize((size_t)(2*(B.poff[(size_t)r1]-B.poff[(size_t)r0])+2*(r1-r0)+2));
          int64_t o = 0;
          for (int r = r0; r < r1; r++)
            { const int64_t np = B.poff[(size_t)r+1]-B.poff[(size_t)r];
              const int64_t l = cp_encode_profile(h_prof.data()+B.poff[(size_t)r],(int)np,c.data()+o,(int64_t)c.size()-o);
              if (l < 0) cp_die((int)l,"cp_encode_profile");
              W.clen[(size_t)r] = l;
              o += l;
            }
        });
      for (int t = 0; t < nt; t++)
        W.append((int)((int64_t)n*t/nt),(int)((int64_t)n*(t+1)/nt),code[(size_t)t].data());
      B.clear();
    };
  pass(false,profile);
  rc = cp_kmer_counts_stats(T,&st);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_stats");
  W.close();
  std::string filtered;                                             // what -f adds to the -v line
  if (verbose && filter_mib)
    { cp_kmer_filter_stats fs;
      rc = cp_kmer_counts_filter_stats(T,&fs);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_filter_stats");
      char m[200];
      snprintf(m,sizeof(m),", %lld table keys, %lld keys kept outside, %lld false positives, %lld filter bytes",
               (long long)fs.n_table_keys,(long long)fs.n_outside,(long long)fs.n_false,(long long)fs.filter_bytes);
      filtered = m;
    }
  if (verbose)
    fprintf(stderr,"%lld reads, %lld bases, %lld k-mers counted, %lld distinct, %lld skipped, %lld slots, %lld growth steps, "
                   "%d profile parts%s%s\n",(long long)nreads,(long long)nbases,(long long)st.n_kmers,(long long)st.n_distinct,
            (long long)st.n_skipped,(long long)st.slots,(long long)st.growths,nparts,filtered.c_str(),tabled.c_str());
  if (st.n_skipped)
    fprintf(stderr,"%s: %lld k-mer positions skipped (a byte other than upper-case A C G T): their count is 0\n",PROG,
            (long long)st.n_skipped);
  cp_kmer_counts_destroy(T);
  return 0;
}

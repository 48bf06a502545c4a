// genome2class.cpp -- ground-truth .class file of a read set from the genome it was sampled from: what
// `FastK -k<K> -t1 -p genome`, `FastK -k<K> -p:genome -N<reads>.truth reads` and `prof2class <reads>.truth.prof reads`
// leave (step 2-1 of the reference's workflow), counted and labelled on the GPU.
//
//   genome2class [-v] [-p] [-k<int(40)>] [-T<int(4)>] [-b<int(67108864)>] [-N<out_root>] [-A<est.class>]
//                <genome>[.f[ast][aq][.gz]|.db|.dam] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// Writes <out_root>.class, one "@header\nseq\n+\nlabels\n" record per read: K-1 'N' (rlen 'N' for a read shorter than K),
// then per k-mer E, H, D or R for 0, 1, 2 or >= 3 occurrences of its canonical form in the genome.  out_root defaults to
// the source's path and root plus ".truth".  The file is byte for byte what prof2class writes from the relative profile
// (class_record.h holds what the two share), including the `rlen > 60000` error for FASTX sources.  Both inputs are found
// as kprof finds its source: the first of .db .dam .fastq .fasta .fq .fa and their .gz forms that exists.
//   -p  also writes the relative profile as <out_root>.prof, .<out_root>.pidx.1..n and .<out_root>.prof.1..n in kprof's
//       layout (nparts = min(T, reads), cp_encode_profile); no .hist, as FastK writes none for -p:.
//   -A  <est.class> is read in step with the source (names and lengths checked with class2acc's messages), the
//       estimate's labels go up with the batch and cp_acc_add counts on the labels still in HBM; after the output is
//       written, stdout gets exactly what `class2acc <est.class> <out_root>.class` prints with default options.
//   -b  bases per device batch, for the genome and for the reads.
//   -v  one summary line on stderr.
// Pass 1 puts the genome into a cp_kmer_counts on GPU 0.  Its a c g t count as A C G T (assemblies are soft-masked; the
// fold is done on the host before upload); a contig longer than -b bases is cut into pieces that overlap by K-1 bases, so
// every k-mer of it is counted exactly once and no piece exceeds -b + K-1 bases.  Pass 2 runs
// cp_kmer_counts_rel_labels over the reads in batches; labels come down packed (0.25 B/base) and the -T host threads
// expand them.  The reads are NOT folded: a read k-mer that holds a byte other than upper-case A C G T is E (count 0),
// as in kprof; how many there were is always said on stderr.
//
// Reported on stderr with exit status 1 before the GPU is touched:
//   Usage: genome2class <usage line>                                              wrong number of arguments
//   genome2class: -<c> is an illegal option
//   genome2class: -<c> '<text>' argument is not an integer
//   genome2class: K-mer length must be positive (<n>)                             -k below 1
//   genome2class: K-mer length must lie in [2, 63] (<K>)
//   genome2class: Number of threads must be positive (<n>)                        -T below 1
//   genome2class: Bases per device batch must be positive (<n>)                   -b below 1
//   genome2class: -A needs a path (-A<est.class>)
//   genome2class: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file       genome or source
//   genome2class: Cannot open <path> for 'w'                                      <out_root>.class, with -p <out_root>.prof
//   genome2class: Cannot open <est.class> [errno=<n>]
#include "gpu_tool.h"
#include "read_source.h"
#include "prof_writer.h"
#include "thread_pool.h"

static const char *USAGE = "[-v] [-p] [-k<int(40)>] [-T<int(4)>] [-b<int(67108864)>] [-N<out_root>] [-A<est.class>]\n"
                           "                    <genome>[.f[ast][aq][.gz]|.db|.dam] <source>[.db|.dam|.f[ast][aq][.gz]]";

struct Batch
  { std::vector<std::string> headers;
    std::vector<char> seq, est;
    std::vector<int64_t> soff{0}, poff{0}, koff{0};                  // bases, profile cells, packed label bytes
    void clear() { headers.clear(); seq.clear(); est.clear(); soff.assign(1,0); poff.assign(1,0); koff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

int main(int argc, char **argv)
{ PROG = "genome2class";
  bool verbose = false, want_prof = false;
  int K = 40, nthreads = 4, batch_bases = 64 << 20;
  std::string out_root;
  const char *est_path = nullptr;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-')
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else if (a[k] == 'p') want_prof = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'k': K = arg_int(a,"K-mer length",true); break;
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'N': out_root = a+2; break;
          case 'A':
            if (a[2] == '\0') die("%s: -A needs a path (-A<est.class>)\n",PROG);
            est_path = a+2;
            break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  if (K < 2 || K > 63)
    die("%s: K-mer length must lie in [2, 63] (%d)\n",PROG,K);

  Source G, S;
  std::string dir, root;
  if (!G.find(pos[0],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[0].c_str());
  if (!S.find(pos[1],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[1].c_str());
  if (out_root.empty()) out_root = dir+"/"+root+".truth";
  const std::string odir = path_to(out_root), oname = root_of(out_root,"");
  const std::string class_path = odir+"/"+oname+".class", stub_path = odir+"/"+oname+".prof";
  FILE *out = fopen(class_path.c_str(),"w");
  if (!out) die("%s: Cannot open %s for 'w'\n",PROG,class_path.c_str());
  FILE *fs = nullptr;
  if (want_prof && !(fs = fopen(stub_path.c_str(),"wb")))
    die("%s: Cannot open %s for 'w'\n",PROG,stub_path.c_str());
  FastxReader est(est_path ? est_path : "/dev/null");
  if (!est.f) die("%s: Cannot open %s [errno=%d]\n",PROG,est_path,errno);
  G.open();
  S.open();
  std::vector<char> obuf(1 << 22);
  setvbuf(out,obuf.data(),_IOFBF,obuf.size());
  if (verbose)
    fprintf(stderr,"Genome = %s, Input = %s, K = %d, Output = %s\n",G.path.c_str(),S.path.c_str(),K,class_path.c_str());

  const int Km1 = K-1;
  const int64_t BB = batch_bases;
  cp_kmer_counts *T = nullptr;
  cp_acc *acc = nullptr;
  DevBuf<char> d_seq, d_lab, d_est;
  DevBuf<uint8_t> d_pack;
  DevBuf<int64_t> d_soff, d_poff, d_koff;
  DevBuf<uint16_t> d_prof;
  int64_t *d_counts = nullptr;
  auto device_up = [&]()                                            // the first device work of the process
    { if (T) return;
      HCHK(hipSetDevice(0));
      int rc = cp_kmer_counts_create(K,0,&T);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_create");
      if (est_path && (rc = cp_acc_create(K,100,0,&acc)) != CP_OK) cp_die(rc,"cp_acc_create");
      HCHK(hipMalloc((void **)&d_counts,4*sizeof(int64_t)));
      HCHK(hipMemset(d_counts,0,4*sizeof(int64_t)));
    };

  // ---- pass 1: the genome into the count table ----
  int64_t ncontigs = 0, gbases = 0, npieces = 0;
  { std::vector<char> seq;
    std::vector<int64_t> soff{0};
    auto add = [&]()
      { if (soff.size() == 1) return;
        device_up();
        d_seq.need(seq.size()+1);
        if (!seq.empty()) HCHK(hipMemcpy(d_seq.p,seq.data(),seq.size(),hipMemcpyHostToDevice));
        d_soff.up(soff);
        const int rc = cp_kmer_counts_add(T,d_seq.p,d_soff.p,(int)soff.size()-1,soff.back(),nullptr);
        if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_add");
        seq.clear();
        soff.assign(1,0);
      };
    while (G.next())
      { std::string &c = G.seq;
        const int64_t len = (int64_t)c.size();
        ncontigs++;
        gbases += len;
        for (int64_t i = 0; i < len; i++)                          // soft-masked bases count
          { const char b = c[(size_t)i];
            if (b == 'a' || b == 'c' || b == 'g' || b == 't') c[(size_t)i] = (char)(b-32);
          }
        // piece i holds the bases [i*BB, (i+1)*BB + K-1): its k-mers end at [i*BB + K-1, (i+1)*BB + K-1)
        for (int64_t s = 0; s+Km1 < len; s += BB)
          { const int64_t e = std::min(len,s+BB+Km1);
            seq.insert(seq.end(),c.begin()+s,c.begin()+e);
            soff.push_back(soff.back()+(e-s));
            npieces++;
            if (soff.back() >= BB) add();
          }
      }
    add();
  }
  device_up();
  cp_kmer_count_stats st;
  int rc = cp_kmer_counts_stats(T,&st);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_stats");

  // ---- pass 2: the reads ----
  int64_t nreads_known = -1;                                         // -p: the parts are cut by read number
  if (want_prof)
    { if (S.is_db) nreads_known = S.db.nreads;
      else
        { nreads_known = 0;
          while (S.next()) nreads_known++;
          S.rewind();
        }
    }
  const int nparts = want_prof ? (int)std::min<int64_t>(nthreads,nreads_known) : 0;
  ProfWriter W;
  if (want_prof) W.open(fs,stub_path,K,nparts,nreads_known,odir,oname);
  ThreadPool pool(nthreads);
  Batch B;
  std::vector<uint8_t> h_pack;
  std::vector<uint16_t> h_prof;
  std::vector<std::string> text((size_t)nthreads);                   // per thread: the records of its reads of the batch
  std::vector<std::vector<uint8_t>> code((size_t)nthreads);          // per thread: the profile codes of its reads
  std::vector<int64_t> tskip((size_t)nthreads,0);
  int64_t nreads = 0, nbases = 0;
  auto flush = [&]()
    { const int n = B.n();
      if (n == 0) return;
      const int64_t bases = B.soff.back(), cells = B.poff.back(), pbytes = B.koff.back();
      d_seq.need(B.seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,B.seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(B.soff);
      d_koff.up(B.koff);
      d_pack.need((size_t)pbytes+8);
      if (want_prof) { d_poff.up(B.poff); d_prof.need((size_t)cells+8); }
      if (est_path) d_lab.need((size_t)bases+1);
      rc = cp_kmer_counts_rel_labels(T,d_seq.p,d_soff.p,n,bases,want_prof ? d_prof.p : nullptr,
                                     want_prof ? d_poff.p : nullptr,est_path ? d_lab.p : nullptr,d_pack.p,d_koff.p,
                                     d_counts,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_counts_rel_labels");
      if (est_path)
        { d_est.up(B.est);
          rc = cp_acc_add(acc,d_est.p,d_lab.p,d_soff.p,n,bases,nullptr);
          if (rc != CP_OK) cp_die(rc,"cp_acc_add");
        }
      h_pack.resize((size_t)pbytes+1);
      if (pbytes > 0) HCHK(hipMemcpy(h_pack.data(),d_pack.p,(size_t)pbytes,hipMemcpyDeviceToHost));
      if (want_prof)
        { h_prof.resize((size_t)cells+1);
          if (cells > 0) HCHK(hipMemcpy(h_prof.data(),d_prof.p,(size_t)cells*2,hipMemcpyDeviceToHost));
        }
      HCHK(hipDeviceSynchronize());
      W.clen.assign((size_t)n,0);
      const int nt = std::min(nthreads,n);
      pool.parallel_for(nt,[&](int64_t t)                            // thread t: a contiguous range of the batch's reads
        { const int r0 = (int)((int64_t)n*t/nt), r1 = (int)((int64_t)n*(t+1)/nt);
          std::string &x = text[(size_t)t], lab;
          x.clear();
          std::vector<uint8_t> &c = code[(size_t)t];
          if (want_prof) c.resize((size_t)(2*(B.poff[(size_t)r1]-B.poff[(size_t)r0])+2*(r1-r0)+2));
          int64_t o = 0, skip = 0;
          for (int r = r0; r < r1; r++)
            { const int64_t s = B.soff[(size_t)r], len = B.soff[(size_t)r+1]-s;
              const char *q = B.seq.data()+s;
              lab.resize((size_t)len);
              if (len > 0)
                { const int e = cp_unpack_labels(h_pack.data()+B.koff[(size_t)r],(int)len,K,&lab[0]);
                  if (e != CP_OK) cp_die(e,"cp_unpack_labels");
                }
              int valid = 0;                                         // k-mers that hold another byte
              for (int64_t i = 0; i < len; i++)
                { const char b = q[i];
                  valid = (b == 'A' || b == 'C' || b == 'G' || b == 'T') ? valid+1 : 0;
                  if (i >= Km1 && valid < K) skip++;
                }
              x += B.headers[(size_t)r]; x += '\n';
              x.append(q,(size_t)len); x += "\n+\n";
              x += lab; x += '\n';
              if (want_prof)
                { const int64_t np = B.poff[(size_t)r+1]-B.poff[(size_t)r];
                  const int64_t l = cp_encode_profile(h_prof.data()+B.poff[(size_t)r],(int)np,c.data()+o,(int64_t)c.size()-o);
                  if (l < 0) cp_die((int)l,"cp_encode_profile");
                  W.clen[(size_t)r] = l;
                  o += l;
                }
            }
          tskip[(size_t)t] += skip;
        });
      for (int t = 0; t < nt; t++)
        { const std::string &x = text[(size_t)t];
          if (!x.empty() && fwrite(x.data(),1,x.size(),out) != x.size()) die("%s: Cannot write %s\n",PROG,class_path.c_str());
          if (want_prof) W.append((int)((int64_t)n*t/nt),(int)((int64_t)n*(t+1)/nt),code[(size_t)t].data());
        }
      B.clear();
    };

  const int rlen_max = S.is_db ? S.db.maxlen : CLASS_FASTX_RLEN_MAX;
  while (S.next())
    { const int64_t rlen = (int64_t)S.seq.size();
      if (want_prof && nreads >= nreads_known) die("%s: %s changed while it was read\n",PROG,S.path.c_str());
      if (rlen > rlen_max)                                           // prof2class.c:154-160
        { flush();
          fflush(out);
          die("rlen (%d) > rlen_max (%d)\n",(int)rlen,rlen_max);
        }
      if (est_path)                                                  // class2acc.c:141-160, this file being the truth
        { const int id = (int)nreads+1;
          const std::string name = class_header_name(S.header);
          if (est.next() < 0)
            die("# seqs in %s < # seqs in %s\n",est_path,class_path.c_str());
          if (est.name != name)
            die("Read %d inconsistent names: %s (estimate) vs %s (truth)\n",id,est.name.c_str(),name.c_str());
          if (!(est.seq.size() == est.qual.size() && est.seq.size() == (size_t)rlen))
            die("Read %d inconsistent lengths\n",id);
          for (int64_t i = 0; i < rlen && i <= Km1; i++)
            if ((est.qual[(size_t)i] == 'N') != (i < Km1))
              die("Read %d inconsistent # of prefix Ns (= K-1)\n",id);
          B.est.insert(B.est.end(),est.qual.begin(),est.qual.end());
        }
      B.headers.push_back(S.header);
      B.seq.insert(B.seq.end(),S.seq.begin(),S.seq.end());
      B.soff.push_back(B.soff.back()+rlen);
      B.poff.push_back(B.poff.back()+(rlen > Km1 ? rlen-Km1 : 0));
      B.koff.push_back(B.koff.back()+((rlen+3) >> 2));
      nreads++;
      nbases += rlen;
      if (B.soff.back() >= BB) flush();
    }
  flush();
  if (want_prof && nreads != nreads_known) die("%s: %s changed while it was read\n",PROG,S.path.c_str());
  if (fclose(out) != 0) die("%s: Cannot write %s\n",PROG,class_path.c_str());
  W.close();
  if (est_path && est.next() >= 0)
    die("# seqs in %s > # seqs in %s\n",est_path,class_path.c_str());

  int64_t counts[4];
  HCHK(hipMemcpy(counts,d_counts,sizeof(counts),hipMemcpyDeviceToHost));
  int64_t rskip = 0;
  for (int64_t x : tskip) rskip += x;
  if (verbose)
    fprintf(stderr,"%lld contigs, %lld genome bases, %lld pieces, %lld k-mers counted, %lld distinct, %lld skipped, "
                   "%lld reads, %lld bases, E %lld, H %lld, D %lld, R %lld\n",(long long)ncontigs,(long long)gbases,
            (long long)npieces,(long long)st.n_kmers,(long long)st.n_distinct,(long long)st.n_skipped,(long long)nreads,
            (long long)nbases,(long long)counts[0],(long long)counts[1],(long long)counts[2],(long long)counts[3]);
  if (rskip)
    fprintf(stderr,"%s: %lld k-mer positions of the reads hold a byte other than upper-case A C G T: their label is E\n",
            PROG,(long long)rskip);
  if (est_path)
    { print_acc_report(stdout,acc_totals(acc));
      fflush(stdout);
      cp_acc_destroy(acc);
    }
  HCHK(hipFree(d_counts));
  cp_kmer_counts_destroy(T);
  return 0;
}

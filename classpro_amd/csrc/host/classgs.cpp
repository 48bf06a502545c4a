// classgs.cpp -- k-mer labels from three global count thresholds (the GenomeScope-style baseline of the paper), and,
// with -A, their accuracy against a ground-truth .class file.
//
//   ClassGS [-A<truth.class>] <source_root> <E/H_thres> <H/D_thres> <D/R_thres>
//
// Without -A this is the reference's tool (src/ClassGS.c): a count c is E if c < E/H, else H if c < H/D, else D if
// c < D/R, else R; profiles come from <source_root>.prof, the reads from the first of <source_root>.db .dam .fastq
// .fasta .fq .fa and their .gz forms that exists, and <source_root>.GS.class gets one "@header\nseq\n+\nlabels\n"
// record per read (K-1 leading 'N's; a read shorter than K gets rlen 'N's).  Same usage line, stderr lines, messages
// and exit status.  Usage errors and files that cannot be opened are reported before the GPU is touched.
// The labelling runs on GPU 0 in batches: FASTK code strings up, cp_decode_profiles, cp_threshold_labels, labels down.
// A code string that does not expand to rlen-(K-1) counts is an error here (the reference does not check).
//   -A  <truth.class> is read in step with the input (names and lengths checked with class2acc's messages), the truth
//       labels go up with the batch and cp_acc_add counts on the labels still in HBM; after the output is written,
//       stdout gets exactly what `class2acc <source_root>.GS.class <truth.class>` prints with default options.
#include "gpu_tool.h"
#include "dazz_db.h"
#include "class_record.h"

static const char *USAGE = "<source_root> <E/H_thres> <H/D_thres> <D/R_thres>";

static const int64_t BATCH_BASES = (int64_t)64 << 20;        // bases per device batch

struct Batch
  { std::vector<std::string> headers;
    std::vector<char> seq, truth;
    std::vector<uint8_t> code;
    std::vector<int64_t> soff{0}, poff{0}, coff{0};
    std::vector<int64_t> id;                                     // 0-based read number, for messages
    void clear()
    { headers.clear(); seq.clear(); truth.clear(); code.clear(); id.clear();
      soff.assign(1,0); poff.assign(1,0); coff.assign(1,0);
    }
    int n() const { return (int)headers.size(); }
  };

struct Device
  { bool up = false;
    cp_workspace *ws = nullptr;
    cp_acc *acc = nullptr;
    DevBuf<uint8_t> code;
    DevBuf<int64_t> soff, poff, coff;
    DevBuf<uint16_t> prof;
    DevBuf<char> lab, truth;
    std::vector<char> h_lab;
  };

int main(int argc, char **argv)
{ PROG = "ClassGS";
  const char *truth_path = nullptr;
  std::vector<const char *> pos;
  for (int i = 1; i < argc; i++)
    if (argv[i][0] == '-')
      { if (argv[i][1] == 'A')
          { if (argv[i][2] == '\0') die("%s: -A needs a path (-A<truth.class>)\n",PROG);
            truth_path = argv[i]+2;
            continue;
          }
        for (int k = 1; argv[i][k]; k++)                           // ARG_FLAGS(""): the reference has no flags
          die("%s: -%c is an illegal option\n",PROG,argv[i][k]);
      }
    else
      pos.push_back(argv[i]);
  if (pos.size() != 4)
    die("Usage: %s %s\n",PROG,USAGE);
  const std::string root = pos[0];
  int32_t thres[3];
  for (int i = 0; i < 3; i++) thres[i] = (int)strtol(pos[(size_t)i+1],nullptr,10);     // ClassGS.c:73-75
  fprintf(stderr,"E < %d <= H < %d <= D < %d <= R\n",thres[0],thres[1],thres[2]);

  int ext;
  for (ext = 0; ext < 10; ext++)                                 // ClassGS.c:20-23: the root as given, not split
    { int fd = open((root+EXT[ext]).c_str(),O_RDONLY);
      if (fd >= 0) { close(fd); break; }
    }
  if (ext == 10)
    die("Cannot open %s[.db|.dam|.f{ast}[aq][.gz]] as a file\n",root.c_str());
  const bool is_db = ext <= 1, is_dam = ext == 1;
  const std::string source = root+EXT[ext], out_path = root+".GS.class";
  FILE *out = fopen(out_path.c_str(),"w");
  if (!out) die("%s: Cannot open %s for 'w'\n",PROG,out_path.c_str());
  fprintf(stderr,"Input = %s, Output = %s\n",source.c_str(),out_path.c_str());

  Profiles P;
  if (!P.open(root))
    die("%s: Cannot open %s.prof\n",PROG,root.c_str());
  FastxReader fx(is_db ? "/dev/null" : source.c_str());
  if (!fx.f) die("%s: Cannot open %s [errno=%d]\n",PROG,source.c_str(),errno);
  DazzDB db;
  if (is_db)
    { db.open(source,is_dam);
      if (P.nreads != db.nreads)                                   // ClassGS.c:116-119
        die("Inconsistent # of reads: .prof (%d) != .db (%d)\n",(int)P.nreads,db.nreads);
    }
  FastxReader tru(truth_path ? truth_path : "/dev/null");
  if (!tru.f) die("%s: Cannot open %s [errno=%d]\n",PROG,truth_path,errno);
  std::vector<char> obuf(1 << 22);
  setvbuf(out,obuf.data(),_IOFBF,obuf.size());

  const int K = P.kmer, Km1 = K-1, rlen_max = is_db ? db.maxlen : CP_MAX_READ_LEN;     // ClassGS.c:165-171
  Device D;
  Batch B;

  auto flush = [&]()
    { const int n = B.n();
      if (n == 0) return;
      const int64_t bases = B.soff[(size_t)n], kmers = B.poff[(size_t)n];
      if (!D.up)                                                   // the first device work of the process
        { HCHK(hipSetDevice(0));
          int rc = cp_workspace_create(&D.ws);
          if (rc != CP_OK) cp_die(rc,"cp_workspace_create");
          if (truth_path && (rc = cp_acc_create(K,100,0,&D.acc)) != CP_OK) cp_die(rc,"cp_acc_create");
          D.up = true;
        }
      D.code.up(B.code); D.coff.up(B.coff); D.poff.up(B.poff); D.soff.up(B.soff);
      D.prof.need((size_t)kmers+8);
      D.lab.need((size_t)bases+1);
      int rc = cp_decode_profiles(D.ws,D.code.p,D.coff.p,D.poff.p,n,D.prof.p,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_decode_profiles");
      if (cp_workspace_check(D.ws) != CP_OK)
        { // a failed decode: find the read on the host, with ClassPro's message (ClassPro.c:234-237)
          std::vector<uint16_t> tmp(1);
          for (int i = 0; i < n; i++)
            { const int rlen = (int)(B.soff[(size_t)i+1]-B.soff[(size_t)i]);
              const int plen = cp_decode_profile(B.code.data()+B.coff[(size_t)i],B.coff[(size_t)i+1]-B.coff[(size_t)i],tmp.data(),0);
              if (plen >= 0 && plen != (rlen > Km1 ? rlen-Km1 : 0))
                die("Read %lld: rlen (%d) != plen+Km1 (%d)\n",(long long)B.id[(size_t)i]+1,rlen,plen+Km1);
            }
          die("%s\n",cp_last_error());
        }
      rc = cp_threshold_labels(K,thres,D.prof.p,D.poff.p,D.soff.p,n,bases,D.lab.p,nullptr,nullptr,nullptr,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_threshold_labels");
      if (truth_path)
        { D.truth.up(B.truth);
          rc = cp_acc_add(D.acc,D.lab.p,D.truth.p,D.soff.p,n,bases,nullptr);
          if (rc != CP_OK) cp_die(rc,"cp_acc_add");
        }
      D.h_lab.resize((size_t)bases+1);
      if (bases > 0) HCHK(hipMemcpy(D.h_lab.data(),D.lab.p,(size_t)bases,hipMemcpyDeviceToHost));
      for (int i = 0; i < n; i++)
        { const int64_t s = B.soff[(size_t)i], len = B.soff[(size_t)i+1]-s;
          write_class_record(out,B.headers[(size_t)i],B.seq.data()+s,(size_t)len,D.h_lab.data()+s,(size_t)len);
        }
      B.clear();
    };

  std::string header;
  for (int64_t id = 0; id < P.nreads; id++)
    { int rlen;
      if (is_db)
        { db.load((int)id,fx.seq);
          rlen = (int)fx.seq.size();
          header = db.header((int)id);
        }
      else
        { rlen = fx.next();
          if (rlen < 0) { rlen = 0; fx.seq.clear(); }                // the reference does not check kseq_read here
          header = "@"+fx.name+" "+(fx.have_comment ? fx.comment : std::string("(null)"));
        }
      if (rlen > rlen_max)                                         // ClassGS.c:197-200
        { flush();
          fflush(out);
          die("rlen (%d) > rlen_max (%d)\n",rlen,rlen_max);
        }
      if (truth_path)                                              // class2acc.c:141-160
        { const std::string name = class_header_name(header);
          if (tru.next() < 0)
            die("# seqs in %s > # seqs in %s\n",out_path.c_str(),truth_path);
          if (name != tru.name)
            die("Read %d inconsistent names: %s (estimate) vs %s (truth)\n",(int)id+1,name.c_str(),tru.name.c_str());
          if (!(tru.seq.size() == tru.qual.size() && tru.seq.size() == (size_t)rlen))
            die("Read %d inconsistent lengths\n",(int)id+1);
          for (int i = 0; i < rlen && i < Km1; i++)
            if (tru.qual[(size_t)i] != 'N')
              die("Read %d inconsistent # of prefix Ns (= K-1)\n",(int)id+1);
          B.truth.insert(B.truth.end(),tru.qual.begin(),tru.qual.end());
        }
      const uint8_t *code; int64_t clen;
      P.fetch(id,&code,&clen);
      B.headers.push_back(header);
      B.id.push_back(id);
      B.seq.insert(B.seq.end(),fx.seq.begin(),fx.seq.end());
      B.code.insert(B.code.end(),code,code+clen);
      B.soff.push_back(B.soff.back()+rlen);
      B.poff.push_back(B.poff.back()+(rlen > Km1 ? rlen-Km1 : 0));
      B.coff.push_back(B.coff.back()+clen);
      if (B.soff.back() >= BATCH_BASES) flush();
    }
  flush();
  if (fclose(out) != 0) die("%s: Cannot write %s\n",PROG,out_path.c_str());

  if (truth_path)
    { if (tru.next() >= 0)
        die("# seqs in %s < # seqs in %s\n",out_path.c_str(),truth_path);
      AccTotals T;
      if (D.acc) T = acc_totals(D.acc);
      print_acc_report(stdout,T);
      fflush(stdout);
    }
  if (D.acc) cp_acc_destroy(D.acc);
  if (D.ws) cp_workspace_destroy(D.ws);
  return 0;
}

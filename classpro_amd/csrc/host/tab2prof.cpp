// tab2prof.cpp -- the profiles of a read set RELATIVE to a FASTK k-mer table: what `FastK -p:<table> <source>` leaves,
// looked up on the GPU in the sorted table itself, with no counting pass and no hash table.
//
//   tab2prof [-v] [-C] [-T<int(4)>] [-b<int(67108864)>] [-N<out_root>] <table>[.ktab] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// Writes <out_root>.prof, .<out_root>.pidx.1..n and .<out_root>.prof.1..n (layout: classpro_amd/fastk.py; nparts =
// min(T, reads), prof_writer.h); no .hist, as FastK writes none for -p:.  out_root defaults to the source's path and root
// plus ".rel".  K comes from the table's stub.  The table may be FastK's own, a Logex product, `kprof -t` or a class
// table of class2ktab; the source is found as kprof finds it.
// The table goes up in pieces of TAB_RANGE entries through one device buffer into cp_kmer_sorted_load_records and is
// checked there (cp_kmer_sorted_load_end: strictly ascending keys; ktab_upload.h); the reads then go through in
// batches of -b bases, one cp_kmer_sorted_profiles each ("Sorted k-mers as input" in include/classpro_amd.h): a cell is min(count, 32767) of
// the canonical k-mer in the table, 0 when it is absent or holds a byte other than upper-case A C G T.  The -T host
// threads encode the cells with cp_encode_profile.
//   -C  also writes <out_root>.class with the labels of prof2class's rule (0 -> E, 1 -> H, 2 -> D, >= 3 -> R after K-1
//       'N'): cp_threshold_labels with thresholds 1 2 3 on the cells still in HBM, the labels come down packed and the
//       records are written through class_record.h.  So `kprof -t1 genome && tab2prof -C genome reads` leaves what
//       `genome2class -p genome reads` leaves for an upper-case genome, including the `rlen > 60000` error for FASTX.
//   -b  bases per device batch.
//   -v  one line on stderr: table entries, minval, table parts, reads, bases, profile parts, cells present / absent /
//       with other bytes.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tab2prof <usage line>                                                  wrong number of arguments
//   tab2prof: -<c> is an illegal option
//   tab2prof: -<c> '<text>' argument is not an integer
//   tab2prof: Number of threads must be positive (<n>)                            -T below 1
//   tab2prof: Bases per device batch must be positive (<n>)                       -b below 1
//   the lines of ktab_reader.h                                                    a table that cannot be read as one
//   tab2prof: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file           the source
//   tab2prof: Cannot open <path> for 'w'                                          <out_root>.prof, with -C <out_root>.class
#include "gpu_tool.h"
#include "read_source.h"
#include "prof_writer.h"
#include "ktab_upload.h"
#include "thread_pool.h"

static const char *USAGE = "[-v] [-C] [-T<int(4)>] [-b<int(67108864)>] [-N<out_root>]\n"
                           "                <table>[.ktab] <source>[.db|.dam|.f[ast][aq][.gz]]";

struct Batch
  { std::vector<std::string> headers;                                // -C only
    std::vector<char> seq;
    std::vector<int64_t> soff{0}, poff{0}, koff{0};                  // bases, profile cells, packed label bytes
    void clear() { headers.clear(); seq.clear(); soff.assign(1,0); poff.assign(1,0); koff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

int main(int argc, char **argv)
{ PROG = "tab2prof";
  bool verbose = false, want_class = false;
  int nthreads = 4, batch_bases = 64 << 20;
  std::string out_root;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-')
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else if (a[k] == 'C') want_class = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'N': out_root = a+2; break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);

  KtabReader tab;
  tab.open(pos[0]);
  const int K = tab.K, Km1 = K-1;
  Source S;
  std::string dir, root;
  if (!S.find(pos[1],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[1].c_str());
  if (out_root.empty()) out_root = dir+"/"+root+".rel";
  const std::string odir = path_to(out_root), oname = root_of(out_root,"");
  const std::string stub_path = odir+"/"+oname+".prof", class_path = odir+"/"+oname+".class";
  const bool stub_fresh = access(stub_path.c_str(),F_OK) != 0;
  FILE *fs = fopen(stub_path.c_str(),"wb");
  if (!fs) die("%s: Cannot open %s for 'w'\n",PROG,stub_path.c_str());
  FILE *out = nullptr;
  if (want_class && !(out = fopen(class_path.c_str(),"w")))
    { fclose(fs);
      if (stub_fresh) unlink(stub_path.c_str());
      die("%s: Cannot open %s for 'w'\n",PROG,class_path.c_str());
    }
  S.open();
  std::vector<char> obuf(want_class ? (size_t)1 << 22 : 0);
  if (want_class) setvbuf(out,obuf.data(),_IOFBF,obuf.size());
  int64_t nreads_known = 0;                                          // the parts are cut by read number
  if (S.is_db) nreads_known = S.db.nreads;
  else
    { while (S.next()) nreads_known++;
      S.rewind();
    }

  // ---- the table, up in pieces and checked ----
  HCHK(hipSetDevice(0));
  int rc;
  cp_kmer_sorted *T;
  { DevBuf<uint8_t> d_rec;
    T = upload_ktab(tab,d_rec);
    d_rec.release();
  }

  // ---- the reads ----
  static const int32_t THRES[3] = { 1, 2, 3 };                       // prof2class.c:241-254
  DevBuf<char> d_seq;
  DevBuf<uint8_t> d_pack;
  DevBuf<int64_t> d_soff, d_poff, d_koff;
  DevBuf<uint16_t> d_prof;
  int64_t *d_tally = nullptr;
  HCHK(hipMalloc((void **)&d_tally,3*sizeof(int64_t)));
  HCHK(hipMemset(d_tally,0,3*sizeof(int64_t)));
  const int nparts = (int)std::min<int64_t>(nthreads,nreads_known);
  ProfWriter W;
  W.open(fs,stub_path,K,nparts,nreads_known,odir,oname);
  ThreadPool pool(nthreads);
  Batch B;
  std::vector<uint8_t> h_pack;
  std::vector<uint16_t> h_prof;
  std::vector<char> h_lab;
  std::vector<std::vector<uint8_t>> code((size_t)nthreads);          // per thread: the profile codes of its reads
  int64_t nreads = 0, nbases = 0;
  auto flush = [&]()
    { const int n = B.n();
      if (n == 0) return;
      const int64_t bases = B.soff.back(), cells = B.poff.back(), pbytes = B.koff.back();
      d_seq.need(B.seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,B.seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(B.soff);
      d_poff.up(B.poff);
      d_prof.need((size_t)cells+8);
      rc = cp_kmer_sorted_profiles(T,1,d_seq.p,d_soff.p,d_poff.p,n,bases,d_prof.p,d_tally,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_profiles");
      if (want_class)
        { d_koff.up(B.koff);
          d_pack.need((size_t)pbytes+8);
          rc = cp_threshold_labels(K,THRES,d_prof.p,d_poff.p,d_soff.p,n,bases,nullptr,d_pack.p,d_koff.p,nullptr,nullptr);
          if (rc != CP_OK) cp_die(rc,"cp_threshold_labels");
          h_pack.resize((size_t)pbytes+1);
          if (pbytes > 0) HCHK(hipMemcpy(h_pack.data(),d_pack.p,(size_t)pbytes,hipMemcpyDeviceToHost));
          h_lab.resize((size_t)bases+1);
        }
      h_prof.resize((size_t)cells+1);
      if (cells > 0) HCHK(hipMemcpy(h_prof.data(),d_prof.p,(size_t)cells*2,hipMemcpyDeviceToHost));
      HCHK(hipDeviceSynchronize());
      W.clen.assign((size_t)n,0);
      const int nt = std::min(nthreads,n);
      pool.parallel_for(nt,[&](int64_t t)                            // thread t: a contiguous range of the batch's reads
        { const int r0 = (int)((int64_t)n*t/nt), r1 = (int)((int64_t)n*(t+1)/nt);
          std::vector<uint8_t> &c = code[(size_t)t];
          c.resize((size_t)(2*(B.poff[(size_t)r1]-B.poff[(size_t)r0])+2*(r1-r0)+2));
          int64_t o = 0;
          for (int r = r0; r < r1; r++)
            { const int64_t s = B.soff[(size_t)r], len = B.soff[(size_t)r+1]-s;
              if (want_class && len > 0)
                { const int e = cp_unpack_labels(h_pack.data()+B.koff[(size_t)r],(int)len,K,h_lab.data()+s);
                  if (e != CP_OK) cp_die(e,"cp_unpack_labels");
                }
              const int64_t np = B.poff[(size_t)r+1]-B.poff[(size_t)r];
              const int64_t l = cp_encode_profile(h_prof.data()+B.poff[(size_t)r],(int)np,c.data()+o,(int64_t)c.size()-o);
              if (l < 0) cp_die((int)l,"cp_encode_profile");
              W.clen[(size_t)r] = l;
              o += l;
            }
        });
      for (int t = 0; t < nt; t++)
        W.append((int)((int64_t)n*t/nt),(int)((int64_t)n*(t+1)/nt),code[(size_t)t].data());
      if (want_class)
        { for (int r = 0; r < n; r++)
            { const int64_t s = B.soff[(size_t)r], len = B.soff[(size_t)r+1]-s;
              write_class_record(out,B.headers[(size_t)r],B.seq.data()+s,(size_t)len,h_lab.data()+s,(size_t)len);
            }
          if (ferror(out)) die("%s: Cannot write %s\n",PROG,class_path.c_str());
        }
      B.clear();
    };

  const int rlen_max = S.is_db ? S.db.maxlen : CLASS_FASTX_RLEN_MAX;
  while (S.next())
    { const int64_t rlen = (int64_t)S.seq.size();
      if (nreads >= nreads_known) die("%s: %s changed while it was read\n",PROG,S.path.c_str());
      if (want_class && rlen > rlen_max)                             // prof2class.c:154-160
        { flush();
          fflush(out);
          die("rlen (%d) > rlen_max (%d)\n",(int)rlen,rlen_max);
        }
      if (want_class) B.headers.push_back(S.header);
      B.seq.insert(B.seq.end(),S.seq.begin(),S.seq.end());
      B.soff.push_back(B.soff.back()+rlen);
      B.poff.push_back(B.poff.back()+(rlen > Km1 ? rlen-Km1 : 0));
      B.koff.push_back(B.koff.back()+((rlen+3) >> 2));
      nreads++;
      nbases += rlen;
      if (B.soff.back() >= batch_bases) flush();
    }
  flush();
  if (nreads != nreads_known) die("%s: %s changed while it was read\n",PROG,S.path.c_str());
  if (want_class && fclose(out) != 0) die("%s: Cannot write %s\n",PROG,class_path.c_str());
  W.close();

  int64_t tally[3];
  HCHK(hipMemcpy(tally,d_tally,sizeof(tally),hipMemcpyDeviceToHost));
  if (verbose)
    fprintf(stderr,"%lld table entries, minval %d, %d table parts, %lld reads, %lld bases, %d profile parts, "
                   "%lld cells present, %lld absent, %lld with other bytes\n",(long long)tab.entries,tab.minval,tab.nparts,
            (long long)nreads,(long long)nbases,nparts,(long long)tally[0],(long long)tally[1],(long long)tally[2]);
  HCHK(hipFree(d_tally));
  cp_kmer_sorted_destroy(T);
  return 0;
}

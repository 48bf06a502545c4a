// class2cns.cpp -- per-k-mer label consensus and consistency of a .class file.
//
//   class2cns [-v] [-c] [-u] [-x] [-C<out.class>] <estimate>.class <fastk_root>[.prof]
//
// Without -u, -x or -C this is the reference's tool (src/class2cns.c:15-78): one line "KMER L" per k-mer position
// (i in [K-1, rlen), K from the .prof stub), the input of scripts/naive_consensus.sh's `sort | uniq -c`.  That mode
// runs on the host only and never touches the GPU.  The flags replace the rest of that pipeline with the device
// table of include/classpro_amd.h (cp_kmer_table_*), on GPU 0:
//   -u  the aggregated table, "%7ld KMER L" per (k-mer, label) with a count > 0, in key order then label order
//       D < E < H < R: byte for byte `class2cns est.class root | LC_ALL=C sort | uniq -c` when every k-mer is made
//       of upper-case A C G T (the table skips other k-mers).
//   -x  "Overall consistency = <v>", the harmonic mean of agg2cons.py's most-common fraction, <v> printed as the
//       shortest string that reads back as the same double (Python's repr).
//   -C  a second pass writes <out.class>: the input's headers and sequences, the consensus labels (tie: R > D > H > E).
//   -c  canonical k-mers (a k-mer and its reverse complement share one entry) for -u, -x and -C; under -u each line
//       then carries the canonical k-mer's text.
//   -v  a summary on stderr: distinct, unanimous and skipped k-mers, table size.
// The batches of records and the table's fill are class_batch.h's, shared with class2ktab; -C walks the file a second
// time through the same buffers.
#include <charconv>
#include <cmath>
#include "class_batch.h"

static const char *USAGE = "[-v] [-c] [-u] [-x] [-C<out.class>] <estimate>.class <fastk_root>[.prof]";

static std::string kmer_text(uint64_t hi, uint64_t lo, int K)
{ std::string s((size_t)K,'A');
  for (int i = 0; i < K; i++)                                // base i from the start: key bits 2(K-1-i)+1 .. 2(K-1-i)
    { const int b = 2*(K-1-i);
      const unsigned v = b >= 63 ? (unsigned)(hi >> (b-63)) & 3 : b == 62 ? (unsigned)((lo >> 62) | (hi << 1)) & 3
                                                                          : (unsigned)(lo >> b) & 3;
      s[(size_t)i] = "ACGT"[v];
    }
  return s;
}

static std::string repr_double(double v)
{ char buf[64];
  if (std::isnan(v)) return "nan";
  auto r = std::to_chars(buf,buf+sizeof(buf),v,std::chars_format::fixed);
  std::string s(buf,r.ptr);
  if (s.find('.') == std::string::npos) s += ".0";
  return s;
}

int main(int argc, char **argv)
{ PROG = "class2cns";
  bool verbose = false, canon = false, table = false, cons = false;
  const char *cns_out = nullptr;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] != '-') { pos.push_back(a); continue; }
      if (a[1] == 'C')
        { if (a[2] == '\0') die("%s: -C needs an output path (-C<out.class>)\n",PROG);
          cns_out = a+2;
          continue;
        }
      for (int k = 1; a[k]; k++)                                 // ARG_FLAGS("vcux")
        switch (a[k])
          { case 'v': verbose = true; break;
            case 'c': canon = true; break;
            case 'u': table = true; break;
            case 'x': cons = true; break;
            default: die("%s: -%c is an illegal option\n",PROG,a[k]);
          }
    }
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  const char *cls = pos[0].c_str();
  { FastxReader probe(cls);                                      // class2cns.c:48-52, then 54-62
    if (!probe.f) die("%s: Cannot open %s [errno=%d]\n",PROG,cls,errno);
  }
  Profiles P;
  if (!P.open(pos[1]))
    die("%s: Cannot open %s.prof\n",PROG,pos[1].c_str());
  const int K = P.kmer, Km1 = K-1;

  static char obuf[1 << 22];
  setvbuf(stdout,obuf,_IOFBF,sizeof(obuf));
  if (!table && !cons && !cns_out)                               // the reference's mode, class2cns.c:62-68
    { FastxReader in(cls);
      std::string line;
      while (in.next() >= 0)
        { const std::string &s = in.seq, &q = in.qual;
          const int n = (int)s.size();
          if (n > Km1 && q.size() < s.size())
            die("%s: record %s of %s carries no labels\n",PROG,in.name.c_str(),cls);
          for (int i = Km1; i < n; i++)
            { line.assign(s,(size_t)(i-Km1),(size_t)K);
              line.push_back(' ');
              line.push_back(q[(size_t)i]);
              line.push_back('\n');
              fwrite(line.data(),1,line.size(),stdout);
            }
        }
      fflush(stdout);
      return 0;
    }

  ClassBatch B;
  cp_kmer_stats st;
  cp_kmer_table *T = fill_label_table(cls,K,canon,verbose,B,&st);

  if (table)
    { const int64_t n = cp_kmer_table_export(T,nullptr,nullptr,nullptr,0);
      if (n < 0) cp_die((int)n,"cp_kmer_table_export");
      std::vector<uint64_t> hi((size_t)std::max<int64_t>(n,1)), lo(hi.size());
      std::vector<uint32_t> cnt(4*hi.size());
      const int64_t m = cp_kmer_table_export(T,hi.data(),lo.data(),cnt.data(),n);
      if (m != n) cp_die((int)m,"cp_kmer_table_export");
      static const int ORDER[4] = { 2, 0, 1, 3 };                   // D < E < H < R (counts are stored E, H, D, R)
      char buf[48];
      for (int64_t i = 0; i < n; i++)
        { const std::string km = kmer_text(hi[(size_t)i],lo[(size_t)i],K);
          for (int o = 0; o < 4; o++)
            { const uint32_t c = cnt[(size_t)(4*i+ORDER[o])];
              if (!c) continue;
              snprintf(buf,sizeof(buf),"%7ld ",(long)c);
              fputs(buf,stdout);
              fwrite(km.data(),1,km.size(),stdout);
              fputc(' ',stdout);
              fputc("EHDR"[ORDER[o]],stdout);
              fputc('\n',stdout);
            }
        }
    }
  if (cons)
    fprintf(stdout,"Overall consistency = %s\n",repr_double(st.consistency).c_str());
  fflush(stdout);

  if (cns_out)
    { FILE *out = fopen(cns_out,"w");
      if (!out) die("%s: Cannot open %s for 'w'\n",PROG,cns_out);
      std::vector<char> wbuf(1 << 22);
      setvbuf(out,wbuf.data(),_IOFBF,wbuf.size());
      for_class_batches(cls,B,CLASS_BATCH_BASES,CLASS_BATCH_READS,true,
                        [&](ClassBatch &b, std::vector<std::string> &headers)
        { b.upload();
          int r = cp_kmer_table_consensus(T,b.d_seq,b.d_off,b.nreads,b.nbases,b.d_lab,nullptr);
          if (r != CP_OK) cp_die(r,"cp_kmer_table_consensus");
          HCHK(hipMemcpy(b.h_lab,b.d_lab,b.nbases,hipMemcpyDeviceToHost));
          for (int i = 0; i < b.nreads; i++)
            { const int64_t s = b.h_off[i], n = b.h_off[i+1]-s;
              write_class_record(out,headers[(size_t)i],b.h_seq+s,(size_t)n,b.h_lab+s,(size_t)n);
            }
        });
      const int rc = cp_kmer_table_stats(T,&st);                    // a k-mer missing from the table would show here
      if (rc != CP_OK) cp_die(rc,"cp_kmer_table_consensus");
      if (fclose(out) != 0) die("%s: Cannot write %s\n",PROG,cns_out);
    }
  cp_kmer_table_destroy(T);
  return 0;
}

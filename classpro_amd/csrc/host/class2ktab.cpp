// class2ktab.cpp -- the consensus classes of the k-mers of a .class file as four FASTK k-mer tables.
//
//   class2ktab [-v] [-T<int(4)>] [-t<int(1)>] [-a<int(0)>] [-N<out_root>] <estimate>.class[.gz] <fastk_root>[.prof]
//
// For each class L of E, H, D, R writes <out_root>.<L>.ktab with its parts .<name>.<L>.ktab.1..n beside it and
// <out_root>.<L>.hist (layouts: classpro_amd/fastk.py), <out_root> being the estimate's path without .class or
// .class.gz, or -N.  libfastk's Root() strips only the .ktab suffix, so Open_Kmer_Stream("reads.H") finds the haploid
// k-mers.  K comes from the .prof stub, as in class2cns; the key is always canonical, which is FASTK's key.
// One pass over the .class in device batches on GPU 0 into a label table (class_batch.h fill_label_table, shared with
// class2cns; cp_kmer_table_*, include/classpro_amd.h); cp_kmer_table_stats then ends the run on a label other than
// E/H/D/R, and the batch buffers are given back before the first sort.  Then the per-class histograms
// (cp_kmer_table_class_hist) and, class by class, a sorted snapshot (cp_kmer_table_sort, "Sorted k-mers of a label
// table"), written by ktab_writer.h and destroyed before the next class is sorted.
//   -t  a table holds the k-mers with at least that many occurrences over all labels (1..32767); it is the stub's minval.
//   -a  and those whose consensus label was given to at least that many percent of the occurrences (0..100): 100 keeps
//       the unanimous k-mers.  The test is 100 * max >= a * total in integers.
//   -T  table parts: n = max(1, min(T, entries)), part p holds the entries [entries*p/n, entries*(p+1)/n).  An empty
//       class still gets its stub and one empty part.
//   -v  on stderr a summary (K, positions, distinct, unanimous and skipped k-mers, table size) and one line per class.
// A .hist covers every k-mer of its class, whatever -t and -a say.  A record carries min(occurrences, 32767).  Usage
// errors, inputs that cannot be opened and outputs that cannot be created are reported before the GPU is touched, and
// then nothing is created.
#include "class_batch.h"
#include "ktab_writer.h"

static const char *USAGE = "[-v] [-T<int(4)>] [-t<int(1)>] [-a<int(0)>] [-N<out_root>] <estimate>.class[.gz] <fastk_root>[.prof]";

int main(int argc, char **argv)
{ PROG = "class2ktab";
  bool verbose = false;
  int nthreads = 4, min_total = 1, min_pct = 0;
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
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
          case 'N': out_root = a+2; break;
          case 't': min_total = (int)arg_range(a,"Table cutoff",1,CP_MAX_KMER_CNT); break;
          case 'a': min_pct = (int)arg_range(a,"Agreement",0,100); break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  const char *cls = pos[0].c_str();
  { FastxReader probe(cls);
    if (!probe.f) die("%s: Cannot open %s [errno=%d]\n",PROG,cls,errno);
  }
  Profiles P;
  if (!P.open(pos[1]))
    die("%s: Cannot open %s.prof\n",PROG,pos[1].c_str());
  const int K = P.kmer;
  if (cp_ktab_ibyte(K) == 0)
    die("%s: needs a K-mer length of at least 5 (%d): a k-mer table has one to three prefix bytes\n",PROG,K);
  if (out_root.empty())
    { std::string name = root_of(pos[0],".class.gz");
      if (name == root_of(pos[0],"")) name = root_of(pos[0],".class");
      out_root = path_to(pos[0])+"/"+name;
    }
  const std::string odir = path_to(out_root), oname = root_of(out_root,"");

  // the eight stubs and histograms: every one is created before the GPU is touched, or none is left behind
  static const char LABELS[5] = "EHDR";
  std::string tab_path[4], hist_path[4];
  FILE *ft[4], *fh[4];
  { std::string path[8];
    int fd[8];
    bool fresh[8];
    for (int l = 0; l < 4; l++)
      { path[2*l] = tab_path[l] = odir+"/"+oname+"."+LABELS[l]+".ktab";
        path[2*l+1] = hist_path[l] = odir+"/"+oname+"."+LABELS[l]+".hist";
      }
    for (int i = 0; i < 8; i++)
      { fresh[i] = access(path[i].c_str(),F_OK) != 0;
        fd[i] = open(path[i].c_str(),O_WRONLY|O_CREAT,0666);
        if (fd[i] >= 0) continue;
        for (int j = 0; j < i; j++)
          { close(fd[j]);
            if (fresh[j]) unlink(path[j].c_str());
          }
        die("%s: Cannot open %s for 'w'\n",PROG,path[i].c_str());
      }
    for (int i = 0; i < 8; i++)
      { FILE *f = ftruncate(fd[i],0) == 0 ? fdopen(fd[i],"wb") : nullptr;
        if (!f) die("%s: Cannot open %s for 'w'\n",PROG,path[i].c_str());
        (i & 1 ? fh : ft)[i >> 1] = f;
      }
  }

  // ---- the label table ----
  cp_kmer_stats st;
  cp_kmer_table *T;
  { ClassBatch B;
    T = fill_label_table(cls,K,true,verbose,B,&st);
    B.release();                                                    // the snapshots want the room
  }

  // ---- the histograms: every key of a class ----
  int64_t nkeys[4];
  { std::vector<int64_t> hist((size_t)4*CP_MAX_KMER_CNT);
    int64_t ilow[4], ihigh[4];
    const int rc = cp_kmer_table_class_hist(T,hist.data(),ilow,ihigh);
    if (rc != CP_OK) cp_die(rc,"cp_kmer_table_class_hist");
    for (int l = 0; l < 4; l++)
      { const int64_t *h = hist.data()+(size_t)l*CP_MAX_KMER_CNT;
        nkeys[l] = 0;
        for (int c = 0; c < CP_MAX_KMER_CNT; c++) nkeys[l] += h[c];
        write_hist(fh[l],hist_path[l],K,ilow[l],ihigh[l],h);
      }
  }

  // ---- the tables, one class at a time ----
  KtabWriter W;
  for (int l = 0; l < 4; l++)
    { cp_kmer_sorted *sorted = nullptr;
      const int rc = cp_kmer_table_sort(T,l,min_total,min_pct,nullptr,&sorted);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_table_sort");
      W.write(sorted,K,min_total,nthreads,ft[l],tab_path[l],odir,oname+"."+LABELS[l]);
      cp_kmer_sorted_destroy(sorted);
      if (verbose)
        fprintf(stderr,"%s: class %c: %lld k-mers, %lld table entries (minval %d, agreement %d%%), %lld occurrences, "
                       "%d table parts\n",PROG,LABELS[l],(long long)nkeys[l],(long long)W.entries,min_total,min_pct,
                (long long)st.cns_total[l],W.nparts);
    }
  W.release();
  if (st.n_skipped)
    fprintf(stderr,"%s: %lld k-mer positions skipped (a base other than upper-case A C G T): they are in no table\n",PROG,
            (long long)st.n_skipped);
  cp_kmer_table_destroy(T);
  return 0;
}

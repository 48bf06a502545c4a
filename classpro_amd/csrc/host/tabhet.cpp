// tabhet.cpp -- the heterozygous k-mer pairs of one FASTK k-mer table: every k-mer paired with the k-mers that differ from
// it only at the centre base, on the GPU; the 2-D histogram of the two counts of such pairs (the coverage list a
// smudge-style plot takes) and, on request, the paired k-mers as a table of their own.
//
//   tabhet [-v] [-a] [-t] [-x<int(1000)>] [-y<int(1000)>] [-T<int(4)>] <table>[.ktab][:<lo>-<hi>] [<out_root>]
//
// Prints one line on stdout, always, and nothing else there:
//   tabhet: <keys> k-mers, <pairs> pairs, <unique> unique pairs, <multi> k-mers in more than one pair
// the k-mers in range, all pairs, the pairs whose two members have no other partner, and the k-mers with two or more
// partners (cp_kmer_sorted_het_pairs; "Heterozygous pairs of sorted k-mers" in include/classpro_amd.h).  With <out_root>
// writes <out_root>.het: the line "#a\tb\tpairs", then one line "a\tb\tn" per non-zero cell, a ascending and then b, a <= b
// the two counts of a pair; a last coordinate of -x or -y means "at least".  Without <out_root> no file is created.  Every
// output is created before the GPU is touched, so that a name that cannot be written costs no GPU work; a failure on the
// device after that leaves them behind, empty.  The table may be FastK's own, a Logex product, `kprof -t`, a class table of
// class2ktab or a tabop result; its k-mers are taken to be canonical.
//   :<lo>-<hi>  the count range, exactly as tabop takes it: k-mers outside it count as absent.
//   -a  count all pairs instead of the unique ones.
//   -t  also write <out_root>.ktab with its parts .<name>.ktab.1..n beside it (ktab_writer.h; n = max(1, min(T, entries)))
//       and <out_root>.hist, in kprof's layout: the k-mers that are members of a counted pair, each with its own count.
//       The stub's minval is the input's.  Needs <out_root>.
//   -x -y  the largest a and the largest b with a cell of their own, each in [1, 32767], at most 4194304 cells together.
//   -T  table parts of the result of -t.
//   -v  one line on stderr: K, the entries of the table, the paired k-mers and the seconds of the device call.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabhet <usage line>                                                    wrong number of arguments
//   tabhet: -<c> is an illegal option
//   tabhet: -<c> '<text>' argument is not an integer                              -x, -y, -T
//   tabhet: Number of threads must be positive (<n>)                              -T below 1
//   tabhet: Histogram bounds must lie in [1, 32767] (<x>, <y>)
//   tabhet: Histogram of <n> cells exceeds 4194304
//   tabhet: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   tabhet: -t needs <out_root>
//   the lines of ktab_reader.h                                                    the table
//   tabhet: <out_root>.ktab is the operand: the result needs a name of its own    -t
//   tabhet: Cannot open <path> for 'w'                                            <out_root>.het, .ktab, .hist
#include "tab_out.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] [-a] [-t] [-x<int(1000)>] [-y<int(1000)>] [-T<int(4)>]\n"
                           "              <table>[.ktab][:<lo>-<hi>] [<out_root>]";

static long int_of(const char *arg)
{ char *end;
  const long v = strtol(arg+2,&end,10);
  if (*end != '\0' || arg[2] == '\0')
    die("%s: -%c '%s' argument is not an integer\n",PROG,arg[1],arg+2);
  return v;
}

int main(int argc, char **argv)
{ PROG = "tabhet";
  bool verbose = false, all = false, table = false;
  long xmax = 1000, ymax = 1000;
  int nthreads = 4;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-' && a[1] != '\0')                         // a bare "-" is an operand like any other name
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else if (a[k] == 'a') all = true;
                else if (a[k] == 't') table = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'x': xmax = int_of(a); break;
          case 'y': ymax = int_of(a); break;
          case 'T': nthreads = arg_int(a,"Number of threads",true); break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 1 && pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  if (xmax < 1 || xmax > CP_MAX_KMER_CNT || ymax < 1 || ymax > CP_MAX_KMER_CNT)
    die("%s: Histogram bounds must lie in [1, 32767] (%ld, %ld)\n",PROG,xmax,ymax);
  const int64_t cells = (int64_t)(xmax+1)*(ymax+1);
  if (cells > 4194304) die("%s: Histogram of %lld cells exceeds 4194304\n",PROG,(long long)cells);
  int64_t range[2];
  const std::string name = split_range(pos[0],range);
  if (table && pos.size() != 2) die("%s: -t needs <out_root>\n",PROG);
  KtabReader A;
  A.open(name);
  const int K = A.K;

  // every output is created before the GPU is touched, or none is left behind
  Outputs outs;
  std::string odir, oname, het_path, tab_path, hist_path;
  FILE *fc = nullptr, *ft = nullptr, *fh = nullptr;
  if (pos.size() == 2)
    { odir = path_to(pos[1]);
      oname = root_of(pos[1],"");
      het_path = odir+"/"+oname+".het";
      tab_path = odir+"/"+oname+".ktab";
      hist_path = odir+"/"+oname+".hist";
      if (table) die_if_operand(tab_path,A.stub,"is the operand");
      fc = outs.create(het_path);
      if (table)
        { ft = outs.create(tab_path);
          fh = outs.create(hist_path);
        }
    }

  // ---- the table up, then the pairing ----
  cp_kmer_sorted *T = upload_table(A), *R = nullptr;
  std::vector<int64_t> mat((size_t)cells);
  int64_t tally[CP_HET_WIDTH];
  const auto t0 = std::chrono::steady_clock::now();
  int rc = cp_kmer_sorted_het_pairs(T,range,all ? 0 : 1,(int)xmax,(int)ymax,mat.data(),tally,nullptr,nullptr,table ? &R : nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_het_pairs");
  const double secs = since(t0);
  cp_kmer_sorted_destroy(T);
  printf("%s: %lld k-mers, %lld pairs, %lld unique pairs, %lld k-mers in more than one pair\n",PROG,(long long)tally[CP_HET_KEYS],
         (long long)tally[CP_HET_PAIRS],(long long)tally[CP_HET_UNIQUE],(long long)tally[CP_HET_MULTI]);
  fflush(stdout);

  if (fc)
    { const int ny = (int)ymax+1;
      bool ok = fprintf(fc,"#a\tb\tpairs\n") > 0;
      for (int64_t c = 0; c < cells; c++)
        if (mat[(size_t)c])
          ok = fprintf(fc,"%lld\t%lld\t%lld\n",(long long)(c/ny),(long long)(c%ny),(long long)mat[(size_t)c]) > 0 && ok;
      if (fclose(fc) != 0 || !ok) die("%s: Cannot write %s\n",PROG,het_path.c_str());
    }
  if (table)
    { std::vector<int64_t> hist((size_t)CP_MAX_KMER_CNT);
      int64_t ilow, ihigh;
      rc = cp_kmer_sorted_hist(R,hist.data(),&ilow,&ihigh);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_hist");
      write_hist(fh,hist_path,K,ilow,ihigh,hist.data());
      KtabWriter W;
      W.write(R,K,A.minval,nthreads,ft,tab_path,odir,oname);
      W.release();
      cp_kmer_sorted_destroy(R);
    }
  if (verbose)
    fprintf(stderr,"K %d: %lld entries; %lld paired k-mers, %lld out; xmax %ld, ymax %ld; %.3f s on the device\n",K,
            (long long)A.entries,(long long)tally[CP_HET_PAIRED],(long long)tally[CP_HET_OUT],xmax,ymax,secs);
  return 0;
}

// tabop.cpp -- set algebra on two FASTK k-mer tables: their AND, OR, SUB or XOR as a third table, merged on the GPU.
//
//   tabop [-v] [-T<int(4)>] [-c<left|sum|min|max>] <A>[.ktab][:<lo>-<hi>] <and|or|sub|xor> <B>[.ktab][:<lo>-<hi>] [<out_root>]
//
// Prints one line on stdout, always, and nothing else there:
//   tabop: <x> only in A, <y> only in B, <z> in both, <w> out
// Without <out_root> that is all: nothing is built and no file is created (cp_kmer_sorted_combine with out == NULL).
// With it writes <out_root>.ktab with its parts .<name>.ktab.1..n beside it (ktab_writer.h; n = max(1, min(T, entries)),
// an empty result still gets its stub and one empty part) and <out_root>.hist, the FASTK histogram of the result's
// counts (cp_kmer_sorted_hist) in kprof's layout.  The stub's minval is the smaller of the two inputs' minval: a lower
// bound on every count the result can hold under all four count rules.
// Either table may be FastK's own, a Logex product, `kprof -t`, a class table of class2ktab or an earlier result; both
// must hold k-mers of the same length.  Both go up in pieces through one device buffer (ktab_upload.h) and are checked
// there; the semantics are those of "Set algebra on sorted k-mers" in include/classpro_amd.h.
//   :<lo>-<hi>  after the LAST ':' of an operand: only its k-mers with lo <= count <= hi take part, the others count as
//       absent.  Taken as a range only when it matches [0-9]*-[0-9]*, so a path may hold a ':'; either end may be empty
//       (":5-" is at least 5, ":-7" at most 7).  A count is what the table's record holds: at most 32767.
//   -c  the count of a kept k-mer: left (A's when A has it, otherwise B's; the default), sum, min or max over the tables
//       that have it.  A record holds min(count, 32767).
//   -T  table parts of the result.
//   -v  one line on stderr: K, then entries, minval and parts of A, of B and of the result.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabop <usage line>                                                     wrong number of arguments
//   tabop: -<c> is an illegal option
//   tabop: -<c> '<text>' argument is not an integer
//   tabop: Number of threads must be positive (<n>)                               -T below 1
//   tabop: Count rule must be one of left, sum, min, max (<text>)                 -c
//   tabop: Operator must be one of and, or, sub, xor (<word>)
//   tabop: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    either table
//   tabop: K of <A stub> (<k>) and <B stub> (<k>) differ
//   tabop: <out_root>.ktab is an operand: the result needs a name of its own
//   tabop: Cannot open <path> for 'w'                                             <out_root>.ktab, <out_root>.hist
#include "tab_out.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] [-T<int(4)>] [-c<left|sum|min|max>]\n"
                           "             <A>[.ktab][:<lo>-<hi>] <and|or|sub|xor> <B>[.ktab][:<lo>-<hi>] [<out_root>]";

int main(int argc, char **argv)
{ PROG = "tabop";
  static const char *RULES[4] = { "left", "sum", "min", "max" }, *OPS[4] = { "and", "or", "sub", "xor" };
  bool verbose = false;
  int nthreads = 4, cnt_op = CP_CNT_LEFT, set_op = -1;
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
          case 'c':
            cnt_op = -1;
            for (int k = 0; k < 4; k++)
              if (strcmp(a+2,RULES[k]) == 0) cnt_op = k;
            if (cnt_op < 0) die("%s: Count rule must be one of left, sum, min, max (%s)\n",PROG,a+2);
            break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 3 && pos.size() != 4)
    die("Usage: %s %s\n",PROG,USAGE);
  for (int k = 0; k < 4; k++)
    if (pos[1] == OPS[k]) set_op = k;
  if (set_op < 0) die("%s: Operator must be one of and, or, sub, xor (%s)\n",PROG,pos[1].c_str());
  int64_t range[4];
  const std::string name_a = split_range(pos[0],range), name_b = split_range(pos[2],range+2);
  KtabReader A, B;
  A.open(name_a);
  B.open(name_b);
  if (A.K != B.K) die("%s: K of %s (%d) and %s (%d) differ\n",PROG,A.stub.c_str(),A.K,B.stub.c_str(),B.K);
  const int K = A.K, minval = std::min(A.minval,B.minval);
  const bool build = pos.size() == 4;

  // the stub and the histogram: both are created before the GPU is touched, or neither is left behind
  std::string odir, oname, tab_path, hist_path;
  Outputs outs;
  FILE *ft = nullptr, *fh = nullptr;
  if (build)
    { odir = path_to(pos[3]);
      oname = root_of(pos[3],"");
      tab_path = odir+"/"+oname+".ktab";
      hist_path = odir+"/"+oname+".hist";
      die_if_operand(tab_path,A.stub,"is an operand");
      die_if_operand(tab_path,B.stub,"is an operand");
      ft = outs.create(tab_path);
      fh = outs.create(hist_path);
    }

  // ---- both tables up, then the merge ----
  HCHK(hipSetDevice(0));
  cp_kmer_sorted *TA, *TB, *R = nullptr;
  { DevBuf<uint8_t> d_rec;                                             // one buffer for both, so not upload_table
    TA = upload_ktab(A,d_rec);
    TB = upload_ktab(B,d_rec);
    d_rec.release();
  }
  int64_t tally[4];
  int rc = cp_kmer_sorted_combine(TA,TB,set_op,cnt_op,range,tally,nullptr,build ? &R : nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_combine");
  cp_kmer_sorted_destroy(TA);
  cp_kmer_sorted_destroy(TB);
  printf("%s: %lld only in A, %lld only in B, %lld in both, %lld out\n",PROG,(long long)tally[0],(long long)tally[1],
         (long long)tally[2],(long long)tally[3]);
  fflush(stdout);

  int nparts = 0;
  if (build)
    { std::vector<int64_t> hist((size_t)CP_MAX_KMER_CNT);
      int64_t ilow, ihigh;
      rc = cp_kmer_sorted_hist(R,hist.data(),&ilow,&ihigh);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_hist");
      write_hist(fh,hist_path,K,ilow,ihigh,hist.data());
      KtabWriter W;
      W.write(R,K,minval,nthreads,ft,tab_path,odir,oname);
      W.release();
      nparts = W.nparts;
      cp_kmer_sorted_destroy(R);
    }
  if (verbose)
    fprintf(stderr,"K %d: A %lld entries, minval %d, %d parts; B %lld entries, minval %d, %d parts; "
                   "result %lld entries, minval %d, %d parts\n",K,(long long)A.entries,A.minval,A.nparts,
            (long long)B.entries,B.minval,B.nparts,(long long)tally[3],minval,nparts);
  return 0;
}

// tabcmp.cpp -- the 2-D count comparison of two FASTK k-mer tables: how many k-mers have count a in A and count b in B,
// for every (a, b), merged on the GPU; from it the k-mer QV of an assembly A against its reads B and its completeness.
//
//   tabcmp [-v] [-q] [-x<int(8)>] [-y<int(1000)>] [-w<keys|a|b>] <A>[.ktab][:<lo>-<hi>] <B>[.ktab][:<lo>-<hi>] [<out_root>]
//
// Prints on stdout, always:
//   tabcmp: <x> only in A, <y> only in B, <z> in both
// the sums of column b = 0, of row a = 0 and of the rest of the matrix of distinct k-mers (cp_kmer_sorted_compare_hist with
// CP_CMP_KEYS; "Count comparison of sorted k-mers" in include/classpro_amd.h).  With <out_root> writes <out_root>.cmp: the
// line "#a\tb\t<keys|sumA|sumB>", then one line "a\tb\tn" per non-zero cell of the -w matrix, a ascending and then b (the
// long layout of Merqury's spectra-cn).  A last coordinate of -x or -y means "at least".  Without <out_root> no file is
// created.  The file is created before the GPU is touched, so that a name that cannot be written costs no GPU work; a
// failure on the device after that leaves it behind, empty.  Either table may be FastK's own, a Logex product,
// `kprof -t`, a class table of class2ktab or a tabop result; both must hold k-mers of the same length.  Both go up in pieces through one device buffer (ktab_upload.h).
//   :<lo>-<hi>  the count range of an operand, exactly as tabop takes it: k-mers outside it count as absent.
//   -x -y  the largest a and the largest b with a cell of their own, each in [1, 32767], at most 4194304 cells together.
//   -w  what a cell sums: keys (1 per distinct k-mer, the default), a (the k-mer's count in A) or b (its count in B).
//   -q  a second line, "tabcmp: QV <%.4f> error <%.3e> completeness <%.4f> %": QV and error by cp_kmer_qv from the
//       a-weighted matrix (the k-mers of A that B does not hold, as a share of all of A's), completeness = 100 * both /
//       (both + only in B) from the keys matrix, the share of B's distinct k-mers in range that A holds.  A field whose
//       denominator is 0 (A, or B, has nothing in range) prints nan.  Runs the comparison a second time for the a weights.
//   -v  one line on stderr: K, the entries of both tables, the two bounds and the non-zero cells of the -w matrix.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabcmp <usage line>                                                    wrong number of arguments
//   tabcmp: -<c> is an illegal option
//   tabcmp: -<c> '<text>' argument is not an integer                              -x, -y
//   tabcmp: Histogram bounds must lie in [1, 32767] (<x>, <y>)
//   tabcmp: Histogram of <n> cells exceeds 4194304
//   tabcmp: Weight must be one of keys, a, b (<text>)
//   tabcmp: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    either table
//   tabcmp: K of <A stub> (<k>) and <B stub> (<k>) differ
//   tabcmp: Cannot open <path> for 'w'                                            <out_root>.cmp
#include <cmath>
#include "gpu_tool.h"
#include "ktab_upload.h"
#include "ktab_range.h"                    // split_range: "<path>[:<lo>-<hi>]"

static const char *USAGE = "[-v] [-q] [-x<int(8)>] [-y<int(1000)>] [-w<keys|a|b>]\n"
                           "              <A>[.ktab][:<lo>-<hi>] <B>[.ktab][:<lo>-<hi>] [<out_root>]";

static long int_of(const char *arg)
{ char *end;
  const long v = strtol(arg+2,&end,10);
  if (*end != '\0' || arg[2] == '\0')
    die("%s: -%c '%s' argument is not an integer\n",PROG,arg[1],arg+2);
  return v;
}

int main(int argc, char **argv)
{ PROG = "tabcmp";
  static const char *WEIGHTS[3] = { "keys", "a", "b" }, *HEADS[3] = { "keys", "sumA", "sumB" };
  bool verbose = false, with_qv = false;
  long xmax = 8, ymax = 1000;
  int weight = CP_CMP_KEYS;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-' && a[1] != '\0')                         // a bare "-" is an operand like any other name
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else if (a[k] == 'q') with_qv = true;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'x': xmax = int_of(a); break;
          case 'y': ymax = int_of(a); break;
          case 'w':
            weight = -1;
            for (int k = 0; k < 3; k++)
              if (strcmp(a+2,WEIGHTS[k]) == 0) weight = k;
            if (weight < 0) die("%s: Weight must be one of keys, a, b (%s)\n",PROG,a+2);
            break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2 && pos.size() != 3)
    die("Usage: %s %s\n",PROG,USAGE);
  if (xmax < 1 || xmax > CP_MAX_KMER_CNT || ymax < 1 || ymax > CP_MAX_KMER_CNT)
    die("%s: Histogram bounds must lie in [1, 32767] (%ld, %ld)\n",PROG,xmax,ymax);
  const int64_t cells = (int64_t)(xmax+1)*(ymax+1);
  if (cells > 4194304) die("%s: Histogram of %lld cells exceeds 4194304\n",PROG,(long long)cells);
  int64_t range[4];
  const std::string name_a = split_range(pos[0],range), name_b = split_range(pos[1],range+2);
  KtabReader A, B;
  A.open(name_a);
  B.open(name_b);
  if (A.K != B.K) die("%s: K of %s (%d) and %s (%d) differ\n",PROG,A.stub.c_str(),A.K,B.stub.c_str(),B.K);
  const int K = A.K;

  // the output is created before the GPU is touched
  std::string cmp_path;
  FILE *fc = nullptr;
  if (pos.size() == 3)
    { cmp_path = path_to(pos[2])+"/"+root_of(pos[2],"")+".cmp";
      if (!(fc = fopen(cmp_path.c_str(),"w"))) die("%s: Cannot open %s for 'w'\n",PROG,cmp_path.c_str());
    }

  // ---- both tables up, then one merge per matrix ----
  HCHK(hipSetDevice(0));
  cp_kmer_sorted *TA, *TB;
  { DevBuf<uint8_t> d_rec;
    TA = upload_ktab(A,d_rec);
    TB = upload_ktab(B,d_rec);
    d_rec.release();
  }
  const int ny = (int)ymax+1;
  std::vector<int64_t> mat[3];                             // by weight; only those that are asked for are made
  auto need = [&](int w) -> const std::vector<int64_t> &
    { if (mat[w].empty())
        { mat[w].resize((size_t)cells);
          const int rc = cp_kmer_sorted_compare_hist(TA,TB,range,w,(int)xmax,(int)ymax,mat[w].data(),nullptr);
          if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_compare_hist");
        }
      return mat[w];
    };
  const std::vector<int64_t> &keys = need(CP_CMP_KEYS);
  int64_t only_a = 0, only_b = 0, both = 0;
  for (int64_t c = 0; c < cells; c++)
    (c%ny == 0 ? only_a : c < ny ? only_b : both) += keys[(size_t)c];
  printf("%s: %lld only in A, %lld only in B, %lld in both\n",PROG,(long long)only_a,(long long)only_b,(long long)both);
  if (with_qv)
    { const std::vector<int64_t> &wa = need(CP_CMP_A);
      int64_t a_miss = 0, a_total = 0;
      for (int64_t c = 0; c < cells; c++)
        { a_total += wa[(size_t)c];
          if (c%ny == 0) a_miss += wa[(size_t)c];
        }
      double qv = NAN, err = NAN;
      if (a_total > 0)
        { const int rc = cp_kmer_qv(K,a_miss,a_total,&qv,&err);
          if (rc != CP_OK) cp_die(rc,"cp_kmer_qv");
        }
      const double comp = both+only_b > 0 ? 100.0*(double)both/(double)(both+only_b) : NAN;
      printf("%s: QV %.4f error %.3e completeness %.4f %%\n",PROG,qv,err,comp);
    }
  fflush(stdout);
  const std::vector<int64_t> &out = need(weight);
  cp_kmer_sorted_destroy(TA);
  cp_kmer_sorted_destroy(TB);
  int64_t nonzero = 0;
  for (int64_t c = 0; c < cells; c++) nonzero += out[(size_t)c] != 0;
  if (fc)
    { bool ok = fprintf(fc,"#a\tb\t%s\n",HEADS[weight]) > 0;
      for (int64_t c = 0; c < cells; c++)
        if (out[(size_t)c])
          ok = fprintf(fc,"%lld\t%lld\t%lld\n",(long long)(c/ny),(long long)(c%ny),(long long)out[(size_t)c]) > 0 && ok;
      if (fclose(fc) != 0 || !ok) die("%s: Cannot write %s\n",PROG,cmp_path.c_str());
    }
  if (verbose)
    fprintf(stderr,"K %d: A %lld entries; B %lld entries; xmax %ld, ymax %ld; %lld non-zero cells\n",K,(long long)A.entries,
            (long long)B.entries,xmax,ymax,(long long)nonzero);
  return 0;
}

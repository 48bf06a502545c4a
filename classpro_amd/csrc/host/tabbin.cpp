// tabbin.cpp -- the reads of a source against TWO FASTK k-mer tables at once: per read the k-mer positions that carry a
// key only in A, only in B, in both, the positions with other bytes, how often the A/B markers switch sides along the
// read, and the bin the read falls in.  With A = the k-mers only the mother has and B = those only the father has this is
// trio binning of the child's reads; with the contigs of an assembly as the source, `switches` counts switch errors.
//
//   tabbin [-v] [-u] [-m<int(1)>] [-b<int(67108864)>] [-o<out_root>]
//          <A>[.ktab][:<lo>-<hi>] <B>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// Prints one line per read on stdout, in source order, tab-separated:
//   <ordinal from 1> <length> <nA> <nB> <nBoth> <nOther> <switches> <A|B|U> <the read's .class header without its '@'>
// and always one line on stderr:
//   tabbin: <n> reads, <x> A, <y> B, <z> U, <r> reads with switches
// Either table may be FastK's own, a Logex product, `kprof -t`, a class table of class2ktab or a result of tabop; both
// must hold k-mers of the same length, and they need not be disjoint: a key in both marks neither side.  Both go up in
// pieces through one device buffer (ktab_upload.h) and are checked there.  One cp_kmer_sorted_combine with out == NULL
// gives the numbers of distinct keys only in A and only in B; the source then goes through in batches of -b bases, whole
// reads per batch, one cp_kmer_sorted_read_hits each ("Read hits in two sorted k-mer sets" in include/classpro_amd.h), and
// only the five numbers per read come down.  The call is cp_bin_call's: A when nA / only_a > nB / only_b, B when it is
// the other way round, U for a tie or fewer than -m markers.
//   :<lo>-<hi>  the count range of an operand, as tabop takes it (ktab_range.h).
//   -u  the call compares nA with nB as they are, not divided by the sizes of the two marker sets.
//   -m  the least nA + nB for a call other than U.
//   -b  bases per device batch.
//   -o  also writes <out_root>.A.fasta, .B.fasta and .U.fasta: ">" and that header, then the sequence on one line.  All
//       three are created, even when empty.
//   -v  one more line on stderr: the entries of A and of B, the keys only in A, only in B and in both, bases, batches.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabbin <usage line>                                                    wrong number of arguments
//   tabbin: -<c> is an illegal option
//   tabbin: -<c> '<text>' argument is not an integer
//   tabbin: Minimum number of markers must be positive (<n>)                      -m below 1
//   tabbin: Bases per device batch must be positive (<n>)                         -b below 1
//   tabbin: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    either table
//   tabbin: K of <A stub> (<k>) and <B stub> (<k>) differ
//   tabbin: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file             the source
//   tabbin: Cannot open <path> for 'w'                                            the files of -o
#include "gpu_tool.h"
#include "read_source.h"
#include "ktab_upload.h"
#include "ktab_range.h"

static const char *USAGE = "[-v] [-u] [-m<int(1)>] [-b<int(67108864)>] [-o<out_root>]\n"
                           "              <A>[.ktab][:<lo>-<hi>] <B>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]";

struct Batch
  { std::vector<std::string> headers;
    std::vector<char> seq;
    std::vector<int64_t> soff{0};
    void clear() { headers.clear(); seq.clear(); soff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

int main(int argc, char **argv)
{ PROG = "tabbin";
  bool verbose = false, normalise = true;
  int min_markers = 1, batch_bases = 64 << 20;
  std::string out_root;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; i++)
    { const char *a = argv[i];
      if (a[0] == '-')
        switch (a[1])
        { default:
            for (int k = 1; a[k]; k++)
              { if (a[k] == 'v') verbose = true;
                else if (a[k] == 'u') normalise = false;
                else die("%s: -%c is an illegal option\n",PROG,a[k]);
              }
            break;
          case 'm': min_markers = arg_int(a,"Minimum number of markers",true); break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'o': out_root = a+2; break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 3)
    die("Usage: %s %s\n",PROG,USAGE);
  int64_t range[4];
  const std::string name_a = split_range(pos[0],range), name_b = split_range(pos[1],range+2);
  KtabReader A, B;
  A.open(name_a);
  B.open(name_b);
  if (A.K != B.K) die("%s: K of %s (%d) and %s (%d) differ\n",PROG,A.stub.c_str(),A.K,B.stub.c_str(),B.K);
  Source S;
  std::string dir, root;
  if (!S.find(pos[2],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[2].c_str());

  // the three files of -o: all are created before the GPU is touched, or none is left behind
  static const char BIN[3] = { 'A', 'B', 'U' };
  FILE *fo[3] = { nullptr, nullptr, nullptr };
  std::string opath[3];
  if (!out_root.empty())
    { bool fresh[3];
      for (int k = 0; k < 3; k++)
        { opath[k] = out_root+"."+BIN[k]+".fasta";
          fresh[k] = access(opath[k].c_str(),F_OK) != 0;
          if ((fo[k] = fopen(opath[k].c_str(),"w"))) continue;
          for (int j = 0; j < k; j++)
            { fclose(fo[j]);
              if (fresh[j]) unlink(opath[j].c_str());
            }
          die("%s: Cannot open %s for 'w'\n",PROG,opath[k].c_str());
        }
    }
  S.open();

  // ---- both tables up, then the sizes of the two marker sets ----
  HCHK(hipSetDevice(0));
  cp_kmer_sorted *TA, *TB;
  { DevBuf<uint8_t> d_rec;
    TA = upload_ktab(A,d_rec);
    TB = upload_ktab(B,d_rec);
    d_rec.release();
  }
  int64_t tally[4];
  int rc = cp_kmer_sorted_combine(TA,TB,CP_SET_AND,CP_CNT_LEFT,range,tally,nullptr,nullptr);
  if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_combine");
  const int64_t only_a = tally[0], only_b = tally[1];

  // ---- the reads ----
  DevBuf<char> d_seq;
  DevBuf<int64_t> d_soff, d_hits;
  std::vector<int64_t> h_hits;
  std::vector<char> obuf((size_t)1 << 20);
  setvbuf(stdout,obuf.data(),_IOFBF,obuf.size());
  Batch R;
  int64_t nreads = 0, nbases = 0, nbatches = 0, ncall[3] = { 0, 0, 0 }, nswitched = 0;
  auto flush = [&]()
    { const int n = R.n();
      if (n == 0) return;
      const int64_t bases = R.soff.back();
      d_seq.need(R.seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,R.seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(R.soff);
      d_hits.need((size_t)n*CP_HIT_WIDTH);
      rc = cp_kmer_sorted_read_hits(TA,TB,1,range,d_seq.p,d_soff.p,n,bases,d_hits.p,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_read_hits");
      h_hits.resize((size_t)n*CP_HIT_WIDTH);
      HCHK(hipMemcpy(h_hits.data(),d_hits.p,(size_t)n*CP_HIT_WIDTH*sizeof(int64_t),hipMemcpyDeviceToHost));
      for (int r = 0; r < n; r++)
        { const int64_t *h = h_hits.data()+(size_t)r*CP_HIT_WIDTH;
          const int64_t s = R.soff[(size_t)r], len = R.soff[(size_t)r+1]-s;
          const int call = cp_bin_call(h,only_a,only_b,min_markers,normalise ? 1 : 0);
          const int bin = call == 'A' ? 0 : call == 'B' ? 1 : 2;
          const char *header = R.headers[(size_t)r].c_str()+(R.headers[(size_t)r].empty() ? 0 : 1);
          ncall[bin]++;
          nswitched += h[CP_HIT_SWITCHES] > 0;
          printf("%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%lld\t%c\t%s\n",(long long)(nreads-n+r+1),(long long)len,
                 (long long)h[CP_HIT_A],(long long)h[CP_HIT_B],(long long)h[CP_HIT_BOTH],(long long)h[CP_HIT_OTHER],
                 (long long)h[CP_HIT_SWITCHES],BIN[bin],header);
          if (fo[bin])
            { fputc('>',fo[bin]); fputs(header,fo[bin]); fputc('\n',fo[bin]);
              fwrite(R.seq.data()+s,1,(size_t)len,fo[bin]);
              fputc('\n',fo[bin]);
            }
        }
      nbatches++;
      R.clear();
    };
  while (S.next())
    { const int64_t rlen = (int64_t)S.seq.size();
      R.headers.push_back(S.header);
      R.seq.insert(R.seq.end(),S.seq.begin(),S.seq.end());
      R.soff.push_back(R.soff.back()+rlen);
      nreads++;
      nbases += rlen;
      if (R.soff.back() >= batch_bases || R.n() == INT32_MAX) flush();
    }
  flush();
  fflush(stdout);
  if (ferror(stdout)) die("%s: Cannot write the standard output\n",PROG);
  for (int k = 0; k < 3; k++)
    if (fo[k] && fclose(fo[k]) != 0) die("%s: Cannot write %s\n",PROG,opath[k].c_str());

  fprintf(stderr,"%s: %lld reads, %lld A, %lld B, %lld U, %lld reads with switches\n",PROG,(long long)nreads,
          (long long)ncall[0],(long long)ncall[1],(long long)ncall[2],(long long)nswitched);
  if (verbose)
    fprintf(stderr,"A %lld entries, B %lld entries, %lld only in A, %lld only in B, %lld in both, %lld bases, %lld batches\n",
            (long long)A.entries,(long long)B.entries,(long long)only_a,(long long)only_b,(long long)tally[2],
            (long long)nbases,(long long)nbatches);
  cp_kmer_sorted_destroy(TA);
  cp_kmer_sorted_destroy(TB);
  return 0;
}

// tabfix.cpp -- the sequences of a source with the errors taken out that a FASTK k-mer table can name: every run of k-mers
// the table does not hold (the runs of `tabtrack <table> <source>`) is tried against the candidate edits of "Fixing reads
// from a k-mer table" (include/classpro_amd.h) on the device, and where exactly one edit makes every k-mer around it
// present, it is applied there.  With the table of the reads themselves and `:3-`, say, that is error correction against
// solid k-mers:  kprof -t2 reads && tabfix -oreads reads:3- reads.fasta && kprof reads.fixed.fasta
//
//   tabfix [-v] [-d<int(1)>] [-b<int(67108864)>] [-o<out_root>] <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]
//
// One line, always, on stderr:
//   tabfix: <n> sequences, <g> gaps, <f> fixed (<s> substitutions, <i> insertions removed, <d> deletions filled),
//           <m> ambiguous, <u> unfixed, <o> open, <w> without candidate, <c> clashes                       (one line)
// g the gaps of all sequences, f those of status CP_FIX_ONE, split by their edit (one base for one base, bases removed,
// bases inserted), then the gaps of status MANY, NONE, OPEN, NOCAND and CLASH.
// -o writes two files, both in source order:
//   <out_root>.fixed.fasta   every sequence, fixed or not, under its .class header without the '@', as tabbin writes
//   <out_root>.fixes.tsv     one line per applied fix: <name> <e> <removed bases> <inserted bases>, tab-separated; <name> is
//                            the header up to its first blank, e the ordinal of the first base the fix replaces (or
//                            inserts before), either string may be empty
//
//   :<lo>-<hi>  the count range of the table, as tabop takes it (ktab_range.h): a k-mer outside it counts as absent.
//   -d  the largest number of bases a fix may insert or remove, 0 .. 4; with 0 only substitutions are fixed.
//   -b  bases per device batch, whole sequences per batch: a batch goes out once it holds that many bases.
//   -v  one more line on stderr: the entries of the table, bases in and out, batches, seconds on the device.
//
// Reported on stderr with exit status 1 before the GPU is touched, and then no file is left behind:
//   Usage: tabfix <usage line>                                                    wrong number of arguments
//   tabfix: -<c> is an illegal option
//   tabfix: -<c> '<text>' argument is not an integer
//   tabfix: Largest indel must lie in [0, 4] (<text>)                             -d outside 0 .. 4
//   tabfix: Bases per device batch must be positive (<n>)                         -b below 1
//   tabfix: Count range of <operand> needs 1 <= lo <= hi (<lo>-<hi>)
//   the lines of ktab_reader.h                                                    the table
//   tabfix: Cannot open <name> as a .db|.dam or .f{ast}[aq][.gz] file             the source
//   tabfix: Cannot open <path> for 'w'                                            the files of -o
#include <algorithm>
#include "tab_out.h"
#include "read_source.h"
#include "ktab_range.h"

static const char *USAGE = "[-v] [-d<int(1)>] [-b<int(67108864)>] [-o<out_root>]\n"
                           "              <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]";

struct Batch
  { std::vector<std::string> headers;
    std::vector<char> seq;
    std::vector<int64_t> soff{0};
    void clear() { headers.clear(); seq.clear(); soff.assign(1,0); }
    int n() const { return (int)soff.size()-1; }
  };

int main(int argc, char **argv)
{ PROG = "tabfix";
  bool verbose = false;
  int max_indel = 1, batch_bases = 64 << 20;
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
          case 'd': max_indel = (int)arg_range(a,"Largest indel",0,4); break;
          case 'b': batch_bases = arg_int(a,"Bases per device batch",true); break;
          case 'o': out_root = a+2; break;
        }
      else
        pos.push_back(a);
    }
  if (pos.size() != 2)
    die("Usage: %s %s\n",PROG,USAGE);
  int64_t range[2];
  const std::string name = split_range(pos[0],range);
  KtabReader A;
  A.open(name);
  const int K = A.K;
  Source S;
  std::string dir, root;
  if (!S.find(pos[1],&dir,&root))
    die("%s: Cannot open %s as a .db|.dam or .f{ast}[aq][.gz] file\n",PROG,pos[1].c_str());
  Outputs outs;
  FILE *fasta = nullptr, *tsv = nullptr;
  if (!out_root.empty())
    { fasta = outs.create(out_root+".fixed.fasta");
      tsv = outs.create(out_root+".fixes.tsv");
    }
  S.open();

  cp_kmer_sorted *T = upload_table(A);

  DevBuf<char> d_seq, d_out;
  DevBuf<int64_t> d_soff, d_foff, d_ooff, d_tally;
  DevBuf<cp_kmer_fix> d_fix;
  std::vector<int64_t> h_foff, h_ooff;
  std::vector<cp_kmer_fix> h_fix;
  std::vector<char> h_out;
  Batch R;
  int64_t nseqs = 0, nbases = 0, nout = 0, nbatches = 0;
  int64_t status[CP_FIX_WIDTH] = { 0, 0, 0, 0, 0, 0 }, kind[3] = { 0, 0, 0 };
  double dev_s = 0;
  auto flush = [&]()
    { const int n = R.n();
      if (n == 0) return;
      const int64_t bases = R.soff.back();
      d_seq.need(R.seq.size()+1);
      if (bases > 0) HCHK(hipMemcpy(d_seq.p,R.seq.data(),(size_t)bases,hipMemcpyHostToDevice));
      d_soff.up(R.soff);
      d_foff.need((size_t)n+1);
      d_ooff.need((size_t)n+1);
      d_fix.need(std::max<size_t>(1024,(size_t)(bases/16)));          // a guess: a gap per 16 bases
      const auto t0 = std::chrono::steady_clock::now();
      int64_t total = 0, out_total = 0;
      int rc = cp_kmer_sorted_read_fixes(T,1,range,max_indel,d_seq.p,d_soff.p,n,bases,d_fix.p,(int64_t)d_fix.cap,d_foff.p,&total,
                                         nullptr,nullptr);
      if (rc == CP_EOVERFLOW)                              // the total is exact: once more at that size
        { d_fix.need((size_t)total);
          rc = cp_kmer_sorted_read_fixes(T,1,range,max_indel,d_seq.p,d_soff.p,n,bases,d_fix.p,(int64_t)d_fix.cap,d_foff.p,&total,
                                         nullptr,nullptr);
        }
      if (rc != CP_OK) cp_die(rc,"cp_kmer_sorted_read_fixes");
      d_out.need((size_t)(bases+4*total)+1);
      rc = cp_apply_fixes(d_seq.p,d_soff.p,n,bases,K,d_fix.p,d_foff.p,d_out.p,(int64_t)d_out.cap,d_ooff.p,&out_total,nullptr);
      if (rc != CP_OK) cp_die(rc,"cp_apply_fixes");
      dev_s += since(t0);
      h_foff.resize((size_t)n+1);
      h_ooff.resize((size_t)n+1);
      h_fix.resize((size_t)total);
      h_out.resize((size_t)out_total);
      HCHK(hipMemcpy(h_foff.data(),d_foff.p,((size_t)n+1)*sizeof(int64_t),hipMemcpyDeviceToHost));
      HCHK(hipMemcpy(h_ooff.data(),d_ooff.p,((size_t)n+1)*sizeof(int64_t),hipMemcpyDeviceToHost));
      if (total > 0) HCHK(hipMemcpy(h_fix.data(),d_fix.p,(size_t)total*sizeof(cp_kmer_fix),hipMemcpyDeviceToHost));
      if (out_total > 0) HCHK(hipMemcpy(h_out.data(),d_out.p,(size_t)out_total,hipMemcpyDeviceToHost));
      for (int r = 0; r < n; r++)
        { const char *header = R.headers[(size_t)r].c_str()+(R.headers[(size_t)r].empty() ? 0 : 1);
          const int name_len = (int)strcspn(header," \t");
          const char *s = R.seq.data()+R.soff[(size_t)r];
          for (int64_t k = h_foff[(size_t)r]; k < h_foff[(size_t)r+1]; k++)
            { const cp_kmer_fix &x = h_fix[(size_t)k];
              status[x.status < CP_FIX_WIDTH ? x.status : CP_FIX_NONE]++;
              if (x.status != CP_FIX_ONE) continue;
              kind[x.del == x.nins ? 0 : x.del > x.nins ? 1 : 2]++;
              if (tsv)
                { const int64_t e = x.first+K-1;
                  fprintf(tsv,"%.*s\t%lld\t%.*s\t%.*s\n",name_len,header,(long long)e,(int)x.del,s+e,(int)x.nins,x.ins);
                }
            }
          if (fasta)
            { fputc('>',fasta); fputs(header,fasta); fputc('\n',fasta);
              fwrite(h_out.data()+h_ooff[(size_t)r],1,(size_t)(h_ooff[(size_t)r+1]-h_ooff[(size_t)r]),fasta);
              fputc('\n',fasta);
            }
        }
      nout += out_total;
      nbatches++;
      R.clear();
    };
  while (S.next())
    { const int64_t rlen = (int64_t)S.seq.size();
      R.headers.push_back(S.header);
      R.seq.insert(R.seq.end(),S.seq.begin(),S.seq.end());
      R.soff.push_back(R.soff.back()+rlen);
      nseqs++;
      nbases += rlen;
      if (R.soff.back() >= batch_bases || R.n() == INT32_MAX) flush();
    }
  flush();
  for (const Outputs::Out &o : outs.made)
    if (fclose(o.f) != 0) die("%s: Cannot write %s\n",PROG,o.path.c_str());

  int64_t gaps = 0;
  for (int k = 0; k < CP_FIX_WIDTH; k++) gaps += status[k];
  fprintf(stderr,"%s: %lld sequences, %lld gaps, %lld fixed (%lld substitutions, %lld insertions removed, %lld deletions filled), "
          "%lld ambiguous, %lld unfixed, %lld open, %lld without candidate, %lld clashes\n",PROG,(long long)nseqs,(long long)gaps,
          (long long)status[CP_FIX_ONE],(long long)kind[0],(long long)kind[1],(long long)kind[2],(long long)status[CP_FIX_MANY],
          (long long)status[CP_FIX_NONE],(long long)status[CP_FIX_OPEN],(long long)status[CP_FIX_NOCAND],
          (long long)status[CP_FIX_CLASH]);
  if (verbose)
    fprintf(stderr,"%lld entries, %lld bases in, %lld out, %lld batches, %.3f s on the device\n",(long long)A.entries,
            (long long)nbases,(long long)nout,(long long)nbatches,dev_s);
  cp_kmer_sorted_destroy(T);
  return 0;
}

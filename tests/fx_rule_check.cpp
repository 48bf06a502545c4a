// fx_rule_check.cpp -- classpro_amd/csrc/fx_rule.h on the host, under AddressSanitizer and UBSan: the candidates and
// checked windows of random closed gaps and the apply map over random edit lists, printed for comparison with
// tests/fix_oracle.py, and the apply map over records that hold anything at all, where only the checks of fx_applies stand
// between a walk and an access outside an array.
//
//   fx_rule_check <cases> <seed>
//
// Per gap one line "G K D n i j near" and one line per candidate that exists, "c del nins ins q0 q1" (ins "-" when empty),
// closed by "end".  Per edit list "A K n records", one line "r first status del nins ins" per record, the read, and the
// read as the walks of 64-base chunks put it together, each chunk beginning a walk of its own as a lane does.  Then
// "wild <n>": n lists of random words were walked.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "fx_rule.h"

typedef std::mt19937_64 rng_t;

static int64_t pick(rng_t &r, int64_t lo, int64_t hi) { return lo+(int64_t)(r()%(uint64_t)(hi-lo+1)); }

// the read as the chunks' walks write it; out has exactly the room the scan of the length changes says
static std::string apply(const std::vector<fx_fix> &fix, const std::string &s, int K, int chunk)
{ const int64_t n = (int64_t)s.size(), nf = (int64_t)fix.size();
  std::vector<int64_t> cum((size_t)nf);
  int64_t run = 0;
  for (int64_t k = 0; k < nf; k++) cum[(size_t)k] = run += fx_delta(fix[(size_t)k],0,n,K);
  const int64_t olen = n+run;
  std::vector<char> out((size_t)(olen > 0 ? olen : 0),'#');
  for (int64_t a = 0; a < n; a += chunk)
    { fx_walk w = fx_walk_begin(fix.data(),cum.data(),0,nf,0,n,K,a);
      for (int64_t p = a; p < n && p < a+chunk; p++)
        fx_walk_step(w,fix.data(),p,s[(size_t)p],[&](int64_t o, char ch) { if (o >= 0 && o < olen) out[(size_t)o] = ch; });
    }
  return std::string(out.begin(),out.end());
}

int main(int argc, char **argv)
{ const int cases = argc > 1 ? atoi(argv[1]) : 1000;
  rng_t r(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  for (int ci = 0; ci < cases; ci++)
    { const int K = (int)pick(r,5,63), D = (int)pick(r,0,4);
      const int64_t i = pick(r,1,50), L = pick(r,0,3) ? pick(r,K > 8 ? K-8 : 1,K+5) : pick(r,1,3*K), j = i+L-1;
      const int64_t e = fx_e(i,K), n = j+K+1+(pick(r,0,2) ? pick(r,0,K) : pick(r,0,3));      // closed: j <= n-K-1
      char near[6] = { 0 };
      for (int k = 0; k < 5; k++) near[k] = "ACGT"[pick(r,0,3)];
      printf("G %d %d %lld %lld %lld %s\n",K,D,(long long)n,(long long)i,(long long)j,near);
      const int64_t g = fx_g(i,j,K);
      const int nc = fx_ncand(g,D);
      if (nc < 0 || nc > FX_MAXC) { printf("bad count %d\n",nc); return 1; }
      for (int c = 0; c < nc; c++)
        { const fx_edit x = fx_cand(c,g,D,near);
          if (!fx_exists(e,x.del,n)) continue;
          int64_t q0, q1;
          fx_window(i,K,x.del,x.nins,n,&q0,&q1);
          printf("c %d %d %.*s%s %lld %lld\n",x.del,x.nins,x.nins,x.ins,x.nins ? "" : "-",(long long)q0,(long long)q1);
          for (int64_t q = q0; q <= q1+K-1; q++)           // every base of the window has a source
            { const int64_t v = fx_source(q,e,x.del,x.nins);
              if (v >= n || v < -x.nins) { printf("bad source\n"); return 1; }
            }
        }
      printf("end\n");
    }
  for (int ci = 0; ci < cases; ci++)
    { const int K = (int)pick(r,5,12);
      const int64_t n = pick(r,K+1,400);
      std::string s((size_t)n,'A');
      for (auto &c : s) c = "ACGT"[pick(r,0,3)];
      std::vector<fx_fix> fix;
      int64_t at = 0;                                      // the first base the next edit may touch
      for (int64_t first = pick(r,1,6); first+K-1 < n; first += pick(r,2,40))
        { fx_fix x;
          memset(&x,0,sizeof(x));
          x.first = first; x.last = first+pick(r,0,K); x.read = 0;
          const int64_t e = fx_e(first,K);
          const int how = (int)pick(r,0,9);
          x.status = (uint8_t)(how < 6 ? FX_ONE : how == 6 ? pick(r,0,5) : how == 7 ? FX_OPEN : FX_ONE);
          x.del = (uint8_t)pick(r,0,4); x.nins = (uint8_t)pick(r,0,4);
          for (int k = 0; k < x.nins; k++) x.ins[k] = "acgt"[pick(r,0,3)];
          if (how == 8) x.del = (uint8_t)pick(r,5,255);                         // records that are no edit
          if (how == 9) x.nins = (uint8_t)pick(r,5,255);
          int64_t ee;
          if (fx_applies(x,0,n,K,&ee))
            { if (e < at) x.status = FX_CLASH;                                   // an edit list is disjoint and ascending
              else at = e+x.del;
            }
          fix.push_back(x);
        }
      printf("A %d %lld %zu\n",K,(long long)n,fix.size());
      for (const fx_fix &x : fix)
        printf("r %lld %d %d %d %.*s%s\n",(long long)x.first,x.status,x.del,x.nins,x.nins <= 4 ? x.nins : 0,x.ins,
               (x.nins && x.nins <= 4) ? "" : "-");
      const std::string whole = apply(fix,s,K,64);
      if (whole != apply(fix,s,K,1) || whole != apply(fix,s,K,1 << 20)) { printf("the chunks disagree\n"); return 1; }
      printf("%s\n%s\n",s.c_str(),whole.c_str());
    }
  // records of another world: any words at all, exact sizes on the heap so that one access too far is seen
  int wild = 0;
  for (int ci = 0; ci < cases; ci++, wild++)
    { const int K = (int)pick(r,5,63);
      const int64_t n = pick(r,0,300), nf = pick(r,0,12);
      std::string s((size_t)n,'C');
      std::vector<fx_fix> fix((size_t)nf);
      for (auto &x : fix)
        { uint64_t w[4] = { r(), r(), r(), r() };
          memcpy(&x,w,sizeof(x));
          if (pick(r,0,1)) x.first = pick(r,-5,n+5);
          if (pick(r,0,1)) x.read = 0;
          if (pick(r,0,1)) x.status = FX_ONE;
          if (pick(r,0,1)) { x.del = (uint8_t)pick(r,0,6); x.nins = (uint8_t)pick(r,0,6); }
        }
      (void)apply(fix,s,K,64);
    }
  printf("wild %d\n",wild);
  return 0;
}

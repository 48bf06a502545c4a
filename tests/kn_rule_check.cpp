// kn_rule_check.cpp -- classpro_amd/csrc/kn_rule.h on the host, under AddressSanitizer and UBSan: the rule of "Pruning the
// unitig graph" over random small graphs, printed for comparison with tests/prune_oracle.py, and over arrays that hold
// anything at all, where only the clamps stand between the rule and an access outside an array.
//
//   kn_rule_check <graphs> <seed>
//
// Per graph one line "G K count links max_island max_tip max_bubble" and the lines "loff ...", "link ...", "off ...",
// "flag ...", "weight ...", "why ...".  The graphs are arrays, not de Bruijn graphs: the rule is written on the arrays as
// they are.  Half of them get a planted bubble and a planted fork so that every mark occurs often; a third carry weights
// near 2^62, where a 64-bit product wraps.  Then "wild <n>": n graphs of random words were run through the rule.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "kn_rule.h"

typedef std::mt19937_64 rng_t;

static int64_t pick(rng_t &r, int64_t lo, int64_t hi) { return lo+(int64_t)(r()%(uint64_t)(hi-lo+1)); }

static void put(const char *name, const std::vector<int64_t> &v)
{ printf("%s",name);
  for (int64_t x : v) printf(" %lld",(long long)x);
  printf("\n");
}

int main(int argc, char **argv)
{ const int graphs = argc > 1 ? atoi(argv[1]) : 1000;
  rng_t r(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  for (int gi = 0; gi < graphs; gi++)
    { const int K = (int)pick(r,2,9);
      const int64_t count = pick(r,1,8);
      std::vector<std::vector<int64_t>> adj((size_t)(2*count));
      for (auto &a : adj)
        { const int64_t d = pick(r,0,9), n = d < 3 ? 0 : d < 7 ? 1 : d < 9 ? 2 : 4;
          for (int64_t k = 0; k < n; k++) a.push_back(pick(r,0,2*count-1));
        }
      if (count >= 4 && gi%2 == 0)
        { // a bubble: p -> {2u, 2v} -> y, mirrored; and a fork: both c and d enter the junction of e from dead ends
          const int64_t u = 0, v = 1, p = 4+pick(r,0,1), y = 6+pick(r,0,1);
          adj[2*u] = { y }; adj[2*v] = { y }; adj[2*u+1] = { p^1 }; adj[2*v+1] = { p^1 };
          adj[p] = { 2*u, 2*v };
          if (count >= 7)
            { const int64_t c = 4, d = 5, e = 12+pick(r,0,1);
              adj[2*c] = { e }; adj[2*c+1].clear(); adj[2*d] = { e }; adj[2*d+1].clear();
              adj[e^1] = { 2*c+1, 2*d+1 };
            }
        }
      std::vector<int64_t> loff(1,0), link, off(1,0), weight, why;
      std::vector<uint8_t> flag;
      for (auto &a : adj)
        { for (int64_t t : a) link.push_back(t);
          loff.push_back((int64_t)link.size());
        }
      const bool big = gi%3 == 0;
      for (int64_t u = 0; u < count; u++)
        { off.push_back(off.back()+K+pick(r,0,3));
          flag.push_back((uint8_t)(pick(r,0,9) == 0 ? 1 : 0));
          weight.push_back(big ? ((int64_t)1 << 62)-pick(r,0,2) : pick(r,-1,3));
        }
      kn_graph g{ loff.data(), link.data(), off.data(), flag.data(), weight.data(), count, (int64_t)link.size(), K,
                  pick(r,0,1)*pick(r,K,K+3), pick(r,0,3) ? pick(r,K,K+3) : 0, pick(r,0,3) ? pick(r,K,K+3) : 0 };
      for (int64_t u = 0; u < count; u++) why.push_back(kn_why(u,g));
      printf("G %d %lld %lld %lld %lld %lld\n",K,(long long)count,(long long)link.size(),(long long)g.max_island,
             (long long)g.max_tip,(long long)g.max_bubble);
      put("loff",loff);
      put("link",link);
      put("off",off);
      put("flag",std::vector<int64_t>(flag.begin(),flag.end()));
      put("weight",weight);
      put("why",why);
    }
  // arrays of another call: any words at all, exact sizes on the heap so that one access too far is seen
  int wild = 0;
  for (int gi = 0; gi < graphs; gi++, wild++)
    { const int64_t count = pick(r,1,6), links = pick(r,0,12);
      std::vector<int64_t> loff((size_t)(2*count+1)), link((size_t)links), off((size_t)(count+1)), weight((size_t)count);
      std::vector<uint8_t> flag((size_t)count);
      auto word = [&]() -> int64_t { const int64_t k = pick(r,0,3); return k == 0 ? (int64_t)r() : k == 1 ? pick(r,-3,3) : pick(r,0,2*count+2); };
      for (auto &x : loff) x = word();
      for (auto &x : link) x = word();
      for (auto &x : off) x = pick(r,-40,40);
      for (auto &x : weight) x = word();
      for (auto &x : flag) x = (uint8_t)r();
      kn_graph g{ loff.data(), links ? link.data() : nullptr, off.data(), flag.data(), weight.data(), count, links, 5, 30, 30, 30 };
      for (int64_t u = 0; u < count; u++)
        { const int w = kn_why(u,g);
          if (w < 0 || w > 3) { printf("bad mark %d\n",w); return 1; }
        }
    }
  printf("wild %d\n",wild);
  return 0;
}

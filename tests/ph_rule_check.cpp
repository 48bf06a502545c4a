// ph_rule_check.cpp -- classpro_amd/csrc/ph_rule.h on the host, under AddressSanitizer and UBSan: the link key taken apart
// again, the order word against the order it stands for, the parity algebra along random chains, and ph_forest_host over
// random graphs, printed for comparison with tests/phase_oracle.py.
//
//   ph_rule_check <cases> <seed>
//
// Per graph one line "G nsites min_support nedges", one line "e s t cis trans" per edge in ascending (s, t), then "b" and
// the blocks, "s" and the sides, "t" and the tally cells EDGES .. LARGEST.  Then "rule <n>": n random checks of the small
// functions held.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>
#include "ph_rule.h"

typedef std::mt19937_64 rng_t;

static int64_t pick(rng_t &r, int64_t lo, int64_t hi) { return lo+(int64_t)(r()%(uint64_t)(hi-lo+1)); }

int main(int argc, char **argv)
{ const int cases = argc > 1 ? atoi(argv[1]) : 200;
  rng_t r(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  for (int ci = 0; ci < cases; ci++)
    { const int64_t nsites = pick(r,0,60), want = nsites < 2 ? 0 : pick(r,0,3*nsites);
      const ph_u64 min_support = (ph_u64)pick(r,1,3);
      std::map<std::pair<ph_u64,ph_u64>,std::pair<ph_u64,ph_u64>> seen;
      for (int64_t k = 0; k < want; k++)
        { const ph_u64 a = (ph_u64)pick(r,0,nsites-1), b = (ph_u64)pick(r,0,nsites-1);
          if (a == b) continue;
          const bool big = pick(r,0,19) == 0;              // margins on both sides of the clamp
          seen[{ std::min(a,b), std::max(a,b) }] = { (ph_u64)pick(r,0,big ? 140000 : 5), (ph_u64)pick(r,0,big ? 140000 : 5) };
        }
      std::vector<ph_host_edge> edges;
      for (const auto &kv : seen)
        if (kv.second.first+kv.second.second > 0)
          edges.push_back(ph_host_edge{ kv.first.first, kv.first.second, kv.second.first, kv.second.second });
      std::vector<int64_t> block;
      std::vector<uint8_t> side;
      int64_t tally[PH_WIDTH];
      ph_forest_host(edges,nsites,min_support,block,side,tally);
      printf("G %lld %llu %zu\n",(long long)nsites,min_support,edges.size());
      for (const ph_host_edge &e : edges) printf("e %llu %llu %llu %llu\n",e.s,e.t,e.cis,e.trans);
      printf("b");
      for (int64_t b : block) printf(" %lld",(long long)b);
      printf("\ns");
      for (uint8_t s : side) printf(" %d",(int)s);
      printf("\nt");
      for (int c = PH_EDGES; c <= PH_LARGEST; c++) printf(" %lld",(long long)tally[c]);
      printf("\n");
    }
  int rule = 0;
  for (int ci = 0; ci < cases; ci++, rule++)
    { const ph_u64 s = (ph_u64)pick(r,0,(1ll << 31)-1), t = (ph_u64)pick(r,0,(1ll << 31)-1);
      const unsigned a = (unsigned)pick(r,0,1), b = (unsigned)pick(r,0,1);
      const ph_u64 key = ph_link_key(s,a,t,b);
      if ((key >> 63) || ph_key_s(key) != std::min(s,t) || ph_key_t(key) != std::max(s,t) || ph_key_x(key) != (a ^ b)
          || key != ph_link_key(t,b,s,a) || ph_key_ok(0,key,((ph_u64)1 << 31)) != (s != t) || ph_key_ok(1,key,~0ull))
        { printf("bad key\n"); return 1; }
      // the order word: a larger clamped margin first, then the smaller ordinal
      const ph_u64 m1 = (ph_u64)pick(r,1,pick(r,0,1) ? 8 : 200000), m2 = (ph_u64)pick(r,1,pick(r,0,1) ? 8 : 200000);
      const ph_u64 o1 = (ph_u64)pick(r,0,(1ll << 48)-1), o2 = (ph_u64)pick(r,0,(1ll << 48)-1);
      const ph_u64 c1 = std::min<ph_u64>(m1,65535), c2 = std::min<ph_u64>(m2,65535);
      const bool first = c1 > c2 || (c1 == c2 && o1 < o2);
      if ((ph_order(m1,o1) > ph_order(m2,o2)) != first || ph_order(m1,o1) == 0 || ph_order_ordinal(ph_order(m1,o1)) != o1)
        { printf("bad order\n"); return 1; }
      // a chain v0 <- v1 <- ... : hopping to the root adds the parities
      const int len = (int)pick(r,1,40);
      std::vector<ph_u64> word((size_t)len);
      unsigned sum = 0;
      word[0] = ph_word(0,0);
      for (int v = 1; v < len; v++) word[(size_t)v] = ph_word((ph_u64)v-1,(unsigned)pick(r,0,1));
      for (int v = 1; v < len; v++) sum ^= ph_par(word[(size_t)v]);
      ph_u64 w = word[(size_t)len-1];
      while (ph_parent(word[(size_t)ph_parent(w)]) != ph_parent(w)) w = ph_hop(w,word[(size_t)ph_parent(w)]);
      if (ph_parent(w) != 0 || ph_par(w) != sum || ph_hook_parity(a,b,sum) != (a ^ b ^ sum)) { printf("bad parity\n"); return 1; }
    }
  printf("rule %d\n",rule);
  return 0;
}

// ph_rule.h -- the rule of kmer_phase.hip ("Phasing heterozygous sites from reads" in include/classpro_amd.h) as plain
// functions that compile for the host as well, so that the rule can be checked without a device (tests/ph_rule_check.cpp).
//
//   link     ph_link_key: the 63-bit key of two markers (site, allele) of different sites that follow each other in a read,
//            min(s,s') << 32 | max(s,s') << 1 | (a ^ a'); ph_key_s, ph_key_t and ph_key_x take it apart again.
//   class    ph_class: the class of a site pair from its two counts (cis: key bit 0, trans: key bit 1), its sign and margin.
//   order    ph_order: one 64-bit word under which the kept edges are totally ordered, the clamped margin in the top 16
//            bits, then 2^48-1 minus an ordinal that ascends with (s, t).  Which ordinal is the caller's choice as long as
//            it ascends: the device takes the index of the pair's first key in the ascending snapshot, the host the index
//            of the edge in its list.  A kept edge has a margin of at least 1, so its word is never 0.
//   parity   a site's word is parent << 1 | parity, the parity that of the path from the site to its parent.  ph_hop
//            replaces a parent by the parent's parent; ph_hook_parity is the parity of a root that hooks along an edge.
//   forest   ph_forest_host STATES the forest: Kruskal over the kept edges from first to last, then block and side of
//            every site and the conflicts.  The device reaches the same forest by Boruvka rounds: under a strict total
//            order the maximum spanning forest is unique.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

typedef unsigned long long ph_u64;            // one name on the host and on the device

#ifndef CP_HDM
#ifdef __HIPCC__
#define CP_HDM __host__ __device__ __forceinline__
#else
#define CP_HDM inline
#endif
#endif

enum { PH_WEAK = 0, PH_TIED = 1, PH_KEPT = 2 };
// the cells of the forest's tally: cp_phase_forest's CP_PH_*
enum { PH_EDGES = 0, PH_NKEPT = 1, PH_NTIED = 2, PH_NWEAK = 3, PH_FOREST = 4, PH_CONFLICTS = 5, PH_BLOCKS = 6, PH_SINGLE = 7,
       PH_LARGEST = 8, PH_ROUNDS = 9, PH_BAD = 10, PH_WIDTH = 11 };

#define PH_ORD_MASK 0xFFFFFFFFFFFFull      // 2^48 - 1

CP_HDM ph_u64 ph_link_key(ph_u64 s, unsigned a, ph_u64 s2, unsigned a2)
{ const ph_u64 lo = s < s2 ? s : s2, hi = s < s2 ? s2 : s;
  return (lo << 32) | (hi << 1) | (ph_u64)((a ^ a2) & 1u);
}

CP_HDM ph_u64 ph_key_s(ph_u64 key) { return key >> 32; }
CP_HDM ph_u64 ph_key_t(ph_u64 key) { return (key & 0xFFFFFFFFull) >> 1; }
CP_HDM unsigned ph_key_x(ph_u64 key) { return (unsigned)(key & 1u); }

// a key names an edge of a graph of nsites sites: no bit above 62, s < t < nsites
CP_HDM bool ph_key_ok(ph_u64 hi, ph_u64 key, ph_u64 nsites)
{ return hi == 0 && (key >> 63) == 0 && ph_key_s(key) < ph_key_t(key) && ph_key_t(key) < nsites; }

CP_HDM int ph_class(ph_u64 cis, ph_u64 trans, ph_u64 min_support, unsigned *sign, ph_u64 *margin)
{ const ph_u64 w = cis > trans ? cis : trans, l = cis > trans ? trans : cis;
  *sign = trans > cis ? 1u : 0u;
  *margin = w-l;
  return w < min_support ? PH_WEAK : w == l ? PH_TIED : PH_KEPT;
}

CP_HDM ph_u64 ph_order(ph_u64 margin, ph_u64 ordinal)
{ return ((margin < 65535 ? margin : 65535) << 48) | (PH_ORD_MASK-(ordinal & PH_ORD_MASK)); }

CP_HDM ph_u64 ph_order_ordinal(ph_u64 word) { return PH_ORD_MASK-(word & PH_ORD_MASK); }

CP_HDM ph_u64 ph_word(ph_u64 parent, unsigned parity) { return (parent << 1) | (ph_u64)(parity & 1u); }
CP_HDM ph_u64 ph_parent(ph_u64 word) { return word >> 1; }
CP_HDM unsigned ph_par(ph_u64 word) { return (unsigned)(word & 1u); }

// the word of a site whose parent's word is wp: the parent's parent, the two parities added
CP_HDM ph_u64 ph_hop(ph_u64 w, ph_u64 wp) { return (wp & ~(ph_u64)1) | ((w ^ wp) & 1u); }

// a root hooks along an edge of sign `sign` between a site of its own tree (parity ps to the root) and a site of the
// other tree (parity pt to that root): the parity of the root to the other root
CP_HDM unsigned ph_hook_parity(unsigned ps, unsigned sign, unsigned pt) { return (ps ^ sign ^ pt) & 1u; }

// ---- the host statement --------------------------------------------------------------------------------------------
struct ph_host_edge { ph_u64 s, t, cis, trans; };

// edges: distinct site pairs s < t < nsites in ascending (s, t).  block and side get nsites cells, tally PH_WIDTH (PH_ROUNDS
// and PH_BAD stay 0: the first is the device algorithm's, and an edge list holds no bad key).
inline void ph_forest_host(const std::vector<ph_host_edge> &edges, int64_t nsites, ph_u64 min_support,
                           std::vector<int64_t> &block, std::vector<uint8_t> &side, int64_t *tally)
{ struct kept { ph_u64 ord; size_t e; unsigned sign; };
  std::vector<kept> k;
  for (int c = 0; c < PH_WIDTH; c++) tally[c] = 0;
  for (size_t e = 0; e < edges.size(); e++)
    { unsigned sign;
      ph_u64 margin;
      const int cls = ph_class(edges[e].cis,edges[e].trans,min_support,&sign,&margin);
      tally[PH_EDGES]++;
      tally[cls == PH_KEPT ? PH_NKEPT : cls == PH_TIED ? PH_NTIED : PH_NWEAK]++;
      if (cls == PH_KEPT) k.push_back(kept{ ph_order(margin,(ph_u64)e), e, sign });
    }
  std::sort(k.begin(),k.end(),[](const kept &a, const kept &b) { return a.ord > b.ord; });
  std::vector<ph_u64> word((size_t)nsites);              // parent << 1 | parity, roots point at themselves
  for (int64_t v = 0; v < nsites; v++) word[(size_t)v] = ph_word((ph_u64)v,0);
  auto find = [&](ph_u64 v)                              // the root's word as seen from v, the path compressed
    { ph_u64 w = word[(size_t)v];
      while (ph_parent(word[(size_t)ph_parent(w)]) != ph_parent(w)) w = ph_hop(w,word[(size_t)ph_parent(w)]);
      word[(size_t)v] = w;
      return w;
    };
  for (const kept &x : k)
    { const ph_u64 ws = find(edges[x.e].s), wt = find(edges[x.e].t);
      if (ph_parent(ws) == ph_parent(wt)) continue;
      word[(size_t)ph_parent(ws)] = ph_word(ph_parent(wt),ph_hook_parity(ph_par(ws),x.sign,ph_par(wt)));
      tally[PH_FOREST]++;
    }
  std::vector<int64_t> low((size_t)nsites,INT64_MAX), size((size_t)nsites,0);
  for (int64_t v = 0; v < nsites; v++)
    { const size_t r = (size_t)ph_parent(find((ph_u64)v));
      low[r] = std::min(low[r],v);
      size[r]++;
    }
  block.assign((size_t)nsites,0);
  side.assign((size_t)nsites,0);
  for (int64_t v = 0; v < nsites; v++)
    { const ph_u64 w = find((ph_u64)v);
      const size_t r = (size_t)ph_parent(w);
      block[(size_t)v] = low[r];
      side[(size_t)v] = (uint8_t)(ph_par(w) ^ ph_par(find((ph_u64)low[r])));
      if ((size_t)v != r) continue;
      if (size[r] >= 2) { tally[PH_BLOCKS]++; tally[PH_LARGEST] = std::max(tally[PH_LARGEST],size[r]); }
      else tally[PH_SINGLE]++;
    }
  for (const kept &x : k)
    if (x.sign != (unsigned)(side[(size_t)edges[x.e].s] ^ side[(size_t)edges[x.e].t])) tally[PH_CONFLICTS]++;
}

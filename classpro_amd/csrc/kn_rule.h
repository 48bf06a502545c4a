// kn_rule.h -- the rule of kmer_prune.hip ("Pruning the unitig graph" in include/classpro_amd.h) as plain functions that
// compile for the host as well, so that the decisions can be checked without a device (tests/kn_rule_check.cpp).
//
// kn_why(u, g) is a function of the arrays of ONE graph alone: it reads loff, link, off, flag and weight and nothing that
// another lane decides.  Everything read from the arrays is clamped before it is used as an index: an offset into link[]
// to [0, links], an oriented unitig to [0, 2*count), an arc count to [0, 4].  On the arrays of the call that made the graph
// no clamp ever changes a value.
//   loads    a lane's loads come in GROUPS, each group behind one dependent step only: the offsets of an oriented unitig
//            and the (at most four) targets behind them are kn_arcs; the tip rule loads the arcs of x, then those of all
//            y^1 together, then what it needs of all (at most sixteen) competitors together, and decides last; the bubble
//            rule does the same over the (at most four) alternatives.  Nothing is a chain per candidate.
//   order    products of a weight (below 2^63) and a node count (below 2^31) are taken in 128 bits.
#pragma once
#include <stdint.h>

#ifndef CP_HDM
#ifdef __HIPCC__
#define CP_HDM __host__ __device__ __forceinline__
#else
#define CP_HDM inline
#endif
#endif

enum { KN_KEPT = 0, KN_ISLAND = 1, KN_TIP = 2, KN_BUBBLE = 3 };

struct kn_graph
  { const int64_t *loff, *link;            // 2*count+1 offsets, `links` targets
    const int64_t *off;                    // count+1 offsets of the sequences
    const uint8_t *flag;                   // count: bit 0 = circular
    const int64_t *weight;                 // count
    int64_t count, links;
    int K;
    int64_t max_island, max_tip, max_bubble;
  };

struct kn_arcs { int n; int64_t y[4]; };   // the targets of an oriented unitig, clamped; y[k] = -1 for k >= n

CP_HDM int64_t kn_clamp(int64_t v, int64_t n) { return v < 0 ? 0 : v > n-1 ? n-1 : v; }

CP_HDM int kn_deg(const kn_graph &g, int64_t x)
{ const int64_t a0 = kn_clamp(g.loff[x],g.links+1), d = kn_clamp(g.loff[x+1],g.links+1)-a0;
  return (int)(d < 0 ? 0 : d > 4 ? 4 : d);
}

CP_HDM kn_arcs kn_targets(const kn_graph &g, int64_t x)
{ kn_arcs a;
  const int64_t a0 = kn_clamp(g.loff[x],g.links+1);
  a.n = kn_deg(g,x);
  for (int k = 0; k < 4; k++) a.y[k] = k < a.n ? kn_clamp(g.link[a0+k],2*g.count) : -1;
  return a;
}

CP_HDM int64_t kn_bases(const kn_graph &g, int64_t u) { return g.off[u+1]-g.off[u]; }

CP_HDM uint64_t kn_weight(const kn_graph &g, int64_t u) { const int64_t w = g.weight[u]; return w < 0 ? 0 : (uint64_t)w; }

// what the rules read of a unitig, loaded in one go
struct kn_node { int d0, d1; int64_t bases; uint64_t w; bool circ; };

CP_HDM kn_node kn_load(const kn_graph &g, int64_t u)
{ kn_node n;
  n.d0 = kn_deg(g,2*u);
  n.d1 = kn_deg(g,2*u+1);
  n.bases = kn_bases(g,u);
  n.w = kn_weight(g,u);
  n.circ = (g.flag[u] & 1) != 0;
  return n;
}

CP_HDM bool kn_tc(const kn_graph &g, const kn_node &n) { return (n.d0 == 0) != (n.d1 == 0) && n.bases <= g.max_tip; }

// v beats u among the tips of one junction
CP_HDM bool kn_beats(const kn_graph &g, const kn_node &nv, int64_t v, const kn_node &nu, int64_t u)
{ if (!kn_tc(g,nv)) return true;
  if (nv.bases != nu.bases) return nv.bases > nu.bases;    // nodes = bases - K + 1 on both sides
  if (nv.w != nu.w) return nv.w > nu.w;
  return v < u;
}

CP_HDM int kn_why(int64_t u, const kn_graph &g)
{ const kn_node nu = kn_load(g,u);
  if (nu.d0 == 0 && nu.d1 == 0) return nu.bases <= g.max_island ? KN_ISLAND : KN_KEPT;
  if ((nu.d0 == 0) != (nu.d1 == 0))
    { if (!kn_tc(g,nu)) return KN_KEPT;
      const kn_arcs ax = kn_targets(g,nu.d0 ? 2*u : 2*u+1);
      kn_arcs at[4];                                       // the arcs of every y^1: who else enters the junction
      for (int k = 0; k < 4; k++)
        { at[k].n = 0;
          if (k < ax.n && (ax.y[k] >> 1) != u) at[k] = kn_targets(g,ax.y[k] ^ 1);
        }
      kn_node nv[16];
      int64_t v[16];
      for (int k = 0; k < 4; k++)
        for (int j = 0; j < 4; j++)
          { const int q = 4*k+j;
            v[q] = j < at[k].n ? (at[k].y[j] >> 1) : -1;
            if (v[q] == u) v[q] = -1;
            if (v[q] >= 0) nv[q] = kn_load(g,v[q]);
          }
      bool beaten = false;
      for (int q = 0; q < 16; q++)
        if (v[q] >= 0 && kn_beats(g,nv[q],v[q],nu,u)) beaten = true;
      return beaten ? KN_TIP : KN_KEPT;
    }
  if (nu.circ || nu.d0 != 1 || nu.d1 != 1 || nu.bases > g.max_bubble) return KN_KEPT;
  const int64_t y = kn_targets(g,2*u).y[0], t = kn_targets(g,2*u+1).y[0];
  if ((y >> 1) == u || (t >> 1) == u) return KN_KEPT;
  const kn_arcs az = kn_targets(g,t ^ 1);
  const int64_t nodes_u = nu.bases-g.K+1;
  kn_node nv[4];
  kn_arcs fw[4], bw[4];
  for (int k = 0; k < 4; k++)
    { if (k >= az.n || (az.y[k] >> 1) == u) continue;
      nv[k] = kn_load(g,az.y[k] >> 1);
      fw[k] = kn_targets(g,az.y[k]);
      bw[k] = kn_targets(g,az.y[k] ^ 1);
    }
  bool popped = false;
  for (int k = 0; k < 4; k++)
    { if (k >= az.n || (az.y[k] >> 1) == u) continue;
      const int64_t v = az.y[k] >> 1;
      if (nv[k].circ || nv[k].bases > g.max_bubble || fw[k].n != 1 || fw[k].y[0] != y || bw[k].n != 1 || bw[k].y[0] != t) continue;
      const unsigned __int128 a = (unsigned __int128)nv[k].w*(unsigned __int128)(uint64_t)nodes_u;
      const unsigned __int128 b = (unsigned __int128)nu.w*(unsigned __int128)(uint64_t)(nv[k].bases-g.K+1);
      if (a > b || (a == b && v < u)) popped = true;
    }
  return popped ? KN_BUBBLE : KN_KEPT;
}

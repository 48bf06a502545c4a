"""Restatement of "Pruning the unitig graph" (include/classpro_amd.h) in plain Python on the walking graph of
tests/unitig_graph_oracle.py and the where arrays of tests/unitig_oracle.py: nothing of the product is imported, nothing here
clamps, scans or compacts.

  limits   (max_island, max_tip, max_bubble), each in bases; 0 switches a rule off
  why      per unitig: 0 kept, 1 island, 2 tip, 3 bubble
  weight   per unitig, or None: the count sum of its nodes"""
import unitig_graph_oracle as GO
import unitig_oracle as UO

TALLY = ("unitigs", "islands", "tips", "bubbles", "removed_keys", "removed_bases", "kept_keys")
KEPT, ISLAND, TIP, BUBBLE = 0, 1, 2, 3


class Rule:
    """The rule on the arrays of one graph: loff, link (targets), bases, circ, weight."""

    def __init__(self, loff, link, bases, circ, weight, K, limits):
        self.loff, self.link, self.bases, self.circ, self.K = loff, link, bases, circ, K
        self.w = [max(int(x), 0) for x in weight]
        self.isl, self.tip, self.bub = limits
        self.n = len(bases)

    def deg(self, x):
        return self.loff[x + 1] - self.loff[x]

    def T(self, x):
        return self.link[self.loff[x]:self.loff[x + 1]]

    def nodes(self, u):
        return self.bases[u] - self.K + 1

    @staticmethod
    def mul(a, b):
        return a * b                                       # exact: Python integers (a test swaps in a product that wraps)

    def tc(self, u):
        return (self.deg(2 * u) == 0) != (self.deg(2 * u + 1) == 0) and self.bases[u] <= self.tip

    def beats(self, v, u):
        if not self.tc(v):
            return True
        a, b = (self.nodes(v), self.w[v]), (self.nodes(u), self.w[u])
        return a > b or (a == b and v < u)

    def why(self, u):
        d0, d1 = self.deg(2 * u), self.deg(2 * u + 1)
        if d0 == 0 and d1 == 0:
            return ISLAND if self.bases[u] <= self.isl else KEPT
        if (d0 == 0) != (d1 == 0):
            if not self.tc(u):
                return KEPT
            x = 2 * u if d0 else 2 * u + 1
            for y in self.T(x):
                if y >> 1 == u:
                    continue
                for t in self.T(y ^ 1):
                    v = (t ^ 1) >> 1
                    if v != u and self.beats(v, u):
                        return TIP
            return KEPT
        if self.circ[u] or d0 != 1 or d1 != 1 or self.bases[u] > self.bub:
            return KEPT
        y, t = self.T(2 * u)[0], self.T(2 * u + 1)[0]
        if y >> 1 == u or t >> 1 == u:
            return KEPT
        for z in self.T(t ^ 1):
            v = z >> 1
            if (v == u or self.circ[v] or self.bases[v] > self.bub or self.deg(z) != 1 or self.T(z)[0] != y
                    or self.deg(z ^ 1) != 1 or self.T(z ^ 1)[0] != t):
                continue
            a, b = self.mul(self.w[v], self.nodes(u)), self.mul(self.w[u], self.nodes(v))
            if a > b or (a == b and v < u):
                return BUBBLE
        return KEPT

    def all(self):
        return [self.why(u) for u in range(self.n)]


def rule_of(L, limits, weight=None):
    """The Rule of a unitig_graph_oracle.Links."""
    return Rule(L.loff(), [y for _, _, y in L.arcs], [len(u[1]) for u in L.utgs], [u[2] for u in L.utgs],
                [u[3] for u in L.utgs] if weight is None else weight, L.K, limits)


def prune(ents, K, count_range=None, limits=(0, 0, 0), weight=None, L=None):
    """(out ents, why, tally) of one call."""
    L = GO.Links(ents, K, count_range) if L is None else L
    R = rule_of(L, limits, weight)
    why = R.all()
    utg, _ = UO.where(ents, K, count_range, L.utgs)
    out = [e for i, e in enumerate(ents) if utg[i] >= 0 and why[utg[i]] == 0]
    gone = [u for u in range(L.n) if why[u]]
    tally = {"unitigs": L.n, "islands": why.count(ISLAND), "tips": why.count(TIP), "bubbles": why.count(BUBBLE),
             "removed_keys": sum(R.nodes(u) for u in gone), "removed_bases": sum(R.bases[u] for u in gone), "kept_keys": len(out)}
    assert tally["kept_keys"] + tally["removed_keys"] == sum(u >= 0 for u in utg)
    return out, why, tally


def clean(ents, K, count_range=None, limits=(0, 0, 0), rounds=10):
    """The loop of tabclean: (out ents, [tally per round]).  Round 1 takes the range, the later ones none; the loop ends after
    a round that removes nothing or after `rounds` rounds."""
    tallies = []
    for r in range(rounds):
        ents, _, t = prune(ents, K, count_range if r == 0 else None, limits)
        tallies.append(t)
        if t["removed_keys"] == 0:
            break
    return ents, tallies


def text(ents, K, count_range=None, limits=(0, 0, 0), rounds=10):
    """(stdout of tabclean, out ents)."""
    out, tallies = clean(ents, K, count_range, limits, rounds)
    lines = [UO.line(ents, K, count_range).replace("tabunitig:", "tabclean:", 1)]
    for r, t in enumerate(tallies):
        lines.append("tabclean: round %d: %d unitigs, %d islands, %d tips, %d bubbles, %d k-mers removed\n" % (
            r + 1, t["unitigs"], t["islands"], t["tips"], t["bubbles"], t["removed_keys"]))
    lines.append(UO.line(out, K).replace("tabunitig:", "tabclean:", 1))
    keys_in = tallies[0]["kept_keys"] + tallies[0]["removed_keys"] if tallies else sum(
        1 for _, c in ents if count_range is None or ((count_range[0] or 1) <= c <= (count_range[1] or (1 << 63) - 1)))
    lines.append("tabclean: %d k-mers in, %d out, %d rounds\n" % (keys_in, len(out), len(tallies)))
    return "".join(lines), out

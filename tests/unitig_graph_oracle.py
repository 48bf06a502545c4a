"""Restatement of "Links between unitigs" (include/classpro_amd.h) on top of the walking unitigs of tests/unitig_oracle.py:
nothing of the product is imported, nothing here packs words, scans or hooks labels.

  oriented unitig   x = 2u + o: unitig u as spelled (o = 0) or reverse complemented (o = 1)
  end(2u) = p[-1], end(2u+1) = flip(p[0]); start(2u) = p[0], start(2u+1) = flip(p[-1]) for the spelled path p
  arc               (x, c, y): c in out(end(x)) and the successor state is start(y)"""
import unitig_oracle as UO

TALLY = ("links", "dead_ends", "tip_unitigs", "isolated_unitigs", "self", "components", "largest_bases")


class Links:
    def __init__(self, ents, K, count_range=None):
        self.ents, self.K, self.range = ents, K, count_range
        self.g = UO.Graph(ents, K, count_range)
        self.utgs = self.g.unitigs()
        self.n = len(self.utgs)
        starts = {}
        for u, (_, _, _, _, path) in enumerate(self.utgs):
            for x, s in ((2 * u, path[0]), (2 * u + 1, path[-1] ^ 1)):
                assert s not in starts                     # a state starts at most one oriented unitig
                starts[s] = x
        self.arcs = []
        for x in range(2 * self.n):
            path = self.utgs[x >> 1][4]
            e = path[0] ^ 1 if x & 1 else path[-1]
            out = self.g.out(e)
            for c in sorted(out):
                assert out[c] in starts, (x, c)            # every successor of an end is the start of exactly one
                self.arcs.append((x, c, starts[out[c]]))
        parent = list(range(self.n))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        for x, _, y in self.arcs:
            a, b = find(x >> 1), find(y >> 1)
            if a != b:
                parent[max(a, b)] = min(a, b)              # the root is the smallest of its set
        self.comp = [find(u) for u in range(self.n)]

    def loff(self):
        off = [0] * (2 * self.n + 1)
        for x, _, _ in self.arcs:
            off[x + 1] += 1
        for x in range(2 * self.n):
            off[x + 1] += off[x]
        return off

    def tally(self):
        deg = [0] * (2 * self.n)
        for x, _, _ in self.arcs:
            deg[x] += 1
        size = {}
        for u, c in enumerate(self.comp):
            size[c] = size.get(c, 0) + len(self.utgs[u][1])
        return {"links": len(self.arcs), "dead_ends": sum(d == 0 for d in deg),
                "tip_unitigs": sum((deg[2 * u] == 0) != (deg[2 * u + 1] == 0) for u in range(self.n)),
                "isolated_unitigs": sum(deg[2 * u] == 0 and deg[2 * u + 1] == 0 for u in range(self.n)),
                "self": sum((x >> 1) == (y >> 1) for x, _, y in self.arcs),
                "components": len(size), "largest_bases": max(size.values(), default=0)}

    def gfa(self):
        text = ["H\tVN:Z:1.0\n"]
        for u, (_, t, _, kc, _) in enumerate(self.utgs):
            text.append("S\t%d\t%s\tLN:i:%d\tKC:i:%d\tco:i:%d\n" % (u, t, len(t), kc, self.comp[u]))
        for x, _, y in self.arcs:
            text.append("L\t%d\t%s\t%d\t%s\t%dM\n" % (x >> 1, "+-"[x & 1], y >> 1, "+-"[y & 1], self.K - 1))
        return "".join(text).encode()

    def line(self):
        t = self.tally()
        first = UO.line(self.ents, self.K, self.range, self.utgs).replace("tabunitig:", "tabgraph:", 1)
        return first + "tabgraph: %d links, %d dead ends, %d tip unitigs, %d components, largest %d bases\n" % (
            t["links"], t["dead_ends"], t["tip_unitigs"], t["components"], t["largest_bases"])


def links(ents, K, count_range=None):
    return Links(ents, K, count_range).arcs


def components(ents, K, count_range=None):
    return Links(ents, K, count_range).comp


def tally(ents, K, count_range=None):
    return Links(ents, K, count_range).tally()


def gfa(ents, K, count_range=None):
    return Links(ents, K, count_range).gfa()


def line(ents, K, count_range=None):
    return Links(ents, K, count_range).line()

"""Restatement of "Reads through the unitig graph" (include/classpro_amd.h) by walking, on top of the unitigs and the where
arrays of tests/unitig_oracle.py and the arcs of tests/unitig_graph_oracle.py: nothing of the product is imported, nothing
here packs words, scans or adds atomically.

  step      of k-mer position i of a read: OTHER, ABSENT, or (x, q): the oriented unitig and the place in it
  segment   (first, n, x, q, read, flags): a maximal stretch of positions with steps (x, q), (x, q+1), ...; flags 1 = joined
  walk      a maximal chain of a read's segments in which every one but the first is joined"""
import unitig_graph_oracle as GO
import unitig_oracle as UO

OTHER, ABSENT = "other", "absent"
TALLY = ("positions", "present", "absent", "other", "segments", "joined", "walks")
FIELDS = ("first", "n", "x", "q", "read", "flags")


class Paths:
    def __init__(self, ents, K, count_range=None):
        self.K, self.ents, self.range = K, ents, count_range
        self.L = GO.Links(ents, K, count_range)
        self.utgs = self.L.utgs
        self.utg, self.at = UO.where(ents, K, count_range, self.utgs)
        self.ord = {x: i for i, (x, _) in enumerate(ents)}
        self.nodes = [len(u[4]) for u in self.utgs]
        self.loff = self.L.loff()
        self._step = {}                                    # the step of a k-mer string, worked out once

    def oriented(self, x):
        """The sequence of the oriented unitig x."""
        t = self.utgs[x >> 1][1]
        return t if not x & 1 else "".join("TGCA"["ACGT".index(c)] for c in reversed(t))

    def step(self, w):
        """The step of the k-mer string w, by the definition."""
        K = self.K
        if any(c not in UO.BASES for c in w):
            return OTHER
        f = UO.key_of(w)
        X = UO.canon(f, K)
        e = self.ord.get(X)
        if e is None or self.utg[e] < 0:
            return ABSENT
        b, u, k, r = int(f != X), self.utg[e], self.at[e] >> 1, self.at[e] & 1
        return (2 * u + (b ^ r), k if b == r else self.nodes[u] - 1 - k)

    def steps(self, read):
        K, out = self.K, []
        for i in range(len(read) - K + 1):
            w = read[i:i + K]
            if w not in self._step:
                self._step[w] = self.step(w)
            out.append(self._step[w])
        return out

    def segments(self, read, r=0):
        """[(first, n, x, q, read, flags)] of one read; the joins are checked against Link and Arc on the way."""
        st, segs = self.steps(read), []
        for i, s in enumerate(st):
            if s in (OTHER, ABSENT):
                continue
            prev = st[i - 1] if i else ABSENT
            if prev not in (OTHER, ABSENT) and prev[0] == s[0] and prev[1] + 1 == s[1]:
                f, n, x, q, _, fl = segs[-1]
                segs[-1] = (f, n + 1, x, q, r, fl)
                continue
            joined = prev not in (OTHER, ABSENT)
            if joined:
                assert prev[1] == self.nodes[prev[0] >> 1] - 1 and s[1] == 0, (prev, s)
                assert self.arc(prev[0], read[i + self.K - 1]) is not None
                assert self.L.arcs[self.arc(prev[0], read[i + self.K - 1])][2] == s[0]
            segs.append((i, 1, s[0], s[1], r, 1 if joined else 0))
        return segs

    def arc(self, x, base):
        """The ordinal of the arc out of x by the base, or None."""
        for a in range(self.loff[x], self.loff[x + 1]):
            if self.L.arcs[a][1] == UO.BASES.index(base):
                return a
        return None

    def batch(self, reads):
        """(seg_off, segs, tally, cov, support) of a batch of reads."""
        off, segs, t = [0], [], dict.fromkeys(TALLY, 0)
        cov, sup = [0] * len(self.utgs), [0] * len(self.L.arcs)
        for r, read in enumerate(reads):
            st = self.steps(read)
            t["positions"] += len(st)
            t["other"] += sum(s == OTHER for s in st)
            t["absent"] += sum(s == ABSENT for s in st)
            mine = self.segments(read, r)
            for k, (f, n, x, q, _, fl) in enumerate(mine):
                cov[x >> 1] += n
                if fl:
                    sup[self.arc(mine[k - 1][2], read[f + self.K - 1])] += 1
            segs += mine
            off.append(len(segs))
        t["present"] = t["positions"] - t["other"] - t["absent"]
        t["segments"], t["joined"] = len(segs), sum(s[5] for s in segs)
        t["walks"] = t["segments"] - t["joined"]
        return off, segs, t, cov, sup

    def walks(self, segs):
        """The walks of ONE read's segments: [(first, end, [x], path length, q)]."""
        K, out = self.K, []
        for f, n, x, q, _, fl in segs:
            if fl:
                w = out[-1]
                w[1] = f + n + K - 1
                w[2].append(x)
                w[3] += len(self.utgs[x >> 1][1]) - (K - 1)
            else:
                out.append([f, f + n + K - 1, [x], len(self.utgs[x >> 1][1]), q])
        return [tuple(w) for w in out]

    def gaf(self, reads, names):
        text = []
        for read, name in zip(reads, names):
            for f, e, xs, plen, q in self.walks(self.segments(read)):
                path = "".join("%s%d" % ("<" if x & 1 else ">", x >> 1) for x in xs)
                text.append("%s\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t255\n" % (name, len(read), f, e, path, plen, q, q + e - f,
                                                                                 e - f, e - f))
        return "".join(text).encode()

    def gfa(self, reads):
        _, _, _, cov, sup = self.batch(reads)
        text = ["H\tVN:Z:1.0\n"]
        for u, (_, t, _, kc, _) in enumerate(self.utgs):
            text.append("S\t%d\t%s\tLN:i:%d\tKC:i:%d\tco:i:%d\tRC:i:%d\n" % (u, t, len(t), kc, self.L.comp[u], cov[u]))
        for a, (x, _, y) in enumerate(self.L.arcs):
            text.append("L\t%d\t%s\t%d\t%s\t%dM\tRC:i:%d\n" % (x >> 1, "+-"[x & 1], y >> 1, "+-"[y & 1], self.K - 1, sup[a]))
        return "".join(text).encode()

    def lines(self, reads):
        _, _, t, cov, sup = self.batch(reads)
        first = UO.line(self.ents, self.K, self.range, self.utgs).replace("tabunitig:", "tabpath:", 1)
        return first + ("tabpath: %d sequences, %d k-mers, %d on the graph, %d segments, %d walks, %d of %d unitigs touched, "
                        "%d of %d links crossed\n" % (len(reads), t["positions"], t["present"], t["segments"], t["walks"],
                                                     sum(c != 0 for c in cov), len(cov), sum(s != 0 for s in sup), len(sup)))


def rcs(text):
    return "".join("TGCA"["ACGT".index(c)] if c in "ACGT" else c for c in reversed(text))


def properties(K, strings, read, segs, segs_rc):
    """Spelling and Mirror of one read from outputs alone: `strings` the sequences of the unitigs, `segs` the segments of the
    read and `segs_rc` those of its reverse complement, each (first, n, x, q, ...)."""
    for f, n, x, q in (s[:4] for s in segs):
        t = strings[x >> 1] if not x & 1 else rcs(strings[x >> 1])
        assert read[f:f + n + K - 1] == t[q:q + n + K - 1], (f, n, x, q)
    nk = len(read) - K + 1
    mirror = []
    for f, n, x, q in (s[:4] for s in reversed(segs)):
        t = strings[x >> 1]
        nodes = len(t) - K + 1
        mirror.append((nk - f - n, n, x if nodes == 1 and t == rcs(t) else x ^ 1, nodes - q - n))
    assert [tuple(s[:4]) for s in segs_rc] == mirror, read


def check_properties(P, read):
    """Spelling and Mirror of one read on the oracle's own segments."""
    properties(P.K, [u[1] for u in P.utgs], read, P.segments(read), P.segments(rcs(read)))

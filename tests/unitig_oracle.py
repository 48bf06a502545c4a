"""Restatement of "Unitigs of sorted k-mers" (include/classpro_amd.h) over dicts, by walking: nothing of the product is
imported, and nothing here jumps pointers, packs words or scans.

  ents     [(key, count)] ascending by key: the table.  A key is the k-mer as an integer of 2K bits, first base most
           significant, A C G T = 0 1 2 3.  The ordinal of an entry is its place in ents, in range or not.
  state    2i spells the key of entry i, 2i+1 its reverse complement."""
BASES = "ACGT"
TALLY = ("keys", "unitigs", "bases", "circular", "longest", "isolated", "tips", "branching", "arcs")


def key_of(text):
    v = 0
    for ch in text:
        v = v * 4 + BASES.index(ch)
    return v


def text_of(x, K):
    return "".join(BASES[(x >> (2 * (K - 1 - i))) & 3] for i in range(K))


def _rc4(b):
    r = 0
    for _ in range(4):
        r = r * 4 + 3 - (b & 3)
        b >>= 2
    return r


_RC4 = [_rc4(b) for b in range(256)]


def rc(x, K):
    """The reverse complement, four bases at a time; the bases past K come out as T's below the key and are dropped."""
    nb, r = (2 * K + 7) // 8, 0
    for _ in range(nb):
        r = (r << 8) | _RC4[x & 255]
        x >>= 8
    return r >> (8 * nb - 2 * K)


def canon(x, K):
    return min(x, rc(x, K))


def table(seqs, K):
    """The canonical k-mers of strings over A C G T with their counts, as ents."""
    cnt = {}
    for s in seqs:
        for p in range(len(s) - K + 1):
            x = canon(key_of(s[p:p + K]), K)
            cnt[x] = cnt.get(x, 0) + 1
    return sorted(cnt.items())


class Graph:
    def __init__(self, ents, K, count_range=None):
        lo, hi = (None, None) if count_range is None else count_range
        lo, hi = 1 if lo is None else lo, (1 << 63) - 1 if hi is None else hi
        self.K, self.ents, self.mask = K, ents, (1 << (2 * K)) - 1
        self.ord = {x: i for i, (x, c) in enumerate(ents) if lo <= c <= hi}
        self._out = {}

    def spell(self, s):
        x = self.ents[s >> 1][0]
        return rc(x, self.K) if s & 1 else x

    def out(self, s):
        """{c: successor state} of the in state s."""
        if s not in self._out:
            w, res = self.spell(s), {}
            for c in range(4):
                f = ((w << 2) & self.mask) | c
                y = canon(f, self.K)
                if y in self.ord:
                    res[c] = 2 * self.ord[y] + (0 if f == y else 1)
            self._out[s] = res
        return self._out[s]

    def palindromic(self, s):
        x = self.ents[s >> 1][0]
        return x == rc(x, self.K)

    def link(self, s):
        """t with s -> t, or None."""
        o = self.out(s)
        if len(o) != 1:
            return None
        t = next(iter(o.values()))
        if len(self.out(t ^ 1)) != 1 or (t >> 1) == (s >> 1) or self.palindromic(s) or self.palindromic(t):
            return None
        assert next(iter(self.out(t ^ 1).values())) == s ^ 1
        return t

    def back(self, s):
        """t with t -> s, or None."""
        t = self.link(s ^ 1)
        return None if t is None else t ^ 1

    def adjacency(self):
        out = []
        for i, (x, _) in enumerate(self.ents):
            b = 0
            if x in self.ord:
                for c in self.out(2 * i):
                    b |= 1 << c
                for c in self.out(2 * i + 1):
                    b |= 16 << c
            out.append(b)
        return out

    def unitigs(self):
        """[(first state, string, circular, count sum, [states])] in the order of the definition."""
        seen, res = set(), []
        for x, i in sorted(self.ord.items()):
            if i in seen:
                continue
            s, circular = 2 * i, False
            while True:                                    # back to the head, or once round
                p = self.back(s)
                if p is None:
                    break
                if p == 2 * i:
                    circular = True
                    break
                s = p
            if circular:
                s = 2 * i                                  # i is the smallest node not seen, so the smallest of its chain
            path = [s]
            while True:
                t = self.link(path[-1])
                if t is None or t == path[0]:
                    break
                path.append(t)
            if not circular and path[-1] ^ 1 < path[0]:
                path = [t ^ 1 for t in reversed(path)]
            for t in path:
                assert (t >> 1) not in seen
                seen.add(t >> 1)
            text = text_of(self.spell(path[0]), self.K) + "".join(BASES[self.spell(t) & 3] for t in path[1:])
            res.append((path[0], text, circular, sum(self.ents[t >> 1][1] for t in path), path))
        res.sort()
        return res


def adjacency(ents, K, count_range=None):
    return Graph(ents, K, count_range).adjacency()


def unitigs(ents, K, count_range=None):
    return Graph(ents, K, count_range).unitigs()


def where(ents, K, count_range=None, utgs=None):
    """(utg, at) per entry: the unitig and 2 * (place in it) + (1 when spelled reversed); -1 for an entry not in."""
    utgs = unitigs(ents, K, count_range) if utgs is None else utgs
    utg, at = [-1] * len(ents), [-1] * len(ents)
    for u, (_, _, _, _, path) in enumerate(utgs):
        for k, s in enumerate(path):
            utg[s >> 1], at[s >> 1] = u, 2 * k + (s & 1)
    return utg, at


def n50(lengths):
    total, run = sum(lengths), 0
    for x in sorted(lengths, reverse=True):
        run += x
        if 2 * run >= total:
            return x
    return 0


def tally(ents, K, count_range=None, utgs=None, adj=None):
    g = Graph(ents, K, count_range)
    utgs = g.unitigs() if utgs is None else utgs
    adj = g.adjacency() if adj is None else adj
    live = [adj[i] for i in g.ord.values()]
    pop = lambda v: bin(v).count("1")
    return {"keys": len(g.ord), "unitigs": len(utgs), "bases": sum(len(u[1]) for u in utgs),
            "circular": sum(u[2] for u in utgs), "longest": max([len(u[1]) for u in utgs] or [0]),
            "isolated": sum(b == 0 for b in live), "tips": sum(((b & 15) == 0) != ((b >> 4) == 0) for b in live),
            "branching": sum(pop(b & 15) >= 2 or pop(b >> 4) >= 2 for b in live), "arcs": sum(pop(b) for b in live)}


def fasta(utgs):
    return "".join(">%d LN:i:%d KC:i:%d%s\n%s\n" % (u, len(t), kc, " CL:Z:circular" if circ else "", t)
                   for u, (_, t, circ, kc, _) in enumerate(utgs)).encode()


def line(ents, K, count_range=None, utgs=None):
    utgs = unitigs(ents, K, count_range) if utgs is None else utgs
    t = tally(ents, K, count_range, utgs)
    return "tabunitig: %d k-mers, %d unitigs, %d bases, %d circular, longest %d, N50 %d\n" % (
        t["keys"], t["unitigs"], t["bases"], t["circular"], t["longest"], n50([len(u[1]) for u in utgs]))

"""The heterozygous pairs of a k-mer table restated over sets and dicts ("Heterozygous pairs of sorted k-mers" in
include/classpro_amd.h): a table is [(key, count)] of canonical K-mers, key = the bases as a 2K-bit number, first base most
significant.  Imports nothing of the product.  Positions are 0-based from the first base; m = K // 2, m' = K - 1 - m."""
import numpy as np

BIG = (1 << 63) - 1


def revcomp(x, K):
    r = 0
    for _ in range(K):
        r = r * 4 + 3 - (x & 3)
        x >>= 2
    return r


def canon(x, K):
    return min(x, revcomp(x, K))


def positions(K):
    m = K // 2
    return sorted({m, K - 1 - m})


def candidates(x, K):
    """The canonical forms of x with one base replaced at m or m', without x itself: a set."""
    out = set()
    for p in positions(K):
        sh = 2 * (K - 1 - p)
        for c in range(4):
            if c != (x >> sh) & 3:
                out.add(canon((x & ~(3 << sh)) | (c << sh), K))
    out.discard(x)
    return out


def in_keys(ents, count_range=None):
    lo, hi = count_range if count_range is not None else (None, None)
    lo, hi = 1 if lo is None else lo, BIG if hi is None else hi
    return {x: c for x, c in ents if lo <= c <= hi}


_last = [None, None]                                       # the last table asked about, and its answer


def siblings(ents, K, count_range=None):
    """{in key: the set of its siblings}"""
    ask = (ents, K, count_range)
    if _last[0] is None or _last[0][0] is not ents or _last[0][1:] != ask[1:]:
        live = in_keys(ents, count_range)
        _last[:] = [ask, {x: {y for y in candidates(x, K) if y in live} for x in live}]
    return _last[1]


def degrees(ents, K, count_range=None):
    """One degree per entry of the table, 0 for an entry outside the range."""
    sib = siblings(ents, K, count_range)
    return [len(sib[x]) if x in sib else 0 for x, _ in ents]


def pairs(ents, K, count_range=None, unique=True):
    """The counted pairs as sorted [(x, y)], x < y."""
    sib = siblings(ents, K, count_range)
    out = []
    for x, ys in sib.items():
        for y in ys:
            assert x in sib[y], "the relation is symmetric"
            if x < y and (not unique or (len(ys) == 1 and len(sib[y]) == 1)):
                out.append((x, y))
    return sorted(out)


def matrix(ents, K, xmax, ymax, count_range=None, unique=True):
    cnt = dict(ents)
    m = np.zeros((xmax + 1, ymax + 1), np.int64)
    for x, y in pairs(ents, K, count_range, unique):
        a, b = sorted((cnt[x], cnt[y]))
        m[min(a, xmax), min(b, ymax)] += 1
    return m


def members(ents, K, count_range=None, unique=True):
    """The entries that are members of a counted pair, ascending, each with its own count."""
    keep = {k for p in pairs(ents, K, count_range, unique) for k in p}
    return [(x, c) for x, c in ents if x in keep]


def tally(ents, K, count_range=None, unique=True):
    deg = degrees(ents, K, count_range)
    return {"keys": len(in_keys(ents, count_range)), "paired": sum(d >= 1 for d in deg), "multi": sum(d >= 2 for d in deg),
            "pairs": sum(deg) // 2, "unique": len(pairs(ents, K, count_range, True)),
            "out": len(members(ents, K, count_range, unique))}


def line(t):
    return "tabhet: %d k-mers, %d pairs, %d unique pairs, %d k-mers in more than one pair\n" % (
        t["keys"], t["pairs"], t["unique"], t["multi"])


def het_text(mat):
    rows = [b"#a\tb\tpairs\n"]
    for a, b in np.argwhere(mat).tolist():
        rows.append(b"%d\t%d\t%d\n" % (a, b, mat[a, b]))
    return b"".join(rows)


def planted(rng, K, n, top=30):
    """A sparse table with planted pairs: n random canonical seeds; half get a partner at m or m', a tenth a second one.
    Counts in [1, top]."""
    keys = set()
    pos = positions(K)
    for _ in range(n):
        x = canon(rng.getrandbits(2 * K), K)
        keys.add(x)
        u = rng.random()
        for _ in range(0 if u >= 0.5 else 2 if u < 0.1 else 1):
            sh = 2 * (K - 1 - rng.choice(pos))
            keys.add(canon(x ^ (rng.randint(1, 3) << sh), K))
    return [(x, rng.randint(1, top)) for x in sorted(keys)]

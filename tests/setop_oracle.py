"""Dict-and-set restatement of the set algebra on sorted k-mer tables ("Set algebra on sorted k-mers" in
include/classpro_amd.h) over the entries of tests/ktab_oracle.py, [(key, count)] ascending.  Nothing of the product is
imported."""
import numpy as np

BIG = (1 << 63) - 1
RULE = {"left": lambda ca, cb: ca if ca is not None else cb,
        "sum": lambda ca, cb: (ca or 0) + (cb or 0),
        "min": lambda ca, cb: min(c for c in (ca, cb) if c is not None),
        "max": lambda ca, cb: max(c for c in (ca, cb) if c is not None)}
KEEP = {"and": lambda a, b: a and b, "or": lambda a, b: a or b, "sub": lambda a, b: a and not b, "xor": lambda a, b: a != b}


def combine(a, b, op, count="left", a_range=None, b_range=None):
    """(entries, (only_a, only_b, both, out)); a range is (lo, hi), either end None."""
    def side(ents, rng):
        lo, hi = rng or (None, None)
        return {k: c for k, c in ents if (1 if lo is None else lo) <= c <= (BIG if hi is None else hi)}
    A, B = side(a, a_range), side(b, b_range)
    out = [(k, RULE[count](A.get(k), B.get(k))) for k in sorted(set(A) | set(B)) if KEEP[op](k in A, k in B)]
    both = len(set(A) & set(B))
    return out, (len(A) - both, len(B) - both, both, len(out))


def hist(ents):
    """(1, 32767, ilowcnt, ihighcnt, int64[32767]) of the counts, as KmerCounts.hist gives it."""
    h = np.zeros(32767, np.int64)
    for _, c in ents:
        if c > 0:
            h[min(c, 32767) - 1] += 1
    return 1, 32767, int(h[0]), sum(c for _, c in ents if c >= 32767), h

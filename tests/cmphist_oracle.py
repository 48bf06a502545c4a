"""Dict restatement of the 2-D count comparison of two sorted k-mer tables ("Count comparison of sorted k-mers" in
include/classpro_amd.h) over the entries of tests/ktab_oracle.py, [(key, count)] ascending, and of what tabcmp prints from
it.  Nothing of the product is imported."""
import math

import numpy as np

BIG = (1 << 63) - 1
HEAD = {"keys": "keys", "a": "sumA", "b": "sumB"}


def side(ents, rng):
    lo, hi = rng or (None, None)
    return {k: c for k, c in ents if (1 if lo is None else lo) <= c <= (BIG if hi is None else hi)}


def matrix(a, b, xmax, ymax, weight="keys", a_range=None, b_range=None):
    """int64 [xmax+1, ymax+1]; a range is (lo, hi), either end None.  Sums are taken modulo 2^64."""
    A, B = side(a, a_range), side(b, b_range)
    cell = {}
    for k in set(A) | set(B):
        ca, cb = A.get(k, 0), B.get(k, 0)
        at = (min(ca, xmax), min(cb, ymax))
        cell[at] = cell.get(at, 0) + {"keys": 1, "a": ca, "b": cb}[weight]
    m = np.zeros((xmax + 1, ymax + 1), np.int64)
    for (x, y), v in cell.items():
        v &= (1 << 64) - 1
        m[x, y] = v - (1 << 64) if v >> 63 else v
    return m


def tally(keys):
    """(only_a, only_b, both) of a "keys" matrix: column 0, row 0, the rest."""
    return int(keys[:, 0].sum()), int(keys[0, :].sum()), int(keys[1:, 1:].sum())


def qv(K, a_only, a_total):
    """(qv, err) by Merqury's rule."""
    err = 1.0 - math.pow(1.0 - a_only / a_total, 1.0 / K)
    return (math.inf if a_only == 0 else -10.0 * math.log10(err)), err


def completeness(keys):
    _, only_b, both = tally(keys)
    return 100.0 * both / (both + only_b) if both + only_b else math.nan


def cmp_text(m, weight):
    """The bytes of tabcmp's <out_root>.cmp."""
    rows = ["#a\tb\t%s\n" % HEAD[weight]]
    rows += ["%d\t%d\t%d\n" % (x, y, m[x, y]) for x in range(m.shape[0]) for y in range(m.shape[1]) if m[x, y]]
    return "".join(rows).encode()

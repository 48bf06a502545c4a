"""Inputs of tests/test_unrel_round_inputs.py and tests/test_gpu_unrel_round_loads.py, and what the oracle makes of them
(computed once per process): the 1250 reads of tests/unrel_paint_inputs.py, and behind them the few that reach what
those miss of a round of k_classify_unrel_grp -- see `round_paths`.

"Comb" reads: a flat diploid profile with a one-error dip of K positions every 70-110 positions.  The dips are the only
non-fixed intervals, none of them reliable and no two of them index neighbours, so no round of the speculation can end
early: the first sweep's rounds start at the multiples of the slot count and its last round has `nnf % slots` positions.
With more than 128 dips such a read is in the size class with eight slots per round (N > 256).
"""
import functools
import math

import numpy as np

from unrel_paint_inputs import K, READ_LEN, HCOV, DCOV, H_CLS, D_CLS, fixed, update_order
from unrel_paint_inputs import inputs as paint_inputs

REP_COV = DCOV + int(math.sqrt(DCOV) * 5)                  # GLOBAL_COV[REPEAT], ClassPro.c:544-548 (N_SIGMA_RCOV = 5)
SMALL_MAXN = 256                                           # N <= this: four slots per round, above it eight


def comb_reads(seed, teeth):
    rng = np.random.default_rng(seed)
    seqs, profs = [], []
    for n in teeth:
        parts = []
        for _ in range(n):
            parts += [np.full(int(rng.integers(70, 111)), DCOV), np.full(K, int(rng.integers(1, 3)))]
        parts.append(np.full(90, DCOV))
        c = np.concatenate(parts)
        seqs.append(bytes(b"ACGT"[x] for x in rng.integers(0, 4, len(c) + K - 1)))
        profs.append(c.astype(np.uint16))
    return seqs, profs


def extra_reads():
    """Two comb reads per size class, `nnf % slots` != 0 in each.  (Everything else `round_paths` counts the 1250 reads
    reach themselves, their 250 adversarial ones most of it: no generator of tests/adversarial.py makes a read of more
    than 256 intervals whose rounds are known to run to their ends.)"""
    return comb_reads(11, (9, 30, 131, 150))


@functools.lru_cache(maxsize=None)
def inputs():
    """(seqs, profs, recs) as tests/unrel_paint_inputs.py's, the extra reads appended."""
    from oracle.oracle import Oracle
    seqs, profs, recs = paint_inputs()
    e_s, e_p = extra_reads()
    O = Oracle(K, READ_LEN, HCOV, DCOV)
    more = []
    for s, p in zip(e_s, e_p):
        l, r = O.seq_context(s)
        iv = O.find_wall(p, l, r)
        iv2, riv = O.find_rel_intvl(iv, p, l, r)
        _, io, _, _ = O.classify_rel(riv, iv2, len(p))
        more.append(dict(io=io, call=O.classify_unrel(io), lab=O.classify_read(s, p)))
    return seqs + e_s, profs + e_p, recs + more


def round_paths(rec):
    """What one read reaches of a round's paths, counted on the oracle's records (`io`: the intervals as classify_unrel
    gets them, `call`: as it leaves them).  The first update of the first sweep is the last non-fixed interval of the
    update order, and it alone sees exactly the state of `io`; the counts that need a state are taken on it."""
    io, call = rec["io"], rec["call"]
    N = len(io)
    out = dict(n1=int(N == 1), all_fixed=0, repeat_exit=0, no_rel=0, poisson=0, other_class=0, short4=0, short8=0, clash1=0)
    if N == 0:
        return out
    order = update_order(io)
    nnf = len(order)
    out["all_fixed"] = int(nnf == 0)
    if nnf == 0:
        return out
    fx = fixed(io)                                         # the reliable-H and the reliable-D set
    hi = np.maximum(io["cb"], io["ce"]).astype(np.int64)
    out["repeat_exit"] = int(np.any(hi[order] >= REP_COV))
    n_relH, n_relD = int((fx & (io["asgn"] == H_CLS)).sum()), int((fx & (io["asgn"] == D_CLS)).sum())
    first = int(order[-1])
    if hi[first] < REP_COV:
        if n_relH == 0 and n_relD == 0:
            # no reliable interval on either side: every estimate is the class's coverage, dcov the diploid one
            out["no_rel"] = 1
            for s, cov in ((H_CLS, HCOV), (D_CLS, DCOV)):
                sides = []
                for nb, peo, c in ((first - 1, io["peo_b"][first], io["cb"][first]), (first + 1, io["peo_e"][first], io["ce"][first])):
                    er = 0 <= nb < N and io["asgn"][nb] == s and peo != -np.inf
                    sides.append(not er and int(c) > cov)  # no er term, no Skellam term, and est < c: no binomial term
                out["poisson"] |= int(all(sides))
        elif (n_relH == 0) != (n_relD == 0):
            out["other_class"] = 1                         # est_cov of the class without reliable intervals: the other class's
    # no round can end early: no reliable non-fixed interval (neither set changes) and no two index neighbours within
    # a round's slots of each other in the order
    slots = 4 if N <= SMALL_MAXN else 8
    pos = np.full(N, -10 ** 6, np.int64)
    pos[order] = np.arange(nnf)
    nf = ~fx
    both = nf[:-1] & nf[1:]
    near = both & (np.abs(pos[:-1] - pos[1:]) < slots)
    quiet = not np.any(near) and not np.any(nf & (io["is_rel"] != 0))
    if nnf < slots or (quiet and nnf % slots != 0):
        out["short4" if slots == 4 else "short8"] = 1
    # a round that ends at slot 1: index neighbours next to each other in the order, and the class of the one the first
    # sweep takes first (the later one in the order) changes to or from H / D
    a, b = order[1:], order[:-1]                           # the first sweep takes a before b
    hd = lambda x: (x == H_CLS) | (x == D_CLS)
    ch = (io["asgn"][a] != call["asgn"][a]) & (hd(io["asgn"][a]) | hd(call["asgn"][a]))
    out["clash1"] = int(np.any((np.abs(a - b) == 1) & ch))
    return out

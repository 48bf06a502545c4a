"""Inputs of tests/test_unrel_wide_inputs.py and tests/test_gpu_unrel_wide_rounds.py, and what the oracle makes of them
(computed once per process): the 1254 reads of tests/unrel_round_inputs.py, and behind them the few that reach what
those miss of k_classify_unrel_grp with four lanes per slot -- eight slots per round for N <= 256, sixteen above --
see `wide_paths`.

"Comb" reads as tests/unrel_round_inputs.py makes them, with as many teeth as a round has slots, one fewer and one more.
"Fence" reads: flat segments that alternate between the diploid and the haploid coverage, every one of them a reliable
interval that classify_rel settles (fixed), with a few one-error dips as the only non-fixed intervals: more than 256
intervals with fewer non-fixed ones than the size class has slots.
"""
import functools

import numpy as np

from unrel_paint_inputs import K, READ_LEN, HCOV, DCOV, H_CLS, D_CLS, fixed, update_order
from unrel_round_inputs import SMALL_MAXN, comb_reads
from unrel_round_inputs import inputs as round_inputs

SLOTS_SMALL, SLOTS_BIG = 8, 16                             # slots per round of the two size classes
LANES_SMALL = 32                                           # order positions a round of the second sweep looks at (N <= 256)


def fence_reads(seed, shapes):
    """shapes: (segments, dips) per read."""
    rng = np.random.default_rng(seed)
    seqs, profs = [], []
    for nseg, ndip in shapes:
        dips = set(int(x) for x in rng.choice(np.arange(2, nseg - 2), ndip, replace=False))
        parts = []
        for j in range(nseg):
            n = int(rng.integers(44, 60))
            seg = np.full(n, DCOV if j % 2 == 0 else HCOV)
            if j in dips:
                seg[2:2 + K] = int(rng.integers(1, 3))
            parts.append(seg)
        c = np.concatenate(parts)
        seqs.append(bytes(b"ACGT"[x] for x in rng.integers(0, 4, len(c) + K - 1)))
        profs.append(c.astype(np.uint16))
    return seqs, profs


def extra_reads():
    c_s, c_p = comb_reads(23, (1, 7, 8, 9, 15, 16, 17, 33, 70))
    f_s, f_p = fence_reads(5, ((300, 5), (280, 21)))
    return c_s + f_s, c_p + f_p


@functools.lru_cache(maxsize=None)
def inputs():
    """(seqs, profs, recs) as tests/unrel_round_inputs.py's, the extra reads appended."""
    from oracle.oracle import Oracle
    seqs, profs, recs = round_inputs()
    e_s, e_p = extra_reads()
    O = Oracle(K, READ_LEN, HCOV, DCOV)
    more = []
    for s, p in zip(e_s, e_p):
        l, r = O.seq_context(s)
        iv = O.find_wall(p, l, r)
        iv2, riv = O.find_rel_intvl(iv, p, l, r)
        _, io, _, _ = O.classify_rel(riv, iv2, len(p))
        more.append(dict(io=io, call=O.classify_unrel(io), lab=O.classify_read(s, p)))   # (the oracle accepts every one)
    return seqs + e_s, profs + e_p, recs + more


def _hd(x):
    return (x == H_CLS) | (x == D_CLS)


def wide_paths(rec):
    """What one read reaches, counted on the oracle's records (`io`: the intervals as classify_unrel gets them, `call`:
    as it leaves them).  The records hold the state before the first sweep and behind the second, so what depends on
    the state in between is decided the cautious way: an interval "changes to or from H / D" if `io` and `call` differ
    in that, and a round is known to start at a multiple of the slot count only while nothing before it has changed."""
    io, call = rec["io"], rec["call"]
    N = len(io)
    out = dict()
    if N == 0:
        return out
    small = N <= SMALL_MAXN
    order = update_order(io)                               # the second sweep's order; the first runs it backwards
    nnf = len(order)
    if small:
        out["nnf_%d" % nnf] = 1
        out["small_two_windows"] = int(nnf > 2 * LANES_SMALL)
    else:
        out["big_ragged"] = int(nnf % SLOTS_BIG != 0)
        out["big_few"] = int(nnf < SLOTS_BIG)
        out["big_two_windows"] = int(nnf > 64)
    if nnf == 0:
        return out
    slots = SLOTS_SMALL if small else SLOTS_BIG
    pos = np.full(N, -10 ** 6, np.int64)
    pos[order] = np.arange(nnf)
    ch = _hd(io["asgn"]) != _hd(call["asgn"])              # changes to or from H / D (io's class is no H / D where it is none yet)
    ch |= _hd(io["asgn"]) & (io["asgn"] != call["asgn"])   # ... or between them
    nf = ~fixed(io)
    # index neighbours d apart in the update order, the one the first sweep takes first (the later in the order) changing
    for i in range(N - 1):
        if nf[i] and nf[i + 1]:
            d = int(abs(pos[i] - pos[i + 1]))
            first = i if pos[i] > pos[i + 1] else i + 1
            if 1 <= d <= 7 and ch[first]:
                out["near_%d" % d] = 1
    # a reliable non-fixed interval that joins the H or the D set, its slot in the first sweep's round: known while no
    # earlier update of that sweep changed anything (then every round before it ran to its end)
    fpos = nnf - 1 - pos                                   # position in the first sweep
    chg = np.sort(fpos[nf & ch])
    if len(chg):
        q = int(chg[0])
        i = int(order[nnf - 1 - q])
        if io["is_rel"][i] and _hd(call["asgn"][i]):
            slot = q % slots
            last = slot == slots - 1 or q == nnf - 1
            out["setc_first" if slot == 0 else "setc_last" if last else "setc_middle"] = 1
            if not small:
                out["setc_big"] = 1
    # second sweep: a position that is dirty when the sweep reaches it -- an index neighbour of an interval that changes
    # and that the first sweep takes later (its bit is set behind the neighbour's evaluation, by that change or, if the
    # change is the second sweep's, from in front) -- in the second half of a window of twice the round's positions
    L = LANES_SMALL if small else 64
    for i in range(N):
        if nf[i] and L <= pos[i] < 2 * L:
            for j in (i - 1, i + 1):
                if 0 <= j < N and nf[j] and ch[j] and pos[j] < pos[i]:
                    out["dirty_second_half" if small else "dirty_second_half_big"] = 1
    return out

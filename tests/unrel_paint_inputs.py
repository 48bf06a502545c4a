"""Inputs of tests/test_unrel_paint_inputs.py, tests/test_gpu_unrel_commit.py and tests/test_gpu_paint.py, and what the oracle
makes of them (computed once per process).

"Staircase" reads: count profiles made of 6-39 flat segments of 8-139 positions whose levels rise, fall or wander by a
fixed step.  Neighbouring intervals then have close counts, so the order of classify_unrel's updates (by min(cb,ce),
class_unrel.c:246-258) puts index neighbours next to each other -- the slots of one speculation round of
k_classify_unrel_grp that must not all commit -- and reliable intervals are left without a class by classify_rel and
end as H or D in classify_unrel: the reliable-H / reliable-D sets change under the sweep.
"""
import functools

import numpy as np

from adversarial import adversarial_reads

K, READ_LEN, HCOV, DCOV = 40, 20000, 20, 40
H_CLS, D_CLS = 2, 3                                        # CP_HAPLO, CP_DIPLO (include/classpro_amd.h)
LETTERS = np.frombuffer(b"ERHD", np.uint8)                 # CP_ERROR, CP_REPEAT, CP_HAPLO, CP_DIPLO


def staircase_reads(seed, n=1000):
    rng = np.random.default_rng(seed)
    seqs, profs = [], []
    for _ in range(n):
        nseg = int(rng.integers(6, 40))
        lens = rng.integers(8, 140, nseg)
        base = int(rng.choice([4, 12, 20, 30, 40]))
        step = int(rng.choice([3, 4, 6, 9]))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            levels = base + step * np.arange(nseg)
        elif kind == 1:
            levels = base + step * np.arange(nseg)[::-1]
        else:
            levels = base + step * rng.integers(0, 8, nseg)
        c = np.repeat(levels, lens)
        seqs.append(bytes(b"ACGT"[x] for x in rng.integers(0, 4, len(c) + K - 1)))
        profs.append(c.astype(np.uint16))
    return seqs, profs


def short_reads(seed=3):
    """Reads of K-1, K, K+1 and K+15 bases: no k-mer at all, one, two, and a label string of 55 bytes."""
    rng = np.random.default_rng(seed)
    seqs, profs = [], []
    for rlen in (K - 1, K, K + 1, K + 15):
        seqs.append(bytes(b"ACGT"[x] for x in rng.integers(0, 4, rlen)))
        profs.append(rng.integers(15, 45, rlen - (K - 1)).astype(np.uint16))
    return seqs, profs


def fixed(iv):
    """Intervals that classify_unrel leaves alone (class_unrel.c:249-252): reliable with class H or D."""
    return (iv["is_rel"] != 0) & ((iv["asgn"] == H_CLS) | (iv["asgn"] == D_CLS))


def update_order(io):
    """The non-fixed intervals in the order of the second sweep (the first one runs it backwards)."""
    order = np.argsort(np.minimum(io["cb"], io["ce"]), kind="stable")
    return order[~fixed(io)[order]]


@functools.lru_cache(maxsize=None)
def inputs():
    """(seqs, profs) of the 1000 staircase reads and the 250 adversarial ones, per read a dict of the oracle's records
    (`io`: intervals after classify_rel, `call`: after classify_unrel, `lab`: the label string)."""
    from oracle.oracle import Oracle
    s_s, s_p = staircase_reads(1, 1000)
    a_s, a_p = adversarial_reads(7, n=250)
    seqs, profs = s_s + a_s, s_p + a_p
    O = Oracle(K, READ_LEN, HCOV, DCOV)
    recs = []
    for s, p in zip(seqs, profs):
        l, r = O.seq_context(s)
        iv = O.find_wall(p, l, r)
        iv2, riv = O.find_rel_intvl(iv, p, l, r)
        _, io, _, _ = O.classify_rel(riv, iv2, len(p))
        recs.append(dict(io=io, call=O.classify_unrel(io), lab=O.classify_read(s, p)))   # (no OverflowError on any of them)
    return seqs, profs, recs


def labels_from_intervals(iv, rlen):
    """ClassPro.c:116-119,265-271: K-1 'N', then every interval's class letter over its positions."""
    if rlen < K:
        return b"N" * rlen
    body = np.repeat(LETTERS[iv["asgn"]], iv["e"] - iv["b"]) if len(iv) else np.zeros(0, np.uint8)
    return b"N" * (K - 1) + body.tobytes()

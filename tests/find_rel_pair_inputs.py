"""Inputs of tests/test_find_rel_pair_inputs.py and tests/test_gpu_find_rel_pairs.py: small reads whose reliable-candidate
intervals sit at every fork of cp_rel_counts (classpro_amd/csrc/cp_wall.h), which takes the two step sums of an
interval's end in one pass over one group of forty counts where it can and sum by sum where it cannot.

A read is a row of PLATEAUS (positions near the diploid coverage, every one an interval of the chosen length) kept apart
by TEETH (K positions at 1: an E-interval between two walls, the motif of wall_path_inputs).  Over a plateau the counts
wander by at most 2 from one position to the next (no candidate: CP_MIN_CNT_CHANGE is 3), so that every range of every
sum holds steps of both signs.  The bases are ACGTACGT..., which has no run of any kind, with runs written in where an
end's context is to be longer: the context right of base b+K-1 decides the begin's second sum (lmax_b), the context left
of base e-1 the end's (lmax_e).

  hp n   a homopolymer of n bases                      lmax = n (n <= 127); 0 to the right once 128 bases follow
  ds n   n bases of a dinucleotide                     lmax = 2*(1+(n-2)//2)
  ts n   n bases of a trinucleotide                    lmax = 3*(1+(n-3)//3)
Over the plain bases lmax is 3 (no homopolymer: 1, no dinucleotide: 1*2, no trinucleotide: 1*3).  Values below 3 other
than 0 do not exist: a base that differs from its neighbour has a dinucleotide context of at least 1 and a trinucleotide
context of at least 1, a base that equals it a homopolymer of at least 2 -- and then, unless the third equals them too
(homopolymer 3), a trinucleotide context of 1.  lmax = 0 exists to the right alone (the reference never writes the cells
of a homopolymer more than 127 bases before its end).

Which fork an interval takes is restated in `forks` from the ORACLE's records and contexts, nothing of the code under test.
"""
import collections
import functools
import itertools

import numpy as np

import wall_path_inputs as W
import wall_load_inputs as L
from wall_path_inputs import Read, READ_LEN, HCOV, DCOV

K = W.K
OTHER_K = (21, 41, 42, 63)
GROUP = 40                                                 # counts in one pass (five loads of eight)
CP_MAX_KMER_CNT = 0x7fff
LOG_PE_FINAL = float(np.log(1e-5))                         # const.c:62-63, PE_THRES[FINAL][SELF] (wall.c:1018)

Seg = collections.namedtuple("Seg", "L brun erun shape")
Seg.__new__.__defaults__ = (None, None, "wander")


def _put_run(x, lo, n, kind):
    """Bases lo .. lo+n-1 become a run whose letters differ from what would carry it on at either side."""
    unit = {"hp": 1, "ds": 2, "ts": 3}[kind]
    assert lo >= 4 and lo + n + 4 <= len(x)
    for pat in itertools.permutations(range(4), unit):
        before, after = pat[(-1) % unit], pat[n % unit]
        if x[lo - 1] != before and x[lo + n] != after:
            for q in range(n):
                x[lo + q] = pat[q % unit]
            return
    raise AssertionError("no letters for a run at %d" % lo)


def _counts(seg, rng, k, repeat):
    if seg.shape == "flat":
        return np.full(seg.L, DCOV)
    if seg.shape == "wander":
        # Steps of -2 .. 2, both signs everywhere: also among the three steps behind the begin and the two before the end
        # (lmax = 3).  The counts rise by 6 over the first 36 positions and fall by 6 over the last: the begin's two sums
        # differ by the rise wherever their ranges are nearly the same (lmax near K-1), the end's by the fall, so that a
        # step counted or left out by mistake shows in ccb / cce and is not lost in max(., 0).
        i = np.arange(seg.L)
        bump = np.minimum(np.minimum(i, seg.L - 1 - i) // 6, 6)
        r = rng.integers(0, 2, seg.L)
        if seg.L >= 3 * k:
            r[k - 1], r[k] = 1, 0                          # a step down from count b+K-1 to b+K: the last one of [b, b+K)
            r[seg.L - k], r[seg.L - k + 1] = 0, 1          # a step up from count e-K to e-K+1: the first one of [e-K, e-1)
        c = DCOV + bump + r
        c[:4], c[-3:] = [DCOV, DCOV + 2, DCOV + 1, DCOV + 2], [DCOV + 1, DCOV + 2, DCOV]
        assert np.abs(np.diff(c)).max() <= 2
        return c
    if seg.shape == "low_end":                             # begins at 42, ends flat at 38: cce < cb unless raised to it
        c = np.full(seg.L, DCOV - 2)
        c[:4] = [DCOV + 2, DCOV + 1, DCOV, DCOV - 1]
        return c
    if seg.shape == "spike":                               # climbs by 2 beyond REPEAT (no candidate on the way), one count at
        up = np.arange(DCOV, repeat + 4, 2)                # the largest value within the first K-1 steps, and down again
        assert len(up) + 2 <= k - 1 and seg.L >= 2 * len(up) + 8
        mid = np.full(seg.L - 2 * len(up), int(up[-1]))
        mid[1] = CP_MAX_KMER_CNT
        return np.concatenate([up, mid, up[::-1]])
    raise ValueError(seg.shape)


def build(name, segs, seed, k=K, tail=(), end_hp=0):
    """Plateaus `segs` with a tooth between two of them, then `tail` ((n, count) parts); end_hp: the read's last end_hp
    bases are one homopolymer."""
    rng = np.random.default_rng(seed)
    repeat = L.tables(k).cov[1]
    parts, at, pos = [], [], 0
    for q, s in enumerate(segs):
        if q:
            parts.append(np.full(k, 1)); pos += k
        at.append(pos)
        parts.append(_counts(s, rng, k, repeat)); pos += s.L
    for n, v in tail:
        parts.append(np.full(n, v)); pos += n
    c = np.concatenate(parts).astype(np.uint16)
    x = np.arange(len(c) + k - 1) % 4
    for s, b in zip(segs, at):
        e = b + s.L
        if s.brun:                                         # from base b+K-1 to the right
            _put_run(x, b + k - 1, s.brun[1], s.brun[0])
        if s.erun:                                         # up to base e-1 from the left
            _put_run(x, e - s.erun[1], s.erun[1], s.erun[0])
        if s.brun and s.erun:
            assert b + k - 1 + s.brun[1] + 4 <= e - s.erun[1], name
    if end_hp:
        x[len(x) - end_hp:] = (x[len(x) - end_hp - 1] + 1) % 4
    return Read(name, bytes(b"ACGT"[v] for v in x), c)


RUNS_B = (("hp", 8), ("hp", 9), ("hp", 38), ("hp", 39), ("hp", 40), ("hp", 127), ("ds", 38), ("ds", 40), ("ts", 39), ("hp", 200), None)
RUNS_E = (("hp", 9), ("hp", 8), ("ds", 38), ("ts", 39), ("hp", 127), ("hp", 40), ("hp", 38), ("hp", 39), ("ds", 40), None, ("hp", 8))


def lengths(k):
    return (k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1)


@functools.lru_cache(maxsize=None)
def reads():
    R = []
    # the six lengths over plain bases; the first plateau is the read's first interval (index 0 at position 0): the
    # three lengths around 2K there, with an end count below the begin count
    for n in lengths(K)[3:]:
        R.append(build("fp_first%d" % n, [Seg(n, shape="low_end"), Seg(100)], 600 + n))
    R.append(build("fp_lengths", [Seg(100)] + [Seg(n) for n in lengths(K)] + [Seg(100)], 610))
    # every context class at either end, on plateaus long enough for both runs; short ones with one short run
    long_ = 2 * 127 + K + 60
    R.append(build("fp_runs", [Seg(120)] + [Seg(long_ if (b and b[1] > 100) or (e and e[1] > 100) else 200, b, e) for b, e in zip(RUNS_B, RUNS_E)] + [Seg(120)], 620))
    R.append(build("fp_short_runs", [Seg(90), Seg(K, ("hp", 8)), Seg(K, None, ("hp", 9)), Seg(K + 1, ("hp", 9)), Seg(K + 1, None, ("hp", 8)),
                                     Seg(3 * K, ("hp", 39), ("hp", 9)), Seg(3 * K + 1, ("hp", 9), ("ts", 39)), Seg(90)], 621))
    # where the groups of forty counts lie in the read: last intervals of K+1, K and K-1 positions (b+40 = plen-1, plen,
    # plen+1), and intervals of K positions one and two positions before the read's end
    for n in (K + 1, K, K - 1):
        R.append(build("fp_last%d" % n, [Seg(100), Seg(n)], 630 + n))
    for n in (1, 2):
        R.append(build("fp_tail%d" % n, [Seg(100), Seg(K)], 640 + n, tail=[(n, 1)]))
    # a last interval under a homopolymer that runs to the read's end: exactly to it (the second sum ends AT plen), and
    # one of 254 bases (lmax_b = 127 with 101 bases left; lmax_e = 127 > 101 as well, on an interval that starts beyond 127)
    R.append(build("fp_end_hp100", [Seg(300), Seg(100)], 650, end_hp=100))
    R.append(build("fp_end_hp254", [Seg(300), Seg(101)], 651, end_hp=254))
    # a corrected count that saturates
    R.append(build("fp_saturated", [Seg(100), Seg(160, shape="spike"), Seg(100)], 660))
    # more than 64 and more than 128 passing intervals; none
    R.append(build("fp_fill70", [Seg(K + q % 5) for q in range(70)], 670))
    R.append(build("fp_fill135", [Seg(K + q % 7) for q in range(135)], 671))
    R.append(build("fp_none", [Seg(K - 1 - q % 3) for q in range(12)], 672))
    names = [r.name for r in R]
    assert len(set(names)) == len(names)
    return tuple(R)


@functools.lru_cache(maxsize=None)
def reads_other_k(k):
    """The same forks for another K: the lengths, the runs around K-1, a run beyond it, the read's ends."""
    long_ = 2 * 127 + k + 60
    runs = [(("hp", 8), ("hp", 9)), (("hp", k - 2), ("hp", k - 1)), (("hp", k - 1), ("hp", k)), (("hp", k), ("hp", k - 2)),
            (("hp", 127), ("hp", 127)), (("ds", k), ("ts", k)), (("ts", k), ("ds", k))]
    return (build("fpk%d_lengths" % k, [Seg(n, shape="low_end") for n in lengths(k)[4:5]] + [Seg(n) for n in lengths(k)] + [Seg(100)], 700 + k, k),
            build("fpk%d_runs" % k, [Seg(2 * k + 20)] + [Seg(long_, b, e) for b, e in runs] + [Seg(k + 1)], 710 + k, k),
            build("fpk%d_ends" % k, [Seg(k + 9), Seg(3 * k), Seg(k)], 720 + k, k),
            build("fpk%d_fill" % k, [Seg(k + q % 5) for q in range(70)], 730 + k, k))


def _expected(O, rs):
    out = []
    for r in rs:
        l, rc = O.seq_context(r.seq)
        try:
            iv = O.find_wall(r.prof, l, rc)
        except RuntimeError:
            out.append(None)
            continue
        out.append(dict(wall=iv, rel=O.find_rel_intvl(iv, r.prof, l, rc), lab=O.classify_read(r.seq, r.prof), ctx=(l, rc)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(k=K):
    """Per read of reads() / reads_other_k(k), the oracle's dict(wall, rel, lab) as wall_path_inputs.expected(), plus its
    context arrays (ctx)."""
    return _expected(L.tables(k).O, reads() if k == K else reads_other_k(k))


def forks(r, e, k=K):
    """The intervals of read r that pass the three record-only tests (wall.c:1016-1019), each a dict: idx, b, e, n (its
    length), lmax_b, lmax_e, pair_b / pair_e (the end's two sums go in one pass) and why not -- the conditions of
    cp_rel_counts restated on the oracle's records (e: expected()'s entry) and contexts."""
    T = L.tables(k)
    lctx, rctx = e["ctx"]
    plen = len(r.prof)
    out = []
    for idx, I in enumerate(e["wall"]):
        b, en, cb, ce = int(I["b"]), int(I["e"]), int(I["cb"]), int(I["ce"])
        if en - b < k or max(cb, ce) >= T.cov[1] or I["pe"] >= LOG_PE_FINAL:
            continue
        lb = max(int(rctx[b + k - 1][t]) * (t + 1) for t in range(3))
        le = max(int(lctx[en - 1][t]) * (t + 1) for t in range(3))
        sb = 1 if k - 1 <= GROUP - 1 else 0
        d = dict(idx=idx, b=b, e=en, n=en - b, lmax_b=lb, lmax_e=le)
        d["pair_b"] = k - 1 <= GROUP and lb <= k - 1 and b + 1 - sb + GROUP <= plen
        d["pair_e"] = k - 1 <= GROUP and le <= k - 1 and en >= GROUP
        d["raise_cce"] = idx == b and en - 2 * k <= b
        out.append(d)
    return out

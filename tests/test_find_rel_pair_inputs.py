"""The reads of tests/find_rel_pair_inputs.py put a passing interval at every fork of cp_rel_counts (cp_wall.h: both step
sums of an interval's end in one pass over forty counts, or sum by sum), and the product's scalar functions in the
harness's sequential orchestration (hh_classify_read, which calls cp_rel_interval) give the oracle's STAGE_REL records
and labels for every one of them.  CPU; tests/test_gpu_find_rel_pairs.py runs the same reads on the device.

Which fork an interval takes is `find_rel_pair_inputs.forks`: the function's conditions restated on the oracle's records
and contexts.  Not reachable, and so not asked for (module docstring of the inputs): a context of 1 or 2 at either end
and of 0 at the end side; an interval that passes the length test with b+40 = plen+1 at K = 40 (fp_last39 is that
interval: it fails the test, as asserted).
"""
import ctypes as C

import numpy as np
import pytest

import find_rel_pair_inputs as F
from test_host_logic import run_harness_read
from test_oracle_wall import same_records

K = F.K


@pytest.fixture(scope="module")
def params(harness):
    P = {k: harness.hh_params_new(k, F.READ_LEN, F.HCOV, F.DCOV) for k in (K,) + F.OTHER_K}
    assert all(P.values())
    yield P
    for p in P.values():
        harness.hh_params_free(C.c_void_p(p))


def all_forks(k=K):
    rs = F.reads() if k == K else F.reads_other_k(k)
    return {r.name: (len(r.prof), F.forks(r, e, k)) for r, e in zip(rs, F.expected(k))}


def test_oracle_accepts_every_read(built):
    for k in (K,) + F.OTHER_K:
        rs = F.reads() if k == K else F.reads_other_k(k)
        for r, e in zip(rs, F.expected(k)):
            assert e is not None, (k, r.name)


def test_a_passing_interval_at_every_fork(built):
    A = all_forks()
    every = [dict(d, read=nm, plen=plen) for nm, (plen, f) in A.items() for d in f]

    def some(pred, what):
        hit = [(d["read"], d["idx"]) for d in every if pred(d)]
        print("%-64s %3d  %s" % (what, len(hit), " ".join("%s:%d" % h for h in hit[:4])))
        assert hit, what

    # interval lengths (K-1 fails the length test: fp_lengths and fp_last39 hold one each, and it is in no list)
    for n in F.lengths(K)[1:]:
        some(lambda d: d["n"] == n, "length %d" % n)
    for nm in ("fp_lengths", "fp_last39"):
        e = F.expected()[[r.name for r in F.reads()].index(nm)]
        assert any(int(I["e"]) - int(I["b"]) == K - 1 and int(I["cb"]) >= F.DCOV for I in e["wall"]), nm
        assert not any(d["n"] < K for d in A[nm][1])
    # line `idx == Ib && Ie-2K <= Ib`: the index equal to the position, on either side of the length clause
    some(lambda d: d["raise_cce"] and d["n"] == 2 * K - 1, "index == position, length 2K-1 (cce raised)")
    some(lambda d: d["raise_cce"] and d["n"] == 2 * K, "index == position, length 2K (cce raised)")
    some(lambda d: d["idx"] == d["b"] and d["n"] == 2 * K + 1 and not d["raise_cce"], "index == position, length 2K+1 (not raised)")
    # contexts: word-decided, fall-back scans around K-1, beyond it
    for side in ("lmax_b", "lmax_e"):
        pair = "pair_" + side[-1]
        for v in (3, 8, 9, K - 2, K - 1):
            some(lambda d: d[side] == v and d[pair], "%s = %d, one pass" % (side, v))
        for v in (K, 127):
            some(lambda d: d[side] == v and not d[pair], "%s = %d, sum by sum" % (side, v))
    some(lambda d: d["lmax_b"] == 0 and d["pair_b"], "lmax_b = 0 (empty second range)")
    some(lambda d: d["lmax_e"] > d["n"] and d["b"] >= 127, "lmax_e beyond the interval's length, b >= 127")
    assert all(d["e"] - d["lmax_e"] >= 0 for d in every)      # (the parent reads outside the read there)
    # the four combinations of the two ends
    for pb in (True, False):
        for pe in (True, False):
            some(lambda d: d["pair_b"] == pb and d["pair_e"] == pe, "begin %s, end %s" % ("paired" if pb else "single", "paired" if pe else "single"))
    # where the groups lie in the read
    some(lambda d: d["b"] == 0, "the read's first interval")
    some(lambda d: d["e"] == d["plen"], "the read's last interval")
    some(lambda d: d["e"] == d["plen"] and d["pair_e"] and d["n"] in (K, K + 1), "... of K / K+1 positions, end in one pass")
    some(lambda d: d["b"] + 40 == d["plen"] - 1 and d["e"] == d["plen"], "b+40 = plen-1, the last interval")
    some(lambda d: d["b"] + 40 == d["plen"] - 1 and d["e"] < d["plen"], "b+40 = plen-1, not the last")
    some(lambda d: d["b"] + 40 == d["plen"] and d["pair_b"], "b+40 = plen, begin in one pass")
    some(lambda d: d["e"] == d["plen"] and d["b"] + d["lmax_b"] == d["plen"], "the begin's second sum ends at plen")
    some(lambda d: d["e"] == d["plen"] and d["b"] + d["lmax_b"] > d["plen"], "... beyond plen")
    # wave fill
    n = {nm: len(f) for nm, (_, f) in A.items()}
    assert 64 < n["fp_fill70"] <= 128 < n["fp_fill135"] and n["fp_none"] == 0
    # a corrected count that saturates; steps of both signs within either range of either end
    sat = next(e for r, e in zip(F.reads(), F.expected()) if r.name == "fp_saturated")
    assert any(int(sat["rel"][0]["ccb"][d["idx"]]) == F.CP_MAX_KMER_CNT for d in A["fp_saturated"][1])
    r = next(r for r in F.reads() if r.name == "fp_lengths")
    p = r.prof.astype(np.int64)
    for d in A["fp_lengths"][1]:
        for lo, hi in ((d["b"], d["b"] + d["lmax_b"]), (d["b"], d["b"] + K - 1), (d["e"] - d["lmax_e"], d["e"] - 1), (d["e"] - K + 1, d["e"] - 1)):
            s = np.diff(p[lo:hi + 1])
            assert (s > 0).any() and (s < 0).any(), (d, lo, hi)


def test_other_k_take_the_other_routes(built):
    """K = 21: groups that would leave the read at either end; K = 41: the begin's group behind the lead count; K = 42
    and 63: never one pass."""
    for k in F.OTHER_K:
        every = [dict(d, plen=plen) for plen, f in all_forks(k).values() for d in f]
        assert len(every) >= 80
        if k <= 41:
            assert any(d["pair_b"] and d["pair_e"] for d in every) and any(not d["pair_b"] and d["lmax_b"] > k - 1 for d in every)
            assert any(d["lmax_b"] == k - 1 and d["pair_b"] for d in every) and any(d["lmax_e"] == k - 1 and d["pair_e"] for d in every)
            assert any(d["lmax_b"] == k and not d["pair_b"] for d in every) and any(d["lmax_e"] == k and not d["pair_e"] for d in every)
        else:
            assert not any(d["pair_b"] or d["pair_e"] for d in every)
        if k == 21:
            assert any(d["e"] < F.GROUP and not d["pair_e"] and d["lmax_e"] <= k - 1 for d in every)
            assert any(d["b"] + F.GROUP > d["plen"] and not d["pair_b"] and d["lmax_b"] <= k - 1 for d in every)


@pytest.mark.parametrize("k", (K,) + F.OTHER_K)
def test_harness_equals_the_oracle(harness, params, k):
    rs = F.reads() if k == K else F.reads_other_k(k)
    for r, e in zip(rs, F.expected(k)):
        N, lab, iv, riv, *_ = run_harness_read(harness, params[k], r.seq, r.prof)
        o_iv, o_riv = e["rel"]
        assert N == len(o_iv) and same_records(iv, o_iv, fields=("b", "e", "cb", "ce", "is_rel")), (k, r.name)
        passing = [d["idx"] for d in F.forks(r, e, k)]
        for f in ("ccb", "cce"):
            assert np.array_equal(iv[f][passing], o_iv[f][passing]), (k, r.name, f, passing, iv[f][passing], o_iv[f][passing])
        assert same_records(riv, o_riv, fields=("b", "e", "cb", "ce", "ccb", "cce", "is_rel")), (k, r.name)
        assert lab == e["lab"], (k, r.name)

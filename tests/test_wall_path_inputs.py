"""The reads of tests/wall_path_inputs.py pass through every fork of k_wall_tasks / k_find_wall, the oracle accepts or
rejects each as its row expects, and the product's scalar functions in the harness's sequential orchestration give the
oracle's find_wall records for them.  CPU; tests/test_gpu_wall_paths.py runs the same reads on the device.

The reach table (rows: the issue's; module docstring of wall_path_inputs.py for the building blocks and for rows (a) to
(d)) is printed with the reads per row; every row of 1 to 12 must have its minimum.
"""
import ctypes as C

import numpy as np
import pytest

import wall_path_inputs as W
from test_host_logic import run_harness_read
from test_oracle_wall import same_records


@pytest.fixture(scope="module")
def params(harness):
    P = {k: harness.hh_params_new(k, W.READ_LEN, W.HCOV, W.DCOV) for k in (W.K,) + W.OTHER_K}
    assert all(P.values())
    yield P
    for p in P.values():
        harness.hh_params_free(C.c_void_p(p))


@pytest.fixture(scope="module")
def accounts(harness, params):
    return {r.name: W.account(harness, params[W.K], r.seq, r.prof) for r in W.reads()}


def test_reach_table(accounts):
    plens = {r.name: len(r.prof) for r in W.reads()}
    table = W.reach_table(accounts, plens)
    for row, what, need, hit in table:
        print("%-3s %-48s %3d (min %d)  %s" % (row, what, len(hit), need, " ".join(hit[:6]) + (" ..." if len(hit) > 6 else "")))
    for nm, a in accounts.items():
        print("%-28s plen %6d  %s" % (nm, plens[nm], " ".join("%s=%d" % kv for kv in a.items())))
    for row, what, need, hit in table:
        assert len(hit) >= need, (row, what)
    # rows (a) to (d): reached, all four (module docstring)
    assert all(hit for row, _, _, hit in table if row in "abcd")
    assert max(plens[nm] for nm in plens if not nm.startswith("plen6")) <= 15500


def test_other_k_reads_keep_the_self_memo_off_chip(harness, params):
    """Row 12: the reads of row 1 whose SELF memo is off chip, built for K = 25 and K = 101, are off chip there too: the
    one-lane replay runs with its paired-flag window (K = 25) and without it (K = 101)."""
    for k in W.OTHER_K:
        for r in W.reads_other_k(k):
            a = W.account(harness, params[k], r.seq, r.prof)
            p = W.wall_paths(a, len(r.prof), k)
            print(k, r.name, a, "use_lds", p["use_lds"], "use_win", p["use_win"])
            assert a["n_live0"] >= 125 and not p["lane_replay"] and a["overflow"] == 0
            assert p["use_win"] == (k == 25)
    assert {W.wall_paths(W.account(harness, params[k], r.seq, r.prof), len(r.prof), k)["use_lds"]
            for k in W.OTHER_K for r in W.reads_other_k(k)} == {0, 2}


def test_oracle_accepts_what_the_account_accepts(accounts):
    """The reference aborts ("# E-intvls >= plen") on exactly the reads whose account says overflow."""
    for r, e in zip(W.reads(), W.expected()):
        assert (e is None) == (accounts[r.name]["overflow"] != 0), r.name
    for k in W.OTHER_K:
        assert all(e is not None for e in W.expected(k))


@pytest.mark.parametrize("k", (W.K,) + W.OTHER_K)
def test_harness_intervals_equal_the_oracle(harness, params, k):
    """hh_classify_read -- the function the account is counted in -- against the oracle's find_wall records: b e cb ce
    equal, pe peo_b peo_e bit for bit, and the labels."""
    rs = W.reads() if k == W.K else W.reads_other_k(k)
    for r, e in zip(rs, W.expected(k)):
        N, lab, iv, *_ = run_harness_read(harness, params[k], r.seq, r.prof)
        if e is None:
            assert N < 0, r.name
            continue
        assert N == len(e["wall"]) and same_records(iv, e["wall"], fields=("b", "e", "cb", "ce")), r.name
        assert lab == e["lab"], r.name

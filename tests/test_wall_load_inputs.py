"""The reads of tests/wall_load_inputs.py reach every case that k_wall_tasks' on-chip lists and the load groups of
cp_wall_candidate_live tell apart (CPU only): the counts by the harness's account, the rest by the restatement
`live_tasks`, which is itself tied to the account (its number of tasks per read is the account's)."""
import ctypes as C
import functools

import numpy as np

import wall_path_inputs as W
import wall_load_inputs as L


@functools.lru_cache(maxsize=None)
def accounts_and_tasks(harness):
    P = harness.hh_params_new(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    T = L.tables()
    acc = {r.name: W.account(harness, P, r.seq, r.prof) for r in L.reads()}
    tasks = {r.name: L.live_tasks(T, r) for r in L.reads()}
    harness.hh_params_free(C.c_void_p(P))
    return acc, tasks


def test_restatement_counts_the_accounts_tasks(harness):
    acc, tasks = accounts_and_tasks(harness)
    for r in L.reads():
        a, t = acc[r.name], tasks[r.name]
        assert len(t) == a["n_t"], r.name
        assert sum(1 for x in t if x["e"] == L.CP_SELF) == a["n_live0"], r.name
    # ... and on reads of the path set, whose sequences are random
    P = harness.hh_params_new(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    for r in W.reads()[:12]:
        a, t = W.account(harness, P, r.seq, r.prof), L.live_tasks(L.tables(), r)
        assert (len(t), sum(1 for x in t if x["e"] == L.CP_SELF)) == (a["n_t"], a["n_live0"]), r.name
    harness.hh_params_free(C.c_void_p(P))


def test_candidate_and_task_counts_are_reached(harness):
    acc, _ = accounts_and_tasks(harness)
    n_c = {a["n_c"] for a in acc.values()}
    n_t = {a["n_t"] for a in acc.values()}
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= n_c, sorted(n_c)
    assert {0, 1, 64, 65, 128, 129} <= n_t, sorted(n_t)
    # the last row of the lists on chip and the last rows of the task list: 255 candidates with more than 128 tasks
    assert any(a["n_c"] == L.FW_LISTS and a["n_t"] > 2 * L.WAVE for a in acc.values())
    # a long read (the lists in HBM, staged step by step) with more than one step of tasks
    assert any(a["n_c"] > L.FW_LISTS + 1 and a["n_t"] > 2 * L.WAVE for a in acc.values())


def test_partner_offsets_around_the_wide_load_are_reached(harness):
    _, tasks = accounts_and_tasks(harness)
    all_t = [x for t in tasks.values() for x in t]
    for right in (True, False):
        seen = {x["d"] for x in all_t if x["right"] == right and x["lc"] == "inside" and x["wide"]}
        assert {-2, -1, 0, 5, 6} <= seen, (right, sorted(seen))
        assert any(x["lc_in_wide"] and x["d"] == -1 for x in all_t if x["right"] == right)
        assert any(x["lc"] == "inside" and x["wide"] and not x["lc_in_wide"] for x in all_t if x["right"] == right)


def test_read_ends_are_reached(harness):
    _, tasks = accounts_and_tasks(harness)
    all_t = [x for t in tasks.values() for x in t]
    plen = {r.name: len(r.prof) for r in L.reads()}
    lo_neg = [x for x in all_t if x["lo8"] < 0 and x["lc"] != "none"]
    hi_out = [(nm, x) for nm, t in tasks.items() for x in t if x["lo8"] >= 0 and x["lo8"] + 8 > plen[nm] and x["lc"] != "none"]
    assert lo_neg and hi_out
    assert any(x["lc"] == "boundary" and x["right"] for x in all_t)
    assert any(x["lc"] == "boundary" and not x["right"] for x in all_t)
    assert any(0 < x["hc_out"] <= L.CP_MAX_N_HC for x in all_t if x["right"])          # some partners inside, some beyond the end
    assert any(0 < x["hc_out"] <= L.CP_MAX_N_HC for x in all_t if not x["right"])
    # exactly at the edge: the eight counts end at the read's last count / begin at its first
    assert any(x["wide"] and x["lo8"] + 8 == plen[nm] for nm, t in tasks.items() for x in t)
    assert any(x["wide"] and x["lo8"] == 0 for x in all_t)


def test_long_read_and_far_skellam_entries_are_reached(harness):
    acc, tasks = accounts_and_tasks(harness)
    long = [r for r in L.reads() if len(r.prof) > 65535]
    assert long and all(1 <= acc[r.name]["n_c"] <= 10 and acc[r.name]["n_t"] >= 1 for r in long)
    assert any(x["i"] > 65535 for r in long for x in tasks[r.name])
    far = [v for t in tasks.values() for x in t if x["e"] == L.CP_OTHERS for v in x["far"]]
    assert any(v > L.SKEL_CDMAX[1024] for v in far)                                     # beyond the default table
    assert any(v > L.SKEL_CDMAX[1] for v in far) and any(v <= L.SKEL_CDMAX[1024] for v in far)
    assert sum(1 for t in tasks.values() for x in t if x["e"] == L.CP_OTHERS) >= 4

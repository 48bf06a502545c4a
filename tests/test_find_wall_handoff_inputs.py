"""The reads of tests/find_wall_handoff_inputs.py reach every edge of the task record and of the replay's chunks that
they are named for (CPU only): the counts by the harness's account, the order of the tasks and their low-complexity
partners by the restatement `wall_load_inputs.live_tasks` (tied to the account here as in test_wall_load_inputs.py).

Which partner a task ACCEPTS the restatement does not say; where a read is there for an accepted partner, it is built so
that the account leaves one possibility: the walk's E-intervals (NSw), the ends of them that are no candidates (x), and
the positions of the read's few candidates decide it (see the single tests)."""
import ctypes as C
import functools

import numpy as np

import wall_path_inputs as W
import wall_load_inputs as L
import find_wall_handoff_inputs as F

K = W.K


@functools.lru_cache(maxsize=None)
def accounts_and_tasks(harness):
    P = harness.hh_params_new(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    T = L.tables()
    kmers = [r for r in F.reads() if len(r.prof)]
    acc = {r.name: W.account(harness, P, r.seq, r.prof) for r in kmers}
    tasks = {r.name: L.live_tasks(T, r) for r in kmers}
    harness.hh_params_free(C.c_void_p(P))
    return acc, tasks


def by_name(name):
    return next(r for r in F.reads() if r.name == name)


def paths(acc, name):
    return W.wall_paths(acc[name], len(by_name(name).prof), K)


def test_oracle_accepts_every_read(built):
    for r, e in zip(F.reads(), F.expected()):
        assert e is not None, r.name
    # the read without k-mers: nothing to abort on; what the oracle is asked for it is its labels
    r, e = next((r, e) for r, e in zip(F.reads(), F.expected()) if r.name == "hf_no_kmer")
    assert e["lab"] == b"N" * len(r.seq) and len(e["wall"]) == 0 and len(e["rel"][0]) == 0 and len(e["rel"][1]) == 0


def test_restatement_counts_the_accounts_tasks(harness):
    acc, tasks = accounts_and_tasks(harness)
    for name, a in acc.items():
        t = tasks[name]
        assert (len(t), sum(1 for x in t if x["e"] == L.CP_SELF)) == (a["n_t"], a["n_live0"]), name
        assert a["n_c"] == len(F.candidates(by_name(name))), name
        assert a["overflow"] == 0, name


def test_task_counts_around_the_chunks(harness):
    acc, _ = accounts_and_tasks(harness)
    for n in (63, 64, 65, 127, 128, 129):
        name = "hf_nt%d" % n
        assert acc[name]["n_t"] == n, name
        p = paths(acc, name)
        assert p["lane_replay"] and p["onchip0"], name        # a lane per task, flags on chip: the row in the record is used


def test_two_tasks_of_one_candidate_straddle_a_chunk(harness):
    acc, tasks = accounts_and_tasks(harness)
    t = tasks["hf_same_cand_63_64"]
    assert t[63]["i"] == t[64]["i"] and (t[63]["e"], t[64]["e"]) == (L.CP_SELF, L.CP_OTHERS)
    assert t[62]["i"] != t[63]["i"] and t[65]["i"] != t[64]["i"]
    assert paths(acc, "hf_same_cand_63_64")["onchip0"]


def test_pairs_across_the_chunk_end_in_both_directions(harness):
    acc, tasks = accounts_and_tasks(harness)
    # forward: 32 teeth, every one an E-interval between two candidates (x = 0); the 32nd's DROP is task 63, its GAIN,
    # K positions on and the only candidate among the DROP's partners, the candidate of task 64
    a, t = acc["hf_pair_63_to_64"], tasks["hf_pair_63_to_64"]
    assert (a["NSw"], a["x"]) == (32, 0) and paths(acc, "hf_pair_63_to_64")["onchip0"]
    assert t[63]["right"] and not t[64]["right"] and t[64]["i"] == t[63]["i"] + K
    # the reverse: 31 teeth and REV make 33 E-intervals, ONE end of which is no candidate.  REV's DROP (task 63) has no
    # candidate among its partners but the GAIN (its reach ends there), so had it taken the GAIN, the GAIN -- paired --
    # would have made no interval of its own: the DROP's interval ends off the candidates, and the GAIN's (task 64) on
    # the only candidate in ITS reach, the DROP, K+4 positions to the left
    a, t = acc["hf_pair_64_to_63"], tasks["hf_pair_64_to_63"]
    assert (a["NSw"], a["x"]) == (33, 1) and paths(acc, "hf_pair_64_to_63")["onchip0"]
    assert t[63]["right"] and not t[64]["right"] and t[64]["i"] == t[63]["i"] + K + 4
    cand = set(F.candidates(by_name("hf_pair_64_to_63")).tolist())
    d, g = t[63]["i"], t[64]["i"]
    assert cand & set(range(d + 1, d + K + F.CP_MAX_N_HC)) == {g}
    assert cand & set(range(g - K - F.CP_MAX_N_HC, g)) == {d}


def test_high_complexity_partners_at_the_largest_offset(harness):
    acc, tasks = accounts_and_tasks(harness)
    far = K - 1 + F.CP_MAX_N_HC
    # to the right: a tooth of K+4 positions is an E-interval between its two candidates, made by the DROP (the first of
    # the two tasks); the GAIN is its last high-complexity partner and not its low-complexity one
    a, t = acc["hf_hc_right"], tasks["hf_hc_right"]
    assert (a["NSw"], a["x"]) == (3, 0) and paths(acc, "hf_hc_right")["onchip0"]
    assert t[-2]["right"] and t[-1]["i"] - t[-2]["i"] == far and t[-2]["j"] != t[-1]["i"]
    # to the left: REV, as above
    a, t = acc["hf_hc_left"], tasks["hf_hc_left"]
    assert (a["NSw"], a["x"]) == (4, 1) and paths(acc, "hf_hc_left")["onchip0"]
    assert not t[-1]["right"] and t[-2]["i"] - t[-1]["i"] == -far and t[-1]["j"] != t[-2]["i"]


def test_boundary_partners_at_both_ends(harness):
    _, tasks = accounts_and_tasks(harness)
    t = tasks["hf_boundaries"]
    assert any(x["lc"] == "boundary" and x["right"] for x in t)          # lc_j = plen
    assert any(x["lc"] == "boundary" and not x["right"] for x in t)      # lc_j = 0


def test_wide_position_and_wide_row(harness):
    acc, tasks = accounts_and_tasks(harness)
    r = by_name("hf_plen66300")
    assert len(r.prof) > 65536 and any(x["i"] >= 65536 for x in tasks[r.name])
    assert not paths(acc, r.name)["onchip0"]
    r = by_name("hf_row256")
    rows = {int(i): k for k, i in enumerate(F.candidates(r))}
    assert acc[r.name]["n_c"] == 257 and any(rows[x["i"]] >= 256 for x in tasks[r.name])


def test_memo_edges(harness):
    acc, _ = accounts_and_tasks(harness)
    want = {"hf_self124": (124, None, True), "hf_self125": (125, None, False),
            "hf_others28": (None, 28, True), "hf_others29": (None, 29, False)}
    for name, (n0, n1, lanes) in want.items():
        a = acc[name]
        assert n0 is None or a["n_live0"] == n0, name
        assert n1 is None or a["n_t"] - a["n_live0"] == n1, name
        assert paths(acc, name)["lane_replay"] == lanes, name


def test_no_kmer_and_no_candidate(harness):
    acc, _ = accounts_and_tasks(harness)
    assert len(by_name("hf_no_kmer").seq) == K - 1 and len(by_name("hf_no_kmer").prof) == 0
    assert acc["hf_no_candidate"]["n_c"] == 0 and acc["hf_no_candidate"]["n_t"] == 0

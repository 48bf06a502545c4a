"""The main class of k_classify_rel_grp with the lane's own DP cell held in registers from one step to the next and the cells
in LDS as 16-byte pieces in a single buffer (kernels.hip: rel_grp_lds<MAXM,8>, rel_grp_pass with LD = 4; cp_class.h:
cp_cell_piece, cp_rel_cell_off), against the oracle.  `-m gpu`.

Compared exactly as tests/test_gpu_rel_grp_stream.py does (its check_batches): the forward and backward assignments, `asgn`
of both record kinds and the label bytes, as shipped and with CLASSPRO_COMPACT_REL=0.  Integers and bytes: equal or not.

  * mixed lengths in one wave: a batch of exactly eight reads -- one wave whatever the sort by M does -- with M = 0, 1, 2, 3
    and four reads of M >= 30: the lanes of a finished read sit on their registers and their cells for dozens of steps
    before the traceback reads the cells.  Both read orders;
  * "only R reachable" steps, where the new cell is the lane's own (dp and dhr from its registers, the rest from LDS): the
    reads of the CPU test with a look-up on a stand-in, each of which has such steps, in batches of eight with reads
    that have none in either direction, so both kinds of step meet in one wave;
  * the top of the class: 160 reads of a 20-kb set, some with 100 <= M <= 112 (the last rows of the back-pointers and the
    last word of the flags), one with M = 112, and some with M > 112 that take the other class beside them;
  * a repeated pass with mixed lengths: the init of the second pass sets the registers again while other reads of the
    wave have long finished.
"""
import numpy as np
import pytest

from test_gpu_rel_grp_stream import MAIN_MAXM, WAVE_READS, RefReads, check_batches, ref_set

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def mixed_eight(built):
    """[(RefReads, index)] x 8: M = 0, 1, 2, 3 from a set of short reads, four reads with M >= 30 from a 10-kb set."""
    short = ref_set(genome_len=60000, cov=40, read_len=600, min_len=60, seed=4)     # its first 300 reads: M 0-9
    long_ = ref_set(genome_len=200000, cov=40, read_len=10000, seed=5)              # its first reads: M 8-70
    Ms = [short.M(j) for j in range(300)]
    pick = [(short, Ms.index(m)) for m in (0, 1, 2, 3)]
    big = [j for j in range(60) if 30 <= long_.M(j) <= MAIN_MAXM][:4]
    assert len(big) == 4
    pick += [(long_, j) for j in big]
    assert sorted(S.M(j) for S, j in pick)[:4] == [0, 1, 2, 3] and len(pick) == WAVE_READS
    return pick


def test_mixed_lengths_in_one_wave(torch_dev, mixed_eight, monkeypatch):
    print("M of the eight reads:", [S.M(j) for S, j in mixed_eight])
    check_batches(monkeypatch, [mixed_eight, mixed_eight[::-1]])


def test_only_r_steps(torch_dev, harness, monkeypatch):
    from rel_anchor_inputs import K, HC, DC, load_probe, reliable_intervals, run_direction, standin_reads
    import ctypes as C
    probe = load_probe()
    rows = [r for r in standin_reads(harness, probe) if r[3] <= MAIN_MAXM]
    with_r = [r for r in rows if r[4] or r[5]]
    # reads without an "only R reachable" step in either direction: no "absolutely repeat" flag set by the DP
    P = probe.rap_params_new(K, 20000, HC, DC)
    none = []
    for r in rows:
        if r[4] or r[5] or len(none) >= len(with_r):
            continue
        riv = reliable_intervals(harness, P, r[1], r[2])
        if not any(run_direction(probe, P, riv, len(r[2]), F, 1)[0]["rpos"].any() for F in (1, 0)):
            none.append(r)
    # ... and each read with a look-up on a stand-in has such a step
    for r in with_r:
        riv = reliable_intervals(harness, P, r[1], r[2])
        assert any(run_direction(probe, P, riv, len(r[2]), F, 1)[0]["rpos"].any() for F in (1, 0)), r[0]
    probe.rap_params_free(C.c_void_p(P))
    print("%d reads with only-R steps, %d without" % (len(with_r), len(none)))
    assert len(with_r) >= 8 and len(none) >= 4
    S = RefReads([r[1] for r in with_r + none], [r[2] for r in with_r + none])
    nw = len(with_r)
    batches = []
    for b in range((nw + 3) // 4):                           # four of each kind: one wave
        a = list(range(4 * b, min(4 * b + 4, nw)))
        n = [nw + (4 * b + x) % len(none) for x in range(WAVE_READS - len(a))]
        batches.append([(S, j) for pair in zip(a, n) for j in pair] + [(S, j) for j in n[len(a):]])
        assert len(batches[-1]) == WAVE_READS
    check_batches(monkeypatch, batches)


def test_top_of_the_class(torch_dev, built, monkeypatch):
    S = ref_set(genome_len=400000, cov=40, read_len=20000, seed=7)
    n = 160
    Ms = np.array([S.M(j) for j in range(n)])
    top, last, over = int(((Ms >= 100) & (Ms <= MAIN_MAXM)).sum()), int((Ms == MAIN_MAXM).sum()), int((Ms > MAIN_MAXM).sum())
    print("160 reads: median M %d, %d with 100 <= M <= 112, %d with M = 112, %d with M > 112" % (np.median(Ms), top, last, over))
    assert top >= 10 and last >= 1 and over >= 5
    check_batches(monkeypatch, [[(S, j) for j in range(n)]])


def test_repeated_pass_with_mixed_lengths(torch_dev, mixed_eight, monkeypatch):
    rep = ref_set(genome_len=60000, cov=40, read_len=6000, seed=3, het=0.0)          # test_repeated_pass's set
    n = 40
    ends_d = 0
    for j in range(n):
        fw = rep.full(j)["fw"]
        ends_d += int(len(fw) > 0 and (fw == 3).any() and not (fw == 2).any())
    assert ends_d >= WAVE_READS, ends_d
    assert max(rep.M(j) for j in range(n)) <= MAIN_MAXM
    check_batches(monkeypatch, [[(rep, j) for j in range(n)] + mixed_eight])

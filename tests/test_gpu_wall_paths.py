"""k_wall_tasks / k_find_wall on the reads of tests/wall_path_inputs.py -- a set known to pass through every fork of the
two kernels (tests/test_wall_path_inputs.py asserts the reach table on the CPU) -- against the oracle.  `-m gpu`.

  * stage parity: STAGE_WALL records equal the oracle's find_wall (b e cb ce equal, pe peo_b peo_e bit for bit), then
    STAGE_REL records and the labels of classify, with the default knobs, find_rel as its own kernel, full records, no tables;
  * the device's own task counts: the words k_wall_tasks leaves per read for k_find_wall (cp_debug_task_counts) equal the
    account's n_c, n_t, n_live0 -- phase 1a (the register windows of the bases, the filters) on the device, and what ties
    the account, which says which fork a read takes, to what the device did.  The fourth word is k_wall_tasks' own list
    overflow (never: 2*n_c <= icap); the account's `overflow` is the reference's abort, which the device reports per
    batch: the reads with it set are exactly the ones that raise code -5 alone;
  * flag arrays left clean: a read that did not keep its flags on chip clears the cells it wrote, a read that overflowed
    its whole range; the arrays are zeroed only when they are allocated, so what a batch leaves behind the next one finds.
    Asserted directly (cp_debug_flag_bytes: no byte of either array is set between calls) and by its consequence (a second
    batch laid over the cells of the first);
  * read order inside a batch.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import wall_path_inputs as W
from test_oracle_wall import same_records

pytestmark = pytest.mark.gpu

KNOBS = ("CLASSPRO_FUSE_REL", "CLASSPRO_COMPACT_REL", "CLASSPRO_TABLES")


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def accepted(k=W.K):
    rs = W.reads() if k == W.K else W.reads_other_k(k)
    return [(r, e) for r, e in zip(rs, W.expected(k)) if e is not None]


def rejected():
    return [r for r, e in zip(W.reads(), W.expected()) if e is None]


def task_counts(clf, b):
    out = np.zeros((b.nreads, 4), np.int32)
    f = clf.L.cp_debug_task_counts
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_int64], C.c_int
    assert f(clf.ws, out.ctypes.data, b.nreads) == 0
    return out


def flag_bytes(clf):
    """Bytes of the two flag arrays of the wall stage that are not zero (cp_debug_flag_bytes: the whole buffers)."""
    out = np.zeros(2, np.int64)
    f = clf.L.cp_debug_flag_bytes
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p], C.c_int
    assert f(clf.ws, out.ctypes.data) == 0
    return list(out)


def live_record_bytes(clf, b):
    """The bytes of the live interval and reliable-interval records of the last run, and the reliable counts."""
    from classpro_amd.api import INTVL_DTYPE
    from classpro_amd._lib import check
    nc, ni, nr, off = clf.counts(b)
    tot = int(off[-1])
    iv = np.zeros((tot, INTVL_DTYPE.itemsize), np.uint8)
    rv = np.zeros((tot, INTVL_DTYPE.itemsize), np.uint8)
    check(clf.L.cp_get_intervals(clf.ws, iv.ctypes.data, rv.ctypes.data, tot))
    idx = np.arange(tot) - off[np.searchsorted(off, np.arange(tot), side="right") - 1]
    return iv[idx < np.repeat(ni, np.diff(off))].tobytes(), rv[idx < np.repeat(nr, np.diff(off))].tobytes(), nr.tobytes()


def check_stages(k, with_counts, harness=None):
    from classpro_amd.api import Classifier, Batch, STAGE_WALL, STAGE_REL
    acc = accepted(k)
    clf = Classifier(k, W.READ_LEN, W.HCOV, W.DCOV)
    b = Batch.from_reads([r.seq for r, _ in acc], [r.prof for r, _ in acc])
    clf.run(b, STAGE_WALL)
    clf.check()
    for (iv, _), (r, e) in zip(clf.intervals(b), acc):
        assert same_records(iv, e["wall"], fields=("b", "e", "cb", "ce")), r.name
    if with_counts:
        P = harness.hh_params_new(k, W.READ_LEN, W.HCOV, W.DCOV)
        for got, (r, _) in zip(task_counts(clf, b), acc):
            a = W.account(harness, P, r.seq, r.prof)
            print(r.name, list(got), a)
            assert list(got) == [a["n_c"], a["n_t"], a["n_live0"], 0], r.name
        harness.hh_params_free(C.c_void_p(P))
    clf.run(b, STAGE_REL)
    clf.check()
    for (iv, riv), (r, e) in zip(clf.intervals(b), acc):
        o_iv, o_riv = e["rel"]
        rel = o_iv["is_rel"] != 0
        assert same_records(iv, o_iv, fields=("b", "e", "cb", "ce", "is_rel")) and same_records(riv, o_riv), r.name
        assert np.array_equal(iv["ccb"][rel], o_iv["ccb"][rel]) and np.array_equal(iv["cce"][rel], o_iv["cce"][rel]), r.name
    raw = live_record_bytes(clf, b)
    lab = clf.classify(b).tobytes()
    off = 0
    for r, e in acc:
        assert lab[off:off + len(r.seq)] == e["lab"], r.name
        off += len(r.seq)
    clf.close()
    return raw + (lab,)


@functools.lru_cache(maxsize=None)
def default_run():
    return check_stages(W.K, False)


@pytest.mark.parametrize("knob", [None, "CLASSPRO_FUSE_REL", "CLASSPRO_COMPACT_REL", "CLASSPRO_TABLES"])
def test_stage_parity(torch_dev, monkeypatch, knob):
    """Against the oracle: the STAGE_WALL records (b e cb ce, the bits of pe peo_b peo_e), the STAGE_REL records (the same
    and is_rel of every interval, ccb / cce of the reliable ones, the reliable records in full: the bar of
    tests/test_gpu_reference.py -- ccb / cce of an interval that is not reliable hold, in the reference, what
    correct_wall_cnt's index-by-position stores left there, DESIGN.md 3.3, and nothing reads them) and the labels.  With
    a knob set to 0, in addition: the STAGE_REL records and the labels equal the default run's byte for byte."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    base = default_run()
    if knob:
        monkeypatch.setenv(knob, "0")
        assert check_stages(W.K, False) == base


@pytest.mark.parametrize("k", W.OTHER_K)
def test_one_lane_replay_at_other_k(torch_dev, harness, monkeypatch, k):
    """Row 12: the reads whose SELF memo is off chip at K = 25 (the one-lane replay keeps its paired-flag window) and at
    K = 101 (it reads the flag array): stages, labels and the device's task counts."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    check_stages(k, True, harness)


def test_device_task_counts_equal_the_account(torch_dev, harness):
    from classpro_amd.api import Classifier, Batch, STAGE_WALL
    from classpro_amd._lib import ClassProError
    rs = W.reads()
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    b = Batch.from_reads([r.seq for r in rs], [r.prof for r in rs])       # every read, the ones the reference aborts on too
    clf.run(b, STAGE_WALL)
    with pytest.raises(ClassProError) as ei:
        clf.check()
    assert ei.value.code == -5
    got = task_counts(clf, b)
    P = harness.hh_params_new(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    for g, r in zip(got, rs):
        a = W.account(harness, P, r.seq, r.prof)
        print(r.name, list(g), a)
        assert list(g) == [a["n_c"], a["n_t"], a["n_live0"], 0], r.name
    harness.hh_params_free(C.c_void_p(P))
    for r in rejected():                                                  # the account's overflow: code -5 for the read alone
        with pytest.raises(ClassProError) as ei:
            clf.classify(Batch.from_reads([r.seq], [r.prof]))
        assert ei.value.code == -5, r.name
    clf.close()


@functools.lru_cache(maxsize=None)
def second_batch():
    """The set in reversed order, then 100 reads of a generated data set: (seqs, profs, labels of the oracle)."""
    from classpro_amd import synth
    from oracle.oracle import Oracle
    ds = synth.make_dataset(genome_len=200000, cov=40, read_len=10000, seed=5)
    O = Oracle(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    acc = accepted()[::-1]
    seqs, profs = [r.seq for r, _ in acc] + list(ds["seqs"][:100]), [r.prof for r, _ in acc] + list(ds["profiles"][:100])
    lab = b"".join(e["lab"] for _, e in acc) + b"".join(O.classify_read(s, p) for s, p in zip(ds["seqs"][:100], ds["profiles"][:100]))
    return seqs, profs, lab


@pytest.mark.parametrize("first", ["set", "set_with_aborting_reads", "aborting_read_alone"])
def test_flag_arrays_left_clean(torch_dev, first):
    """Classify the set, then -- same Classifier -- the set reversed followed by 100 generated reads: another read lies
    over every cell of the flag arrays that a read of the first batch wrote and should have cleared.  The same after a
    batch that holds the reads the reference aborts on (code -5; their whole range is cleared), and after such a read alone.
    The arrays are zeroed when they are allocated and an allocation that grows replaces them: the second batch, the larger
    one, runs once before the sequence, so that nothing is allocated (workspace_bytes stays) between the two."""
    from classpro_amd.api import Classifier, Batch
    from classpro_amd._lib import ClassProError
    seqs2, profs2, lab2 = second_batch()
    acc, rej = accepted(), rejected()
    assert len(rej) >= 3
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    b2 = Batch.from_reads(seqs2, profs2)
    assert clf.classify(b2).tobytes() == lab2
    assert flag_bytes(clf) == [0, 0]
    size = clf.workspace_bytes()
    if first == "set":
        b1 = Batch.from_reads([r.seq for r, _ in acc], [r.prof for r, _ in acc])
        assert clf.classify(b1).tobytes() == b"".join(e["lab"] for _, e in acc)
    else:
        rs = list(W.reads()) if first == "set_with_aborting_reads" else rej[:1]
        with pytest.raises(ClassProError) as ei:
            clf.classify(Batch.from_reads([r.seq for r in rs], [r.prof for r in rs]))
        assert ei.value.code == -5
    assert flag_bytes(clf) == [0, 0]                       # (the direct form of the claim; what follows is its consequence)
    assert clf.classify(b2).tobytes() == lab2
    assert flag_bytes(clf) == [0, 0]
    assert clf.workspace_bytes() == size
    clf.close()


def test_flag_arrays_clean_after_each_read_alone(torch_dev):
    """Every read of the set alone in a batch, the aborting ones too: not a byte of the flag arrays is left set, whichever
    way the read cleans up after itself (flags never off the chip; the candidates and the ends of its E-intervals; its
    whole range after an overflow)."""
    from classpro_amd.api import Classifier, Batch
    from classpro_amd._lib import ClassProError
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    for r, e in zip(W.reads(), W.expected()):
        b = Batch.from_reads([r.seq], [r.prof])
        if e is None:
            with pytest.raises(ClassProError):
                clf.classify(b)
        else:
            assert clf.classify(b).tobytes() == e["lab"], r.name
        assert flag_bytes(clf) == [0, 0], r.name
    clf.close()


def test_read_order_inside_a_batch(torch_dev):
    from classpro_amd.api import Classifier, Batch
    acc = accepted()
    order = np.random.default_rng(17).permutation(len(acc))
    acc = [acc[i] for i in order]
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    lab = clf.classify(Batch.from_reads([r.seq for r, _ in acc], [r.prof for r, _ in acc])).tobytes()
    off = 0
    for r, e in acc:
        assert lab[off:off + len(r.seq)] == e["lab"], r.name
        off += len(r.seq)
    clf.close()

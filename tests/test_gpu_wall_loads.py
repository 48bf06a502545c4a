"""k_wall_tasks with its lists on chip and cp_wall_candidate_live with its loads in groups, on the reads of
tests/wall_load_inputs.py (the edges of both: tests/test_wall_load_inputs.py) plus the 59 of tests/wall_path_inputs.py,
against the oracle, at the bar of tests/test_gpu_wall_paths.py.  `-m gpu`.

  * stage parity at STAGE_WALL, STAGE_REL and on the whole path, under the default knobs, without tables
    (CLASSPRO_TABLES=0: every look-up computed on the spot) and with a Skellam table of 1 MB (look-ups beyond it);
  * the device's task counts equal the account;
  * flag arrays zero afterwards;
  * the same reads reversed and interleaved give the same per-read records and labels: a read leaves nothing on chip
    for the one the next block of its SIMD takes up.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import wall_path_inputs as W
import wall_load_inputs as L
from test_oracle_wall import same_records
from test_gpu_wall_paths import task_counts, flag_bytes

pytestmark = pytest.mark.gpu

KNOBS = ("CLASSPRO_FUSE_REL", "CLASSPRO_COMPACT_REL", "CLASSPRO_TABLES", "CLASSPRO_SKELLAM_TABLE_MB")


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def accepted():
    """(read, oracle's results) of both sets, without the reads the reference aborts on."""
    both = list(zip(L.reads(), L.expected())) + list(zip(W.reads(), W.expected()))
    return tuple((r, e) for r, e in both if e is not None)


def fields(rec):
    """The named fields of interval records as bytes (the six bytes of padding in a record belong to nobody)."""
    return b"".join(np.ascontiguousarray(rec[f]).tobytes() for f in rec.dtype.names)


def per_read(clf, b, acc, order):
    """Stages and labels of batch b (reads acc[order[k]]) against the oracle; returns per read, by its index in acc,
    the bytes of its STAGE_REL records, its reliable records and its labels."""
    from classpro_amd.api import STAGE_WALL, STAGE_REL
    clf.run(b, STAGE_WALL)
    clf.check()
    for (iv, _), k in zip(clf.intervals(b), order):
        r, e = acc[k]
        assert same_records(iv, e["wall"], fields=("b", "e", "cb", "ce")), r.name
    clf.run(b, STAGE_REL)
    clf.check()
    out = {}
    for (iv, riv), k in zip(clf.intervals(b), order):
        r, e = acc[k]
        o_iv, o_riv = e["rel"]
        rel = o_iv["is_rel"] != 0
        assert same_records(iv, o_iv, fields=("b", "e", "cb", "ce", "is_rel")) and same_records(riv, o_riv), r.name
        assert np.array_equal(iv["ccb"][rel], o_iv["ccb"][rel]) and np.array_equal(iv["cce"][rel], o_iv["cce"][rel]), r.name
        out[k] = [fields(iv), fields(riv)]
    lab = clf.classify(b).tobytes()
    off = 0
    for k in order:
        r, e = acc[k]
        assert lab[off:off + len(r.seq)] == e["lab"], r.name
        out[k].append(lab[off:off + len(r.seq)])
        off += len(r.seq)
    assert flag_bytes(clf) == [0, 0]
    return out


def run_order(order):
    from classpro_amd.api import Classifier, Batch
    acc = accepted()
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    b = Batch.from_reads([acc[k][0].seq for k in order], [acc[k][0].prof for k in order])
    out = per_read(clf, b, acc, order)
    clf.close()
    return out


@functools.lru_cache(maxsize=None)
def default_run():
    return run_order(tuple(range(len(accepted()))))


@pytest.mark.parametrize("knob", [None, ("CLASSPRO_TABLES", "0"), ("CLASSPRO_SKELLAM_TABLE_MB", "1")])
def test_stage_parity(torch_dev, monkeypatch, knob):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    base = default_run()
    if knob:
        monkeypatch.setenv(*knob)
        assert run_order(tuple(range(len(accepted())))) == base


def test_device_task_counts_equal_the_account(torch_dev, harness, monkeypatch):
    from classpro_amd.api import Classifier, Batch, STAGE_WALL
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    acc = accepted()
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    b = Batch.from_reads([r.seq for r, _ in acc], [r.prof for r, _ in acc])
    clf.run(b, STAGE_WALL)
    clf.check()
    P = harness.hh_params_new(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    for got, (r, _) in zip(task_counts(clf, b), acc):
        a = W.account(harness, P, r.seq, r.prof)
        assert list(got) == [a["n_c"], a["n_t"], a["n_live0"], 0], r.name
    harness.hh_params_free(C.c_void_p(P))
    assert flag_bytes(clf) == [0, 0]
    clf.close()


@pytest.mark.parametrize("how", ["reversed", "interleaved"])
def test_read_order(torch_dev, monkeypatch, how):
    """A read of 255 candidates fills every row of the lists on chip; whatever read follows it must find nothing of it."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    base = default_run()
    n = len(accepted())
    if how == "reversed":
        order = tuple(range(n))[::-1]
    else:                                                  # the reads of many candidates, each followed by short ones
        by_nc = sorted(range(n), key=lambda k: -len(accepted()[k][0].prof))
        half = (n + 1) // 2
        order = tuple(k for pair in zip(by_nc[:half], by_nc[half:][::-1] + [None]) for k in pair if k is not None)
        assert sorted(order) == list(range(n))
    assert run_order(order) == base

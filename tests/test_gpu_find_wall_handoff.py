"""The task records k_wall_tasks hands to k_find_wall (position, pass, wall type and candidate row in the record; one
load group per replay chunk; the head's loads in three rounds), on the reads of tests/find_wall_handoff_inputs.py (their
edges: tests/test_find_wall_handoff_inputs.py) together with the 43 of tests/wall_load_inputs.py and the 59 of
tests/wall_path_inputs.py in one batch, against the oracle, at the bar of tests/test_gpu_wall_loads.py.  `-m gpu`.

  * stage parity at STAGE_WALL, STAGE_REL and on the whole path, under the default knobs, without tables
    (CLASSPRO_TABLES=0) and with find_rel as a kernel of its own (CLASSPRO_FUSE_REL=0): equal records and labels;
  * the device's task counts equal the account;
  * flag arrays zero afterwards;
  * the same reads reversed and interleaved give the same per-read records and labels: nothing of a read stays in LDS
    for the one the next block of its SIMD takes up.
"""
import ctypes as C
import functools

import pytest

import wall_path_inputs as W
import wall_load_inputs as L
import find_wall_handoff_inputs as F
from test_gpu_wall_paths import task_counts, flag_bytes
from test_gpu_wall_loads import per_read, KNOBS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@functools.lru_cache(maxsize=None)
def accepted():
    """(read, oracle's results) of the three sets, without the reads the reference aborts on (none of the new ones)."""
    new = list(zip(F.reads(), F.expected()))
    assert all(e is not None for _, e in new)
    both = new + list(zip(L.reads(), L.expected())) + list(zip(W.reads(), W.expected()))
    return tuple((r, e) for r, e in both if e is not None)


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


@pytest.mark.parametrize("knob", [None, ("CLASSPRO_TABLES", "0"), ("CLASSPRO_FUSE_REL", "0")])
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
        if len(r.prof) == 0:                               # no k-mer: nothing to walk
            assert list(got)[:3] == [0, 0, 0], r.name
            continue
        a = W.account(harness, P, r.seq, r.prof)
        assert list(got) == [a["n_c"], a["n_t"], a["n_live0"], 0], r.name
    harness.hh_params_free(C.c_void_p(P))
    assert flag_bytes(clf) == [0, 0]
    clf.close()


@pytest.mark.parametrize("how", ["reversed", "interleaved"])
def test_read_order(torch_dev, monkeypatch, how):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    base = default_run()
    n = len(accepted())
    if how == "reversed":
        order = tuple(range(n))[::-1]
    else:                                                  # the long reads, each followed by a short one
        by_len = sorted(range(n), key=lambda k: -len(accepted()[k][0].prof))
        half = (n + 1) // 2
        order = tuple(k for pair in zip(by_len[:half], by_len[half:][::-1] + [None]) for k in pair if k is not None)
        assert sorted(order) == list(range(n))
    assert run_order(order) == base

"""cp_rel_counts with both step sums of an interval's end in one pass (cp_wall.h), on the device: the reads of
tests/find_rel_pair_inputs.py (their forks: tests/test_find_rel_pair_inputs.py) in one batch with the 59 of
tests/wall_path_inputs.py and the 20 of tests/find_wall_handoff_inputs.py, against the oracle, at the bar of
tests/test_gpu_wall_loads.py.  `-m gpu`.

  * stage parity at STAGE_WALL, STAGE_REL and on the whole path (equal records and labels; ccb / cce of every reliable
    interval, and for the new reads of every interval that passes the record-only tests, reliable or not), under the
    default knobs (find_rel inside k_find_wall), with find_rel as a kernel of its own (CLASSPRO_FUSE_REL=0: k_find_rel,
    through the same function with its LDS windows) and without tables (CLASSPRO_TABLES=0);
  * each of the three in the given, the reversed and an interleaved read order, with equal per-read results.
"""
import functools

import numpy as np
import pytest

import wall_path_inputs as W
import find_wall_handoff_inputs as H
import find_rel_pair_inputs as F
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
    both = new + list(zip(H.reads(), H.expected())) + list(zip(W.reads(), W.expected()))
    return tuple((r, e) for r, e in both if e is not None)


@functools.lru_cache(maxsize=None)
def passing():
    """Per new read (by its index in accepted()), the indices of the intervals that pass the record-only tests."""
    return {k: np.array([d["idx"] for d in F.forks(r, e)], np.int64) for k, (r, e) in enumerate(accepted()[:len(F.reads())])}


def orders():
    n = len(accepted())
    by_len = sorted(range(n), key=lambda k: -len(accepted()[k][0].prof))
    half = (n + 1) // 2                                    # the long reads, each followed by a short one
    inter = tuple(k for pair in zip(by_len[:half], by_len[half:][::-1] + [None]) for k in pair if k is not None)
    assert sorted(inter) == list(range(n))
    return {"given": tuple(range(n)), "reversed": tuple(range(n))[::-1], "interleaved": inter}


def run_order(order):
    from classpro_amd.api import Classifier, Batch, STAGE_REL
    acc = accepted()
    clf = Classifier(W.K, W.READ_LEN, W.HCOV, W.DCOV)
    b = Batch.from_reads([acc[k][0].seq for k in order], [acc[k][0].prof for k in order])
    out = per_read(clf, b, acc, order)
    clf.run(b, STAGE_REL)
    clf.check()
    for (iv, _), k in zip(clf.intervals(b), order):
        if k in passing():
            r, e = acc[k]
            p, o_iv = passing()[k], e["rel"][0]
            assert np.array_equal(iv["ccb"][p], o_iv["ccb"][p]) and np.array_equal(iv["cce"][p], o_iv["cce"][p]), r.name
    clf.close()
    return out


@functools.lru_cache(maxsize=None)
def default_run():
    return run_order(orders()["given"])


@pytest.mark.parametrize("how", ["given", "reversed", "interleaved"])
@pytest.mark.parametrize("knob", [None, ("CLASSPRO_FUSE_REL", "0"), ("CLASSPRO_TABLES", "0")])
def test_stages_and_labels(torch_dev, monkeypatch, knob, how):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    base = default_run()
    if knob:
        monkeypatch.setenv(*knob)
    if knob or how != "given":
        assert run_order(orders()[how]) == base

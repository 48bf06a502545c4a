"""bench.py --dump-outputs: the sampling, gathering and writing helpers on host tensors whose labels are known, laid out
as the bench lays them out (sub-batches inside resident windows, one share of reads per rank)."""
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402


def _layout(nreads=1500, seed=0):
    rng = np.random.default_rng(seed)
    so_all = np.concatenate([[0], np.cumsum(rng.integers(5000, 30000, nreads))]).astype(np.int64)
    labels = torch.from_numpy(rng.choice(np.frombuffer(b"NEHDR", dtype=np.uint8), int(so_all[-1])))
    return so_all, labels


def _batch(so_all, labels, r0, n):
    """A (rd, b) pair as bench.make_batches builds it: global first read, local offsets, the batch's own label array."""
    so = so_all[r0:r0 + n + 1] - so_all[r0]
    b = types.SimpleNamespace(labels=labels[so_all[r0]:so_all[r0 + n]].clone(), total_bases=int(so[-1]))
    return dict(first=r0, nreads=n, seq_off_h=so), b


def test_dump_matches_known_labels(tmp_path):
    so_all, labels = _layout()
    first, last = 100, 1400
    sample = bench.dump_sample(so_all, first, last)
    assert np.array_equal(sample, bench.dump_sample(so_all, first, last))          # the same reads on every run
    assert (np.diff(sample) > 0).all() and sample[0] >= first and sample[-1] < last
    assert 0 < np.diff(so_all)[sample].sum() <= bench.DUMP_SAMPLE_BASES
    parts, counts = [], np.zeros(256, dtype=np.int64)
    bench.collect_outputs([_batch(so_all, labels, 100, 500), _batch(so_all, labels, 600, 200)], sample, parts, counts)  # window 1
    bench.collect_outputs([_batch(so_all, labels, 800, 600)], sample, parts, counts)                                     # window 2
    bench.write_outputs(str(tmp_path), "", so_all, sample, parts, counts)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["label_counts", "labels", "labels_read_index", "labels_read_offset"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES
    assert np.array_equal(got["labels_read_index"], sample)
    off = got["labels_read_offset"].astype(np.int64)
    for j, r in enumerate(sample):
        want = labels[so_all[r]:so_all[r + 1]].numpy()
        assert np.array_equal(got["labels"][off[j]:off[j + 1]], want.astype(np.float32)), "read %d" % r
    assert np.array_equal(got["label_counts"], np.bincount(labels[so_all[first]:so_all[last]].numpy(), minlength=256))


def test_dump_budget_is_shared_by_the_ranks():
    so_all, _ = _layout(nreads=6000, seed=1)
    for world in (1, 2, 8):
        bounds = np.linspace(0, len(so_all) - 1, world + 1).astype(int)
        bases = sum(np.diff(so_all)[bench.dump_sample(so_all, bounds[r], bounds[r + 1], world)].sum() for r in range(world))
        assert 0 < bases <= bench.DUMP_SAMPLE_BASES
        assert 4 * bases + world * (256 * 8 + 2 * 8 * 2000) <= bench.DUMP_MAX_BYTES     # labels, counts, index + offsets


def test_bench_has_full_and_dump_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr

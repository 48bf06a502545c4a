"""The filtered count table without a GPU: the numpy model of the filter (tests/kfilter_model.py) on the fixture the GPU
tests use, inside the caps they assert, the usage errors of `kprof -f` -- reported before the GPU is touched -- and the
Python mirror of the new calls."""
import os
import subprocess

import pytest

import kfilter_model as M
import kprof_oracle as O
from conftest import ROOT

KPROF = os.path.join(ROOT, "classpro_amd", "kprof")
NO_GPU = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
K = 40
DISTINCT, SINGLE = 161558, 110939          # the fixture at K = 40: distinct keys, and those that occur once


def test_python_mirror_is_present():
    from classpro_amd import _lib, api
    assert all(hasattr(api.KmerCounts, m) for m in ("mark", "mark_tensors", "filter_stats"))
    assert {"cp_kmer_counts_create_filtered", "cp_kmer_counts_mark", "cp_kmer_counts_filter_stats"} <= set(_lib.SYMBOLS)
    assert [f for f, _ in _lib.KmerFilterStats._fields_] == ["filter_bits", "filter_bytes", "n_marked", "n_counted",
                                                             "n_table_keys", "n_outside", "n_false"]


def test_model_stays_inside_the_caps_of_the_gpu_tests():
    """The sequential model of the hash the library uses, on the fixture: the false positives stay below the caps that
    tests/test_gpu_kfilter.py asserts (1 % of the singletons at 2^24 bits, 10 % at 2^20), and the identities hold that
    hold for any order."""
    from classpro_amd import api, synth
    assert hasattr(api.KmerCounts, "mark")                 # the calls this models
    ds = synth.make_dataset(genome_len=60000, cov=30, read_len=6000, seed=11)
    cnt, _, skipped = O.count([bytes(s) for s in ds["seqs"]], K)
    keyed = {M.key_of(k): c for k, c in cnt.items()}       # first-occurrence order is kept
    single = sum(1 for c in cnt.values() if c == 1)
    assert (len(keyed), single, skipped) == (DISTINCT, SINGLE, 0)
    for bits, cap in ((1 << 24, 0.01), (1 << 20, 0.10), (64, None)):
        r = M.simulate(keyed, bits)
        print("filter_bits %d: %r" % (bits, r))
        assert r["n_table_keys"] - r["n_false"] == DISTINCT - SINGLE == 50619
        assert r["n_table_keys"] + r["n_outside"] == DISTINCT and r["n_outside"] <= bits
        if cap is not None:
            assert r["n_false"] <= cap * SINGLE
        else:
            assert r["n_outside"] <= 64 and r["n_table_keys"] >= DISTINCT - 64
    assert M.simulate(keyed, 1 << 24)["n_outside"] > 100000


def test_usage_errors_of_the_filter_option_without_a_gpu(built, tmp_path):
    """HIP sees no device here, so a command that touched the GPU first could not answer like this."""
    d = str(tmp_path)
    env = dict(os.environ, **NO_GPU)
    src = os.path.join(d, "reads.fasta")
    with open(src, "wb") as f:
        f.write(b">r1\nACGTACGTAC\n")
    run = lambda *a: subprocess.run([KPROF] + list(a), capture_output=True, text=True, env=env)
    for bad in ("-f", "-fx", "-f1.5", "-f16M"):
        r = run(bad, src)
        assert (r.returncode, r.stdout) == (1, "") and r.stderr == "kprof: -f '%s' argument is not an integer\n" % bad[2:]
    for bad in ("-1", "131073", "99999999999999999999"):
        r = run("-f" + bad, src)
        assert (r.returncode, r.stdout) == (1, "")
        assert r.stderr == "kprof: Filter size must lie in [0, 131072] MiB (%s)\n" % bad
    r = run("-f16", "-k64", src)                           # the other usage errors still come first
    assert r.returncode == 1 and r.stderr == "kprof: K-mer length must lie in [2, 63] (64)\n"
    r = run("-f16", os.path.join(d, "nope"))
    assert r.returncode == 1 and r.stderr.startswith("kprof: Cannot open ")
    assert sorted(os.listdir(d)) == ["reads.fasta"]

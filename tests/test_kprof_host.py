"""kprof without a GPU: the brute-force oracle of tests/kprof_oracle.py against an independent numpy restatement, the
histograms it gives for the two synthetic sets the GPU tests and the docs use (their peaks are where ClassPro's
histogram reader needs them), and the built command's error contract -- reported before the GPU is touched."""
import os
import subprocess

import numpy as np
import pytest

import kprof_oracle as O
from conftest import ROOT

KPROF = os.path.join(ROOT, "classpro_amd", "kprof")
NO_GPU = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


def numpy_counts(seqs, k):
    """Independent restatement for k <= 31: canonical keys as uint64, sorted, np.unique with counts.
    Returns (per-read profiles, sorted counts of the distinct keys, skipped positions)."""
    code = np.full(256, 4, np.uint64)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    keys, valid = [], []
    for s in seqs:
        b = code[np.frombuffer(bytes(s), np.uint8)]
        n = max(len(b) - k + 1, 0)
        fw, rc, ok = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.ones(n, bool)
        for j in range(k):
            bj = b[j:j + n]
            ok &= bj < 4
            bj = np.minimum(bj, np.uint64(3))
            fw = fw * np.uint64(4) + bj
            rc = rc + ((np.uint64(3) - bj) << np.uint64(2 * j))
        keys.append(np.minimum(fw, rc))
        valid.append(ok)
    allk = np.concatenate([kk[v] for kk, v in zip(keys, valid)]) if keys else np.zeros(0, np.uint64)
    u, c = np.unique(allk, return_counts=True)
    prof = []
    for kk, v in zip(keys, valid):
        p = np.minimum(c[np.searchsorted(u, kk[v])], O.MAXC) if v.any() else np.zeros(0, np.int64)
        out = np.zeros(len(kk), np.uint16)
        out[v] = p
        prof.append(out)
    return prof, np.sort(c), int(sum((~v).sum() for v in valid))


def test_oracle_agrees_with_numpy_restatement():
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = acgt[rng.integers(0, 4, 3000)]
    rc = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for i in range(60):
        a = int(rng.integers(0, 2500))
        s = bytes(genome[a:a + int(rng.integers(5, 500))])
        seqs.append(s.translate(rc)[::-1] if i % 2 else s)
    seqs += [b"", b"ACG", b"ACGT" * 8, seqs[0][:40] + b"N" + seqs[0][40:], b"acgtACGTACGTACGTACGTACGTAC\0ACGTTGCATGCATGCAGTCAGTCA"]
    for k in (2, 16, 21, 31):
        want = O.run(seqs, k)
        prof, counts, skipped = numpy_counts(seqs, k)
        assert all(np.array_equal(a, b) for a, b in zip(prof, want["profiles"])) and len(prof) == len(want["profiles"])
        assert np.array_equal(counts, np.sort(np.array(list(want["counter"].values()), np.int64)))
        assert skipped == want["stats"]["n_skipped"] and want["stats"]["n_kmers"] == int(counts.sum())
        low, high, il, ih, h = want["hist"]
        assert (low, high, ih) == (1, 32767, 0) and il == h[0] == int((counts == 1).sum())
        assert np.array_equal(h, np.bincount(counts, minlength=32768)[1:])


def test_oracle_hidden_cells_at_saturation():
    seqs = [b"A" * 1000] * 20 + [b"T" * 1000] * 20
    want = O.run(seqs, 40)
    low, high, il, ih, h = want["hist"]
    assert (il, ih) == (0, 38440) and h[32766] == 1 and h.sum() == 1
    assert all((p == 32767).all() and len(p) == 961 for p in want["profiles"])


@pytest.mark.parametrize("args,peak", [(dict(genome_len=60000, cov=30, read_len=6000, seed=11), 31),
                                       (dict(genome_len=200000, cov=40, read_len=10000, seed=1), 37)], ids=["60k", "200k"])
def test_counted_histogram_has_the_peak_classpro_needs(built, args, peak):
    """The tallest occurrence-weighted peak of the counted histogram, and cp_hist_covs' verdict on it: a peak >= 10 is
    found, so neither ClassPro nor the reference's reader stops on files made from these sets."""
    from classpro_amd import synth
    from classpro_amd.api import hist_covs
    ds = synth.make_dataset(**args)
    cnt, _, skipped = O.count([bytes(s) for s in ds["seqs"]], 40)
    low, high, il, ih, h = O.hist(cnt)
    assert skipped == 0 and ih == 0
    w = h * np.arange(1, 32768)                                # occurrences per count
    inner = np.flatnonzero((w[1:-1] > w[:-2]) & (w[1:-1] >= w[2:])) + 1       # local maxima; count 1, the error
    assert int(inner[np.argmax(w[inner])]) + 1 == peak                        # k-mers' falling edge, is none
    hc, dc = hist_covs(h, low, high, il, ih, 0)
    assert dc >= 10 and hc >= 10 // 2


def test_command_is_built(built):
    assert os.path.exists(KPROF) and os.access(KPROF, os.X_OK), "classpro_amd/kprof was not built"


def test_error_contract_without_a_gpu(built, tmp_path):
    """HIP sees no device here, so a command that touched the GPU first could not answer like this."""
    d = str(tmp_path)
    env = dict(os.environ, **NO_GPU)
    src = os.path.join(d, "reads.fasta")
    with open(src, "wb") as f:
        f.write(b">r1\nACGTACGTAC\n")
    run = lambda *a: subprocess.run([KPROF] + list(a), capture_output=True, text=True, env=env)
    usage = "Usage: kprof [-v] [-k<int(40)>] [-T<int(4)>] [-N<out_root>] <source>[.db|.dam|.f[ast][aq][.gz]]\n"
    for a in ([], ["-v"], [src, src]):
        r = run(*a)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", usage), a
    r = run("-q", src)
    assert r.returncode == 1 and r.stderr == "kprof: -q is an illegal option\n"
    for k in ("1", "64", "100"):
        r = run("-k" + k, src)
        assert r.returncode == 1 and r.stderr == "kprof: K-mer length must lie in [2, 63] (%s)\n" % k
    for bad in ("-k0", "-kx", "-T0", "-k"):
        r = run(bad, src)
        assert r.returncode == 1 and r.stderr.startswith("kprof: ") and r.stdout == "", bad
    r = run(os.path.join(d, "nope"))
    assert r.returncode == 1 and r.stderr == "kprof: Cannot open %s/nope as a .db|.dam or .f{ast}[aq][.gz] file\n" % d
    r = run("-N" + os.path.join(d, "no_such_dir", "out"), src)
    assert r.returncode == 1 and r.stderr == "kprof: Cannot open %s/no_such_dir/out.hist for 'w'\n" % d
    assert sorted(os.listdir(d)) == ["reads.fasta"]


def test_python_mirror_is_present():
    from classpro_amd import api
    assert all(hasattr(api.KmerCounts, m) for m in ("add", "add_tensors", "profiles", "hist", "stats", "close"))
    assert callable(api.Batch.from_seqs)

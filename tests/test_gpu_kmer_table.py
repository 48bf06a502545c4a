"""The per-k-mer label table (cp_kmer_table_*, KmerTable, class2cns) on a real MI355X (`-m gpu`), against the Python
restatement of the reference pipeline in tests/cns_oracle.py: exact exports and statistics, order independence, key
edges, growth, the consensus tie rule, the command line, and a 200-Mbase set against a torch-side oracle."""
import os
import random
import subprocess

import numpy as np
import pytest

import cns_oracle as O
from conftest import ROOT

pytestmark = pytest.mark.gpu
K = 40
TOOLS = os.path.join(ROOT, "classpro_amd")


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def labelled(torch_dev):
    """A synth.make_dataset batch labelled on the device: (Batch, records)."""
    from classpro_amd import synth
    from classpro_amd.api import Batch, Classifier, hist_covs
    ds = synth.make_dataset(genome_len=60000, cov=30, read_len=6000, seed=11)
    low, high, il, ih, h = ds["hist"]
    hc, dc = hist_covs(h, low, high, il, ih, 0)
    clf = Classifier(K=K, read_len=20000, hcov=hc, dcov=dc)
    b = Batch.from_reads(ds["seqs"], ds["profiles"])
    lab = clf.classify(b)
    clf.close()
    so = b.seq_off_h
    recs = [(b"read%d" % (i + 1), bytes(ds["seqs"][i]), lab[so[i]:so[i + 1]].tobytes()) for i in range(b.nreads)]
    return b, recs, ds


def oracle_entries(t):
    ks = sorted(t)
    hi = np.array([k >> 63 for k in ks], np.uint64)
    lo = np.array([k & ((1 << 63) - 1) for k in ks], np.uint64)
    cnt = np.array([t[k] for k in ks], np.uint32).reshape(-1, 4)
    return hi, lo, cnt


def check_table(T, t, skipped):
    hi, lo, cnt = T.entries()
    ohi, olo, ocnt = oracle_entries(t)
    assert np.array_equal(hi, ohi) and np.array_equal(lo, olo) and np.array_equal(cnt, ocnt)
    s, want = T.stats(), O.stats(t, skipped)
    for k, v in want.items():
        if k == "consistency":
            assert (np.isnan(v) and np.isnan(s[k])) or s[k] == v, (k, s[k], v)      # bit for bit
        else:
            assert s[k] == v, (k, s[k], v)
    return s


def flat(torch, recs):
    seq = b"".join(r[1] for r in recs)
    lab = b"".join(r[2] for r in recs)
    off = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r[1]) for r in recs], out=off[1:])
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.frombuffer(x, np.uint8).copy() if x else np.zeros(1, np.uint8)).to(dev)
    return t(seq), torch.from_numpy(off).to(dev), t(lab)


@pytest.mark.parametrize("canonical", [False, True], ids=["forward", "canonical"])
def test_table_matches_oracle(labelled, canonical):
    from classpro_amd.api import KmerTable
    b, recs, _ = labelled
    T = KmerTable(K, canonical=canonical)
    T.add(b)
    t, skipped = O.table(recs, K, canonical)
    s = check_table(T, t, skipped)
    assert s["n_distinct"] > 1000 and s["n_kmers"] == b.total_kmers
    T.close()


def test_order_independence(torch_dev, labelled):
    from classpro_amd.api import KmerTable
    _, recs, _ = labelled
    results = []
    for canonical in (False, True):
        for parts in ([recs], [recs[:5], recs[5:40], recs[40:]], [recs[::-1]]):
            T = KmerTable(K, canonical=canonical)
            for p in parts:
                T.add_tensors(*flat(torch_dev, p))
            results.append((T.entries(), T.stats()))
            T.close()
        a = results[-3:]
        for e, s in a[1:]:
            assert all(np.array_equal(x, y) for x, y in zip(e, a[0][0]))
            assert {k: v for k, v in s.items() if k not in ("slots", "bytes", "growths")} == \
                   {k: v for k, v in a[0][1].items() if k not in ("slots", "bytes", "growths")}


def _labels(rng, n, k):
    return b"N" * min(n, k - 1) + bytes(rng.choice(b"EHDR") for _ in range(max(0, n - k + 1)))


def _rc(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@pytest.mark.parametrize("k", [2, 21, 31, 32, 33, 40, 63])
def test_key_edges(torch_dev, k):
    from classpro_amd.api import KmerTable
    rng = random.Random(k)
    seqs = [b"A" * (k + 20), b"T" * (k + 20), b"A" * (k - 1), b"", b"C" * k]
    half = bytes(rng.choice(b"ACGT") for _ in range(k // 2))
    if k % 2 == 0:
        seqs.append(half + _rc(half))                                           # a reverse-complement palindrome
    seqs.append(bytes(rng.choice(b"ACGT") for _ in range(3 * k)) + b"N" + bytes(rng.choice(b"ACGT") for _ in range(2 * k)))
    seqs.append(bytes(rng.choice(b"ACGTacgt") for _ in range(4 * k)))
    seqs.append(bytes(rng.choice(b"ACGT") for _ in range(5 * k + 3)))
    seqs.append(_rc(seqs[-1]))
    recs = [(b"r%d" % i, s, _labels(rng, len(s), k)) for i, s in enumerate(seqs)]
    for canonical in (False, True):
        T = KmerTable(k, canonical=canonical)
        T.add_tensors(*flat(torch_dev, recs))
        t, skipped = O.table(recs, k, canonical)
        s = check_table(T, t, skipped)
        assert s["n_skipped"] > 0
        hi, lo, _ = T.entries()
        top = (int(hi[-1]) << 63) | int(lo[-1])
        if not canonical:
            assert top == (1 << (2 * k)) - 1                                   # all-T: the largest key, not EMPTY
        T.close()


def test_bad_k_and_bad_label(torch_dev):
    from classpro_amd.api import KmerTable
    from classpro_amd._lib import ClassProError
    for k in (1, 64, 100):
        with pytest.raises(ClassProError):
            KmerTable(k)
    T = KmerTable(5)
    T.add_tensors(*flat(torch_dev, [(b"x", b"ACGTACGT", b"NNNNEHXD")]))
    with pytest.raises(ClassProError) as e:
        T.stats()
    assert e.value.code == -1
    T.close()


def test_growth(torch_dev):
    from classpro_amd.api import KmerTable
    rng = np.random.default_rng(5)
    k = 31
    recs = []
    for i in range(250):
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4000)])
        recs.append((b"g%d" % i, s, _labels(random.Random(i), len(s), k)))
    T = KmerTable(k, initial_slots=64)
    T.add_tensors(*flat(torch_dev, recs))
    t, skipped = O.table(recs, k)
    s = check_table(T, t, skipped)
    assert s["n_distinct"] > 900_000 and s["slots"] >= 2 * s["n_distinct"] and s["growths"] > 0
    T.close()


@pytest.mark.parametrize("canonical", [False, True], ids=["forward", "canonical"])
def test_growth_across_batches(torch_dev, canonical):
    """Three batches of about 39 400 new keys each into 64 slots: the first grows the table to 2^17 slots inside its add,
    the second passes half of that, so its growth rehashes a table that already holds the counts of an earlier batch."""
    from classpro_amd.api import KmerTable
    rng = np.random.default_rng(17)
    k = 31
    recs = []
    for i in range(60):
        s = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000)])
        recs.append((b"b%d" % i, s, _labels(random.Random(100 + i), len(s), k)))
    t, skipped = O.table(recs, k, canonical)
    got = []
    for slots in (64, 1 << 20):
        T = KmerTable(k, canonical=canonical, initial_slots=slots)
        for b in (recs[:20], recs[20:40], recs[40:]):
            T.add_tensors(*flat(torch_dev, b))
        got.append((T.entries(), check_table(T, t, skipped)))
        T.close()
    (e_small, s_small), (e_big, s_big) = got
    assert s_small["growths"] >= 2 and s_big["growths"] == 0 and s_big["slots"] == 1 << 20
    assert all(np.array_equal(x, y) for x, y in zip(e_small, e_big))
    drop = ("slots", "bytes", "growths")
    assert {k_: v for k_, v in s_small.items() if k_ not in drop} == {k_: v for k_, v in s_big.items() if k_ not in drop}


def test_consensus(torch_dev, labelled):
    from classpro_amd.api import KmerTable
    k = 5
    ties = {b"ACGTT": b"EH", b"CCGTA": b"HD", b"GGATC": b"DR", b"TTACA": b"EHDR", b"AAACC": b"EEHHH"}
    recs = [(b"t", km, b"NNNN" + bytes([c])) for km, labs in ties.items() for c in labs]
    T = KmerTable(k)
    seq, off, lab = flat(torch_dev, recs)
    T.add_tensors(seq, off, lab)
    got = T.consensus_tensors(seq, off, lab).cpu().numpy().tobytes()
    want = {b"ACGTT": b"H", b"CCGTA": b"D", b"GGATC": b"R", b"TTACA": b"R", b"AAACC": b"H"}
    assert got == b"".join(b"NNNN" + want[km] for km, labs in ties.items() for _ in labs)
    T.close()
    b, recs, _ = labelled
    for canonical in (False, True):
        T = KmerTable(K, canonical=canonical)
        T.add(b)
        out = T.consensus(b)[:b.total_bases].cpu().numpy().tobytes()
        t, _ = O.table(recs, K, canonical)
        assert out == b"".join(r[2] for r in O.consensus_records(recs, K, t, canonical))
        T.stats()                                                  # no deferred error
        T.close()


def test_cli(labelled, tmp_path):
    from classpro_amd import fastk
    b, recs, ds = labelled
    d = str(tmp_path)
    recs = list(recs)
    recs.insert(3, (b"tiny", b"ACGTAC", b"NNNNNN"))
    est = os.path.join(d, "est.class")
    with open(est, "wb") as f:
        for i, (n, s, q) in enumerate(recs):
            f.write(b"@" + n + (b" some comment" if i % 3 == 0 else b"") + b"\n" + s + b"\n+\n" + q + b"\n")
    fastk.write_fastk(d, "reads", K, [np.zeros(max(len(r[1]) - K + 1, 0), np.uint16) for r in recs], ds["hist"])
    root = os.path.join(d, "reads")
    cns = os.path.join(TOOLS, "class2cns")
    run = lambda *a: subprocess.run([cns] + list(a), capture_output=True, check=True).stdout
    recs_in = O.read_class(est)
    env = dict(os.environ, LC_ALL="C")
    dumped = run(est, root)
    s = subprocess.run(["sort"], input=dumped, capture_output=True, env=env, check=True).stdout
    u = subprocess.run(["uniq", "-c"], input=s, capture_output=True, env=env, check=True).stdout
    assert run("-u", est, root) == u
    for canonical in (False, True):
        c = ["-c"] if canonical else []
        t, skipped = O.table(recs_in, K, canonical)
        st = O.stats(t, skipped)
        assert run(*c, "-u", est, root) == O.uniq_table(t, K)
        assert run(*c, "-x", est, root) == b"Overall consistency = %s\n" % repr(st["consistency"]).encode()
        out = os.path.join(d, "cns%d.class" % canonical)
        r = subprocess.run([cns] + c + ["-v", "-C" + out, est, root], capture_output=True, check=True)
        assert r.stdout == b"" and b"distinct" in r.stderr
        want = O.consensus_records(recs_in, K, t, canonical)
        with open(est, "rb") as f:
            hdrs = f.read().split(b"\n")[0::4]
        with open(out, "rb") as f:
            got = f.read()
        assert got == b"".join(b"%s\n%s\n+\n%s\n" % (h, s_, q) for h, (_, s_, q) in zip(hdrs, want))
        acc = subprocess.run([os.path.join(TOOLS, "class2acc"), out, est], capture_output=True)
        assert acc.returncode == 0 and b"Accuracy" in acc.stdout


def test_scale_against_torch_oracle(torch_dev):
    """200 Mbases of DeviceSynth, labelled by the classifier: distinct keys, label totals and the consistency against a
    torch-side oracle (packed keys, sorts, group sums)."""
    torch = torch_dev
    from classpro_amd.synth_dev import DeviceSynth
    from classpro_amd.api import Batch, Classifier, KmerTable, hist_covs
    ds = DeviceSynth(genome_len=5_000_000, cov=40, read_len=20000, K=K, seed=3)
    low, high, il, ih, h = ds.hist
    hc, dc = hist_covs(h, low, high, il, ih, 0)
    clf = Classifier(K=K, read_len=20000, hcov=hc, dcov=dc)
    T = KmerTable(K)
    rd = ds.reads(0, ds.n_reads)
    b = Batch.from_device(rd)
    clf.classify(b, check_overflow=True)
    T.add(b)
    s = T.stats()
    assert s["n_kmers"] == b.total_kmers and s["n_skipped"] == 0
    # torch oracle: key = hi (first 9 bases) : lo (last 31 bases) at every k-mer end
    code = torch.full((256,), -1, dtype=torch.int64, device=b.device)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    base = code[b.seq[:b.total_bases].long()]
    assert bool((base >= 0).all())
    pos = torch.arange(b.total_bases, device=b.device)
    rid = torch.searchsorted(b.seq_off, pos, right=True) - 1
    ends = pos[pos >= b.seq_off[rid] + K - 1]
    hi = torch.zeros_like(ends)
    lo = torch.zeros_like(ends)
    for j in range(K):
        bj = base[ends - (K - 1) + j]
        if j < 9:
            hi = hi * 4 + bj
        else:
            lo = lo * 4 + bj
    lab = torch.full((256,), -1, dtype=torch.int64, device=b.device)
    for i, c in enumerate(b"EHDR"):
        lab[c] = i
    lb = lab[b.labels[ends].long()]
    key = hi * (1 << 42) + (lo >> 20)                                     # 60 high bits; the rest breaks ties next
    order = torch.argsort(lo & ((1 << 20) - 1), stable=True)
    order = order[torch.argsort(key[order], stable=True)]
    hi, lo, lb = hi[order], lo[order], lb[order]
    new = torch.ones_like(hi, dtype=torch.bool)
    new[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    g = torch.cumsum(new.long(), 0) - 1
    ng = int(g[-1].item()) + 1
    cnt = torch.zeros(ng * 4, dtype=torch.int64, device=b.device)
    cnt.index_add_(0, g * 4 + lb, torch.ones_like(lb))
    cnt = cnt.view(ng, 4)
    tot, mx = cnt.sum(1), cnt.max(1).values
    q, r = tot // mx, tot % mx
    a1 = r << 32
    q1, r1 = a1 // mx, a1 % mx
    q2 = (r1 << 32) // mx
    S = (int(q.sum().item()) << 64) + (int(q1.sum().item()) << 32) + int(q2.sum().item())
    assert s["n_distinct"] == ng
    assert s["label_total"] == cnt.sum(0).cpu().tolist()
    assert s["s_fixed"] == S
    assert s["consistency"] == O.consistency(ng, S)
    T.close()
    clf.close()

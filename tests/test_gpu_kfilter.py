"""The filtered count table (cp_kmer_counts_create_filtered / _mark / _filter_stats, KmerCounts(filter_bits=...),
kprof -f) on a real MI355X (`-m gpu`), against the brute-force restatement in tests/kprof_oracle.py: profiles,
histogram with its hidden cells, n_kmers, n_distinct and n_skipped are those of the unfiltered table, exactly, for any
filter size, batching and order.  Everything is integers and bytes: the tolerance is zero."""
import os
import random
import subprocess

import numpy as np
import pytest

import kfilter_model as M
import kprof_oracle as O
from conftest import ROOT
from test_gpu_kprof import _rc, _write_source, check, flat, run_table, split

pytestmark = pytest.mark.gpu
K = 40
TOOLS = os.path.join(ROOT, "classpro_amd")
KPROF = os.path.join(TOOLS, "kprof")
DISTINCT, SINGLE = 161558, 110939          # the fixture at K = 40: distinct keys, and those that occur once


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def small(torch_dev):
    """The 60 kbp / 30x set and its oracle at K = 40."""
    from classpro_amd import synth
    ds = synth.make_dataset(genome_len=60000, cov=30, read_len=6000, seed=11)
    seqs = [bytes(s) for s in ds["seqs"]]
    return ds, seqs, O.run(seqs, K)


def run_filtered(torch, seqs, k, filter_bits, batches=None, **kw):
    """Marks `batches` (lists of reads; default: all in one), adds the same, then profiles all reads in one batch.
    Returns (profiles, hist, stats) as run_table does, and the filter statistics."""
    from classpro_amd.api import KmerCounts
    T = KmerCounts(k, filter_bits=filter_bits, **kw)
    for b in batches or [seqs]:
        T.mark_tensors(*flat(torch, b))
    for b in batches or [seqs]:
        T.add_tensors(*flat(torch, b))
    prof = split(T.profiles(flat(torch, seqs)), seqs, k)
    h, s, f = T.hist(), T.stats(), T.filter_stats()
    T.close()
    return (prof, h, s), f


def check_filtered(got, f, want):
    """Exact against the oracle, and what holds for every filtered table: the keys are in the table or outside, a key
    that occurs twice is in the table, and every key judged new set at least one fresh bit.  With the oracle's per-read
    k-mers (want["per"]) also cell by cell: a key that occurs twice never reads as 1."""
    s = check(got, want)
    twice = sum(1 for c in want["counter"].values() if c >= 2)
    assert f["n_marked"] == f["n_counted"] == s["n_kmers"]
    assert f["n_table_keys"] + f["n_outside"] == s["n_distinct"]
    assert f["n_table_keys"] - f["n_false"] == twice
    assert f["n_outside"] <= f["filter_bits"] and f["filter_bytes"] * 8 == f["filter_bits"]
    assert s["slots"] >= 2 * f["n_table_keys"] and s["bytes"] >= 32 * s["slots"] + f["filter_bytes"]
    for p, per in zip(got[0], want.get("per", ())):
        for c, km in zip(p.tolist(), per):
            assert km is None or (c >= 2) == (want["counter"][km] >= 2)
    return s


def oracle(seqs, k):
    cnt, per, skipped = O.count(seqs, k)
    return dict(profiles=O.profiles(cnt, per), hist=O.hist(cnt), stats=O.stats(cnt, skipped), counter=cnt, per=per)


@pytest.mark.parametrize("bits", [1 << 24, 1 << 20, 64])
def test_fixture_matches_oracle(torch_dev, small, bits):
    _, seqs, want = small
    got, f = run_filtered(torch_dev, seqs, K, bits)
    s = check_filtered(got, f, want)
    print("filter_bits %d: %r %r" % (bits, f, s))
    assert f["filter_bits"] == bits and s["n_distinct"] == DISTINCT and s["growths"] == 0
    assert f["n_table_keys"] - f["n_false"] == DISTINCT - SINGLE == 50619
    if bits == 1 << 24:
        assert f["n_false"] <= 0.01 * SINGLE and f["n_outside"] > 100000
    if bits == 1 << 20:
        assert f["n_false"] <= 0.10 * SINGLE


def test_filter_bits_are_rounded_up_and_bounded(torch_dev):
    from classpro_amd.api import KmerCounts
    from classpro_amd._lib import ClassProError
    for bits, want in ((64, 64), (65, 128), (1000, 1024), (1 << 20, 1 << 20)):
        T = KmerCounts(21, filter_bits=bits)
        assert T.filter_stats()["filter_bits"] == want
        T.close()
    for bits in (1, 63, -64, (1 << 40) + 1):
        with pytest.raises(ClassProError) as e:
            KmerCounts(21, filter_bits=bits)
        assert e.value.code == -1
    T = KmerCounts(21)                                     # no filter: today's object
    assert T.filter_stats()["filter_bits"] == 0
    T.close()


def test_fewer_slots_than_unfiltered(torch_dev, small):
    _, seqs, want = small
    got, f = run_filtered(torch_dev, seqs, K, 1 << 24, initial_slots=64)
    s = check_filtered(got, f, want)
    u = check(run_table(torch_dev, seqs, K, initial_slots=64), want)
    assert s["growths"] > 0 and s["slots"] >= 2 * f["n_table_keys"] and s["slots"] < u["slots"]


def test_first_batch_sizing(torch_dev):
    """A first marked batch past 2^21 bases sizes the default table to pow2(total_bases / 2) slots, a quarter of the
    unfiltered rule, and that is no growth step."""
    rng = np.random.default_rng(5)
    s = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150000)])
    seqs = [s] * 20                                         # 3 Mbases, 150 k distinct keys
    got, f = run_filtered(torch_dev, seqs, K, 1 << 22)
    prof, h, st = got
    total = sum(len(x) for x in seqs)
    assert st["slots"] == 1 << (total // 2 - 1).bit_length() == 1 << 21 and st["growths"] == 0
    n = len(s) - K + 1
    assert st["n_kmers"] == 20 * n and f["n_false"] == 0 and f["n_table_keys"] + f["n_outside"] == st["n_distinct"]
    assert all((p == 20).sum() >= n - 100 and (p % 20 == 0).all() for p in prof)


def test_model_predicts_a_sequential_run(torch_dev):
    """One k-mer per read and one read per mark call: the device's order is the model's, so the model of
    tests/kfilter_model.py must give the table keys, the false positives and the keys outside exactly."""
    from classpro_amd.api import KmerCounts
    rng = random.Random(41)
    uniq = [bytes(rng.choice(b"ACGT") for _ in range(K)) for _ in range(150)]
    seqs = uniq + [uniq[i] for i in range(0, 150, 5)] + [_rc(uniq[i]) for i in range(1, 150, 10)]
    rng.shuffle(seqs)
    cnt, _, _ = O.count(seqs, K)
    model = M.simulate({M.key_of(k): c for k, c in cnt.items()}, 256)
    assert 0 < model["n_false"] < model["n_table_keys"] and model["n_outside"] > 0
    T = KmerCounts(K, filter_bits=256)
    for s in seqs:
        T.mark_tensors(*flat(torch_dev, [s]))
    assert T.filter_stats()["n_table_keys"] == model["n_table_keys"]
    T.add_tensors(*flat(torch_dev, seqs))
    f = T.filter_stats()
    T.close()
    assert {k: f[k] for k in model} == model


def test_concurrent_first_occurrences(torch_dev):
    rng = random.Random(13)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    read = rnd(300)
    copies = [read] * 64 + [_rc(read)] * 64                 # every first occurrence of a key in one launch
    tandem = [rnd(50) + rnd(7) * 60 + rnd(50), rnd(200)]    # a key recurs inside one lane's 64 positions
    pal = b"ACGT" * 10
    assert _rc(pal) == pal
    for seqs in (copies, tandem, [pal, pal + b"ACG"]):
        want = oracle(seqs, K)
        for bits in (64, 1 << 16):
            got, f = run_filtered(torch_dev, seqs, K, bits)
            check_filtered(got, f, want)
    got, f = run_filtered(torch_dev, copies, K, 1 << 16)
    assert f["n_table_keys"] == 261 and f["n_outside"] == 0 and all((p == 128).all() for p in got[0])


def test_order_and_batching(torch_dev, small):
    _, seqs, want = small
    bits = 1 << 20
    got, f = run_filtered(torch_dev, seqs, K, bits, batches=[[s] for s in seqs])
    check_filtered(got, f, want)
    got, f = run_filtered(torch_dev, seqs, K, bits, batches=[seqs[:5], seqs[5:40], seqs[40:]])
    check_filtered(got, f, want)
    order = list(range(len(seqs)))
    random.Random(7).shuffle(order)
    sh = [seqs[i] for i in order]
    (prof, h, s), f = run_filtered(torch_dev, sh, K, bits)
    back = [None] * len(seqs)
    for pos, i in enumerate(order):
        back[i] = prof[pos]
    check_filtered((back, h, s), f, want)


def test_growth_and_replay(torch_dev):
    rng = np.random.default_rng(23)
    seqs = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000)]) for _ in range(60)]
    batches = [seqs[:20] * 2, seqs[20:40] * 2, seqs[40:] * 2]
    every = [s for b in batches for s in b]
    got, f = run_filtered(torch_dev, every, K, 1 << 22, batches=batches, initial_slots=64)
    s = check_filtered(got, f, oracle(every, K))
    assert s["growths"] >= 2 and f["n_table_keys"] > 100000


@pytest.mark.parametrize("k", [2, 21, 63])
def test_key_and_input_edges(torch_dev, k):
    rng = random.Random(k)
    rnd = lambda n, alpha=b"ACGT": bytes(rng.choice(alpha) for _ in range(n))
    seqs = [b"A" * (k + 20), b"T" * (k + 20), b"A" * (k - 1), b"", b"C" * k, b"G"]
    seqs.append(rnd(3 * k) + b"N" + rnd(2 * k))
    seqs.append(rnd(2 * k) + b"a" + rnd(k) + b"\0" + rnd(k + 1))
    seqs.append(rnd(4 * k, b"ACGTacgtN"))
    seqs.append(rnd(5 * k + 3))
    seqs.append(_rc(seqs[-1]))
    seqs.append(b"")
    want = oracle(seqs, k)
    for bits in (64, 1 << 12):
        got, f = run_filtered(torch_dev, seqs, k, bits)
        s = check_filtered(got, f, want)
        assert s["n_skipped"] == want["stats"]["n_skipped"] > 0


def test_saturation(torch_dev):
    seqs = [b"A" * 1000] * 20 + [b"T" * 1000] * 20
    (prof, h, st), f = run_filtered(torch_dev, seqs, K, 1 << 10)
    assert all(len(p) == 961 and (p == 32767).all() for p in prof)
    low, high, il, ih, hist = h
    assert (low, high, il, ih) == (1, 32767, 0, 38440)
    assert hist[32766] == 1 and hist.sum() == 1
    assert st["n_kmers"] == 38440 and st["n_distinct"] == 1
    assert f["n_table_keys"] == 1 and f["n_outside"] == 0 and f["n_false"] == 0
    check((prof, h, st), O.run(seqs, K))


def test_protocol(torch_dev):
    """Each refused call is CP_EINVAL and leaves the table as it was: it is still usable and exact afterwards."""
    from classpro_amd.api import KmerCounts
    from classpro_amd._lib import ClassProError
    rng = random.Random(9)
    a, b = (bytes(rng.choice(b"ACGT") for _ in range(500)) * 2 for _ in range(2))
    k = 21
    want = oracle([a, b], k)

    def refused(fn, *words):
        with pytest.raises(ClassProError) as e:
            fn()
        assert e.value.code == -1 and all(w in str(e.value) for w in words), str(e.value)

    U = KmerCounts(k)                                      # mark on a table without a filter
    refused(lambda: U.mark_tensors(*flat(torch_dev, [a])), "no filter")
    U.add_tensors(*flat(torch_dev, [a, b]))
    check((split(U.profiles(flat(torch_dev, [a, b])), [a, b], k), U.hist(), U.stats()), want)
    U.close()

    T = KmerCounts(k, filter_bits=1 << 12)
    T.mark_tensors(*flat(torch_dev, [a]))
    T.mark_tensors(*flat(torch_dev, [b]))
    n = 2 * (1000 - k + 1)
    refused(T.stats, "%d k-mers were marked" % n, " 0 added")           # marked, nothing added yet
    refused(T.hist, "%d k-mers were marked" % n, " 0 added")
    assert T.filter_stats()["n_marked"] == n                            # legal at any time
    T.add_tensors(*flat(torch_dev, [a]))
    refused(T.stats, "%d k-mers were marked" % n, " %d added" % (n // 2))
    refused(lambda: T.mark_tensors(*flat(torch_dev, [b])), "before the first add")
    refused(lambda: T.rel_labels(flat(torch_dev, [a])), "filtered")
    T.add_tensors(*flat(torch_dev, [b]))
    got = (split(T.profiles(flat(torch_dev, [a, b])), [a, b], k), T.hist(), T.stats())
    check_filtered(got, T.filter_stats(), want)
    refused(lambda: T.rel_labels(flat(torch_dev, [a])), "filtered")
    refused(lambda: T.mark_tensors(*flat(torch_dev, [a])), "before the first add")
    got = (split(T.profiles(flat(torch_dev, [a, b])), [a, b], k), T.hist(), T.stats())
    check_filtered(got, T.filter_stats(), want)
    c = rng.choice(b"ACGT")                                # a batch that was never marked or added reads 1: no error
    p = T.profiles(flat(torch_dev, [bytes([c]) * 10 + a[:30]])).cpu().numpy()
    assert p.min() >= 1
    T.stats()
    T.close()


def test_scale_against_torch_oracle(torch_dev):
    """200 Mbases of DeviceSynth at K = 31, marked and added in two batches behind 2^30 filter bits: profiles, histogram
    and statistics against canonical keys packed into int64 and torch.unique on the device; at most half the slots of an
    unfiltered table built beside it."""
    torch = torch_dev
    from classpro_amd.synth_dev import DeviceSynth
    from classpro_amd.api import KmerCounts
    k = 31
    ds = DeviceSynth(genome_len=5_000_000, cov=40, read_len=20000, K=K, seed=3)
    rd = ds.reads(0, ds.n_reads)
    seq, seq_off, total = rd["seq"], rd["seq_off"], rd["total_bases"]
    del rd
    half = ds.n_reads // 2
    cut = int(seq_off[half].item())
    parts = ((seq[:cut], seq_off[:half + 1]), (seq[cut:], seq_off[half:] - cut))
    T = KmerCounts(k, filter_bits=1 << 30)
    for p in parts:
        T.mark_tensors(*p)
    for p in parts:
        T.add_tensors(*p)
    got = T.profiles((seq, seq_off)).view(torch.int16).long()
    low, high, il, ih, hist = T.hist()
    s, f = T.stats(), T.filter_stats()
    T.close()
    U = KmerCounts(k)
    for p in parts:
        U.add_tensors(*p)
    u = U.stats()
    U.close()
    print("filtered %r %r\nunfiltered %r" % (s, f, u))
    assert 2 * s["slots"] <= u["slots"] and s["slots"] >= 2 * f["n_table_keys"]
    code = torch.full((256,), -1, dtype=torch.int64, device=seq.device)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    base = code[seq[:total].long()]
    assert bool((base >= 0).all())
    pos = torch.arange(total, device=seq.device)
    rid = torch.searchsorted(seq_off, pos, right=True) - 1
    ends = pos[pos >= seq_off[rid] + k - 1]
    del pos, rid
    fw = torch.zeros_like(ends)
    rc = torch.zeros_like(ends)
    for j in range(k):
        bj = base[ends - (k - 1) + j]
        fw = fw * 4 + bj
        rc = rc + ((3 - bj) << (2 * j))
    key = torch.minimum(fw, rc)
    del fw, rc, base
    _, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    want = cnt.clamp(max=32767)[inv]
    assert got.numel() == want.numel() and bool((got == want).all())
    wh = torch.bincount(cnt.clamp(max=32767), minlength=32768)[1:].cpu().numpy()
    assert np.array_equal(hist, wh) and il == wh[0]
    assert ih == int(cnt[cnt >= 32767].sum().item())
    assert s["n_distinct"] == cnt.numel() == u["n_distinct"] and s["n_kmers"] == ends.numel() == u["n_kmers"]
    assert s["n_skipped"] == 0
    twice = int((cnt >= 2).sum().item())
    assert f["n_table_keys"] - f["n_false"] == twice and f["n_table_keys"] + f["n_outside"] == cnt.numel()


OUTPUTS = ["reads.hist", "reads.prof"]


def _outputs(d, parts):
    names = OUTPUTS + [".reads.%s.%d" % (w, p + 1) for w in ("pidx", "prof") for p in range(parts)]
    return {n: open(os.path.join(d, n), "rb").read() for n in names}


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("kind", ["fasta", "fasta.gz", "fastq"])
def test_command(small, tmp_path, kind, threads):
    ds, seqs, want = small
    out = {}
    for how, opt in (("plain", []), ("filtered", ["-f16"])):
        d = os.path.join(str(tmp_path), how)
        os.mkdir(d)
        src = _write_source(d, kind, ds["names"], seqs)
        r = subprocess.run([KPROF, "-v", "-T%d" % threads] + opt + [src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "" and ("keys kept outside" in r.stderr) == bool(opt)
        assert "%d distinct" % DISTINCT in r.stderr
        out[how] = _outputs(d, threads)
        assert sorted(n for n in os.listdir(d) if not n.startswith("reads.fa")) == sorted(out[how])
    assert out["plain"] == out["filtered"]
    assert all(len(v) > 0 for v in out["plain"].values())


def test_classpro_on_filtered_files(small, tmp_path):
    """ClassPro on what `kprof -f16` wrote and on what `kprof` wrote: the same .class, byte for byte."""
    ds, seqs, _ = small
    out = []
    for how, opt in (("plain", []), ("filtered", ["-f16"])):
        d = os.path.join(str(tmp_path), how)
        os.mkdir(d)
        src = _write_source(d, "fasta", ds["names"], seqs)
        r = subprocess.run([KPROF, "-T4"] + opt + [src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([os.path.join(TOOLS, "ClassPro"), "-T4", "-P" + d, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out.append(open(os.path.join(d, "reads.class"), "rb").read())
    assert len(out[0]) > 2 * sum(len(s) for s in seqs) and out[0] == out[1]

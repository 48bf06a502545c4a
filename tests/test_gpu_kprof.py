"""The k-mer count table (cp_kmer_counts_*, KmerCounts, kprof) on a real MI355X (`-m gpu`), against the brute-force
restatement in tests/kprof_oracle.py: exact profiles, histogram and statistics, independence of order and batching,
growth, key and input edges, saturation, a 200-Mbase set against a torch-side oracle, the command line, and ClassPro
run on what the command wrote.  Everything is integers and bytes: the tolerance is zero."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import kprof_oracle as O
from conftest import ROOT

pytestmark = pytest.mark.gpu
K = 40
TOOLS = os.path.join(ROOT, "classpro_amd")
KPROF = os.path.join(TOOLS, "kprof")


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


def flat(torch, seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    x = b"".join(seqs)
    dev = torch.device("cuda:0")
    seq = torch.from_numpy(np.frombuffer(x, np.uint8).copy() if x else np.zeros(1, np.uint8)).to(dev)
    return seq, torch.from_numpy(off).to(dev)


def split(prof, seqs, k):
    """A flat profile (device tensor) as per-read numpy arrays."""
    p = prof.cpu().numpy()
    out, o = [], 0
    for s in seqs:
        n = max(len(s) - (k - 1), 0)
        out.append(p[o:o + n])
        o += n
    assert o == len(p)
    return out


def run_table(torch, seqs, k, batches=None, **kw):
    """Adds `batches` (lists of reads; default: all in one), then profiles all reads in one batch."""
    from classpro_amd.api import KmerCounts
    T = KmerCounts(k, **kw)
    for b in batches or [seqs]:
        T.add_tensors(*flat(torch, b))
    prof = split(T.profiles(flat(torch, seqs)), seqs, k)
    h, s = T.hist(), T.stats()
    T.close()
    return prof, h, s


def same_profiles(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def check(got, want):
    prof, h, s = got
    assert same_profiles(prof, want["profiles"])
    wl, wh, wil, wih, whist = want["hist"]
    assert h[:4] == (wl, wh, wil, wih) and np.array_equal(h[4], whist)
    for k, v in want["stats"].items():
        assert s[k] == v, (k, s[k], v)
    return s


def test_library_matches_oracle(torch_dev, small):
    from classpro_amd.api import Batch, KmerCounts
    _, seqs, want = small
    s = check(run_table(torch_dev, seqs, K), want)
    assert s["n_distinct"] > 1000 and s["n_skipped"] == 0 and s["slots"] >= 2 * s["n_distinct"]
    total = sum(len(x) for x in seqs)                  # a first batch past the default table: sized for it, no growth
    assert 2 * total > 1 << 20 and s["growths"] == 0 and s["slots"] == 1 << (2 * total - 1).bit_length()
    b = Batch.from_seqs(seqs, K)                       # the Batch form fills b.prof in place
    T = KmerCounts(K)
    T.add(b)
    out = T.profiles(b)
    assert out.dtype == torch_dev.uint16 and out.data_ptr() == b.prof.data_ptr() and b.total_kmers == out.numel()
    assert same_profiles(split(out, seqs, K), want["profiles"])
    T.close()


def test_order_and_batching(torch_dev, small):
    _, seqs, want = small
    check(run_table(torch_dev, seqs, K, batches=[[s] for s in seqs]), want)
    check(run_table(torch_dev, seqs, K, batches=[seqs[:5], seqs[5:40], seqs[40:]]), want)
    order = list(range(len(seqs)))
    random.Random(7).shuffle(order)
    sh = [seqs[i] for i in order]
    prof, h, s = run_table(torch_dev, sh, K)
    back = [None] * len(seqs)
    for pos, i in enumerate(order):
        back[i] = prof[pos]
    check((back, h, s), want)


def test_growth(torch_dev, small):
    _, seqs, want = small
    s = check(run_table(torch_dev, seqs, K, initial_slots=64), want)
    assert s["growths"] > 0 and s["slots"] >= 2 * s["n_distinct"]


def test_growth_across_batches(torch_dev):
    """Three batches of about 39 200 new keys each into 64 slots: the first grows the table to 2^17 slots inside its add,
    the second passes half of that, so its growth rehashes a table that already holds the counts of an earlier batch."""
    rng = np.random.default_rng(23)
    seqs = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 2000)]) for _ in range(60)]
    batches = [seqs[:20], seqs[20:40], seqs[40:]]
    want = O.run(seqs, K)
    s_small = check(run_table(torch_dev, seqs, K, batches=batches, initial_slots=64), want)
    s_big = check(run_table(torch_dev, seqs, K, batches=batches, initial_slots=1 << 20), want)
    assert s_small["growths"] >= 2 and s_big["growths"] == 0 and s_big["slots"] == 1 << 20
    drop = ("slots", "bytes", "growths")
    assert {k: v for k, v in s_small.items() if k not in drop} == {k: v for k, v in s_big.items() if k not in drop}


def _rc(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


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
    want = O.run(seqs, k)
    s = check(run_table(torch_dev, seqs, k), want)
    assert s["n_skipped"] == want["stats"]["n_skipped"] > 0
    assert len(want["profiles"][2]) == len(want["profiles"][3]) == 0


def test_reverse_complement_read_mirrors_and_doubles(torch_dev):
    rng = random.Random(3)
    s = bytes(rng.choice(b"ACGT") for _ in range(3000))
    one, _, _ = run_table(torch_dev, [s], K)
    two, h, st = run_table(torch_dev, [s, _rc(s)], K)
    check((two, h, st), O.run([s, _rc(s)], K))
    assert np.array_equal(two[0], two[1][::-1])
    assert np.array_equal(two[0], 2 * one[0])


def test_palindrome_counts_once_per_occurrence(torch_dev):
    s = b"ACGT" * 10
    assert _rc(s) == s
    prof, h, st = run_table(torch_dev, [s, s + b"ACG"], K)
    check((prof, h, st), O.run([s, s + b"ACG"], K))
    assert prof[0].tolist() == [2] and prof[1][0] == 2 and st["n_kmers"] == 5


def test_saturation(torch_dev):
    seqs = [b"A" * 1000] * 20 + [b"T" * 1000] * 20
    prof, h, st = run_table(torch_dev, seqs, K)
    assert all(len(p) == 961 and (p == 32767).all() for p in prof)
    low, high, il, ih, hist = h
    assert (low, high, il, ih) == (1, 32767, 0, 38440)
    assert hist[32766] == 1 and hist.sum() == 1
    assert st["n_kmers"] == 38440 and st["n_distinct"] == 1
    check((prof, h, st), O.run(seqs, K))


def test_profiling_a_batch_that_was_never_added(torch_dev):
    from classpro_amd.api import KmerCounts
    from classpro_amd._lib import ClassProError
    rng = random.Random(9)
    a, b = (bytes(rng.choice(b"ACGT") for _ in range(500)) for _ in range(2))
    T = KmerCounts(21)
    T.add_tensors(*flat(torch_dev, [a]))
    p = T.profiles(flat(torch_dev, [b])).cpu().numpy()
    assert (p == 0).all()
    with pytest.raises(ClassProError) as e:
        T.stats()
    assert e.value.code == -1
    s = T.stats()                                         # reported once; the table is as it was
    assert s["n_kmers"] == 480
    T.add_tensors(*flat(torch_dev, [b]))
    want = O.run([a, b], 21)
    prof = split(T.profiles(flat(torch_dev, [a, b])), [a, b], 21)
    check((prof, T.hist(), T.stats()), want)
    T.close()
    for k in (1, 64):
        with pytest.raises(ClassProError):
            KmerCounts(k)


def test_scale_against_torch_oracle(torch_dev):
    """200 Mbases of DeviceSynth at K = 31: profiles, histogram and statistics against canonical keys packed into int64
    and torch.unique on the device."""
    torch = torch_dev
    from classpro_amd.synth_dev import DeviceSynth
    from classpro_amd.api import KmerCounts
    k = 31
    ds = DeviceSynth(genome_len=5_000_000, cov=40, read_len=20000, K=K, seed=3)
    rd = ds.reads(0, ds.n_reads)
    seq, seq_off, total = rd["seq"], rd["seq_off"], rd["total_bases"]
    del rd
    T = KmerCounts(k)
    half = ds.n_reads // 2                                               # two batches, one profile pass
    cut = int(seq_off[half].item())
    T.add_tensors(seq[:cut], seq_off[:half + 1])
    T.add_tensors(seq[cut:], seq_off[half:] - cut)
    got = T.profiles((seq, seq_off)).view(torch.int16).long()
    low, high, il, ih, hist = T.hist()
    s = T.stats()
    T.close()
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
    assert s["n_distinct"] == cnt.numel() and s["n_kmers"] == ends.numel() and s["n_skipped"] == 0


def _write_source(d, kind, names, seqs):
    if kind == "fastq":
        path = os.path.join(d, "reads.fastq")
        with open(path, "wb") as f:
            for n, s in zip(names, seqs):
                f.write(b"@" + n.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
        return path
    path = os.path.join(d, "reads.fasta.gz" if kind == "fasta.gz" else "reads.fasta")
    with (gzip.open if kind == "fasta.gz" else open)(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + s + b"\n")
    return path


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("kind", ["fasta", "fasta.gz", "fastq"])
def test_command(small, tmp_path, kind, threads):
    import struct
    from classpro_amd import fastk
    ds, seqs, want = small
    d = str(tmp_path)
    src = _write_source(d, kind, ds["names"], seqs)
    r = subprocess.run([KPROF, "-v", "-T%d" % threads, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "distinct" in r.stderr and r.stdout == ""
    kk, low, high, il, ih, h = fastk.read_fastk_hist(os.path.join(d, "reads.hist"))
    wl, wh, wil, wih, whist = want["hist"]
    assert (kk, low, high, il, ih) == (K, wl, wh, wil, wih) and np.array_equal(h, whist)
    kk, codes = fastk.read_fastk_codes(d, "reads")
    assert kk == K and len(codes) == len(seqs)
    assert same_profiles([fastk.decode_profile(c) for c in codes], want["profiles"])
    assert codes == [fastk.encode_profile(p) for p in want["profiles"]]
    with open(os.path.join(d, "reads.prof"), "rb") as f:
        assert struct.unpack("<ii", f.read(8)) == (K, threads)
    first = 0
    for p in range(threads):
        with open(os.path.join(d, ".reads.pidx.%d" % (p + 1)), "rb") as f:
            pk, = struct.unpack("<i", f.read(4))
            pf, pn = struct.unpack("<qq", f.read(16))
        assert pk == K and pf == first and pn > 0
        first += pn
    assert first == len(seqs)


def test_command_files_through_the_reference_readers(small, tmp_path):
    """The files kprof wrote, read by the reference's own Open_Profiles / Fetch_Profile and process_global_hist."""
    from classpro_amd.api import hist_covs
    from oracle import oracle
    if not oracle.ref_available():
        pytest.skip("the reference's own readers (oracle/_ref) are not built here")
    ds, seqs, want = small
    d = str(tmp_path)
    src = _write_source(d, "fasta", ds["names"], seqs)
    r = subprocess.run([KPROF, "-T4", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    wl, wh, wil, wih, whist = want["hist"]
    R = oracle.Ref()
    rk, rprof = R.fetch_profiles(os.path.join(d, "reads"))
    assert rk == K and same_profiles(rprof, want["profiles"])
    assert R.hist_covs(os.path.join(d, "reads")) == hist_covs(whist, wl, wh, wil, wih, 0)


def test_command_options(small, tmp_path):
    """-k and -N: another K, another root; a read shorter than K and one with an N keep their place."""
    from classpro_amd import fastk
    ds, seqs, _ = small
    d = str(tmp_path)
    seqs = [seqs[0], b"ACGTAC", seqs[1][:300] + b"N" + seqs[1][300:600], b""] + seqs[2:6]
    src = _write_source(d, "fasta", ["r%d" % i for i in range(len(seqs))], seqs)
    root = os.path.join(d, "sub", "other")
    os.mkdir(os.path.join(d, "sub"))
    r = subprocess.run([KPROF, "-k21", "-T3", "-N" + root, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = O.run(seqs, 21)
    assert want["stats"]["n_skipped"] == 21 and "21" in r.stderr and "skipped" in r.stderr
    kk, codes = fastk.read_fastk_codes(os.path.join(d, "sub"), "other")
    assert kk == 21 and same_profiles([fastk.decode_profile(c) for c in codes], want["profiles"])
    got = fastk.read_fastk_hist(root + ".hist")
    assert got[:5] == (21,) + want["hist"][:4] and np.array_equal(got[5], want["hist"][4])


def test_classpro_on_kprof_files(small, tmp_path):
    """ClassPro on what kprof wrote, and on fastk.write_fastk of the oracle's counts: the same .class, byte for byte."""
    from classpro_amd import fastk
    ds, seqs, want = small
    out = []
    for how in ("kprof", "oracle"):
        d = os.path.join(str(tmp_path), how)
        os.mkdir(d)
        src = _write_source(d, "fasta", ds["names"], seqs)
        if how == "kprof":
            r = subprocess.run([KPROF, "-T4", src], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
        else:
            fastk.write_fastk(d, "reads", K, want["profiles"], want["hist"])
        r = subprocess.run([os.path.join(TOOLS, "ClassPro"), "-T4", "-P" + d, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out.append(open(os.path.join(d, "reads.class"), "rb").read())
    assert len(out[0]) > 2 * sum(len(s) for s in seqs) and out[0] == out[1]

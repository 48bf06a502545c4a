"""The sorted snapshot of a label table, one consensus class per call, and its per-class histogram (cp_kmer_table_sort,
cp_kmer_table_class_hist, KmerTable.sorted / class_hist) on a real MI355X (`-m gpu`), against the brute-force
restatement in tests/cnstab_oracle.py: keys, exact totals, .ktab records and prefix index for every class, cutoff and
agreement, every prefix width, sizes around the sort's tile inside one bucket that holds all four classes, the first
and the last bucket, the count clamp, forward tables, the two identities with the count table, snapshots against later
adds, growth and batching, and bad arguments.  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import cns_oracle as CO
import cnstab_oracle as CT
import kprof_oracle as O
import ktab_oracle as KO
from test_ktab_host import KS

pytestmark = pytest.mark.gpu
EINVAL = -1
CLASSES = (None, "E", "H", "D", "R")


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def flat(torch, recs):
    seq = b"".join(r[1] for r in recs)
    lab = b"".join(r[2] for r in recs)
    off = np.zeros(len(recs) + 1, np.int64)
    np.cumsum([len(r[1]) for r in recs], out=off[1:])
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.frombuffer(x, np.uint8).copy() if x else np.zeros(1, np.uint8)).to(dev)
    return t(seq), torch.from_numpy(off).to(dev), t(lab)


def table_of(torch, recs, k, canonical=True, batches=None, **kw):
    from classpro_amd.api import KmerTable
    T = KmerTable(k, canonical=canonical, **kw)
    for b in batches or [recs]:
        T.add_tensors(*flat(torch, b))
    return T


def one_kmer_records(spec, k):
    """One k-mer per read and one label per read: spec is [(k-mer, [E, H, D, R] counts)]."""
    return [(b"r", km, b"N" * (k - 1) + CT.LABELS[l].encode()) for km, c in spec for l in range(4) for _ in range(c[l])]


def check(torch, s, ents, k, ktab=True, whole_index=False):
    """A snapshot against the oracle's entries: keys, totals, records, and the index against a prefix count made on the
    device from the oracle's prefixes.  Returns the record bytes (and the index bytes with whole_index)."""
    hi, lo, cnt = KO.hi_lo_cnt(ents)
    assert len(s) == len(ents)
    assert s.hi.cpu().tolist() == hi and s.lo.cpu().tolist() == lo and s.counts.cpu().tolist() == cnt
    if not ktab:
        return None
    rec, idx = s.ktab()
    recb = rec.cpu().numpy().tobytes()
    assert recb == KO.records_fast(ents, k)
    per = torch.zeros(idx.numel(), dtype=torch.int64, device=idx.device)
    if ents:
        p = torch.tensor([KO.prefix(x, k) for x, _ in ents], dtype=torch.int64, device=idx.device)
        per = torch.bincount(p, minlength=idx.numel())
    assert torch.equal(idx, per.cumsum(0))
    return (recb, idx.cpu().numpy().tobytes()) if whole_index else recb


TIES = [[1, 1, 0, 0], [0, 2, 2, 0], [0, 0, 3, 3], [2, 2, 2, 2], [2, 1, 0, 0], [3, 0, 0, 3], [1, 0, 1, 0]]


def mixed_spec(k, seed=3, n=300):
    """A few hundred distinct k-mers with 0 to 3 occurrences per label, the tie shapes among them."""
    rng = random.Random(seed * 1000 + k)
    kms = set()
    while len(kms) < min(n, 4 ** k // 3):
        kms.add(bytes(rng.choice(b"ACGT") for _ in range(k)))
    spec = []
    for i, km in enumerate(sorted(kms)):
        c = TIES[i] if i < len(TIES) else [rng.randint(0, 3) for _ in range(4)]
        if not any(c):
            c[rng.randrange(4)] = 1
        spec.append((km, c))
    rng.shuffle(spec)
    return spec


@pytest.mark.parametrize("k", [3] + KS)
def test_against_oracle_every_class_and_filter(torch_dev, k):
    recs = one_kmer_records(mixed_spec(k), k)
    random.Random(k).shuffle(recs)
    t, skipped = CO.table(recs, k, True)
    assert skipped == 0
    top = max(sum(c) for c in t.values())
    assert top >= 6 and {CT.LABELS[CO.consensus_label(c)] for c in t.values()} == set("EHDR")
    T = table_of(torch_dev, recs, k)
    empty = 0
    for label in CLASSES:
        for mt in (1, 2, 3, top + 1):
            for pct in (0, 50, 67, 100):
                ents = CT.select(t, label, mt, pct)
                empty += not ents
                assert (mt == top + 1) <= (not ents)
                s = T.sorted(label, mt, pct)
                check(torch_dev, s, ents, k, ktab=k >= 5)
                s.close()
    assert empty >= 20
    a = [len(CT.select(t, None, 1, pct)) for pct in (100, 67, 50, 0)]
    assert a[0] <= a[1] < a[2] < a[3] == len(t) and (k < 5 or a[0] < a[1])          # every agreement step drops keys
    T.close()


def bucket_kmers(head, n, seed):
    """n distinct 40-mers behind `head` (12 bases), the forward strand canonical: they end in C."""
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add(head + bytes(rng.choice(b"ACGT") for _ in range(27)) + b"C")
    return sorted(out)


def test_tile_edges_inside_one_bucket(torch_dev):
    """tile-1 keys of class E, tile of H, tile+1 of D and 3*tile+5 of R share the bucket behind A x 12: every class
    filter meets the on-chip path, its edge or the oversize path among keys of the other classes."""
    from classpro_amd.api import ktab_tile
    tile = ktab_tile()
    assert tile >= 64
    k = 40
    sizes = [tile - 1, tile, tile + 1, 3 * tile + 5]
    kms = bucket_kmers(b"A" * 12, sum(sizes), 1)
    random.Random(2).shuffle(kms)
    rng = random.Random(3)
    spec, at = [], 0
    for l, n in enumerate(sizes):
        for km in kms[at:at + n]:
            c = [0, 0, 0, 0]
            c[l] = rng.randint(1, 2)
            if rng.random() < 0.3:
                c[(l + 1 + rng.randrange(3)) % 4] = c[l] - 1           # a minority label that never ties
            spec.append((km, c))
        at += n
    spec += [(km, [rng.randint(0, 2) for _ in range(3)] + [1]) for km in bucket_kmers(b"A" * 11 + b"C", 50, 4)]
    recs = one_kmer_records(spec, k)
    rng.shuffle(recs)
    t, _ = CO.table(recs, k, True)
    T = table_of(torch_dev, recs, k)
    first = lambda ents: sum(1 for x, _ in ents if KO.prefix(x, k) == 0)
    for label, n in zip(CLASSES, [sum(sizes)] + sizes):
        ents = CT.select(t, label)
        assert first(ents) == n and len(ents) > n                      # the second bucket holds every class too
        s = T.sorted(label)
        check(torch_dev, s, ents, k)
        s.close()
    s = T.sorted("R", 1, 100)                                          # a filter that thins the oversize bucket
    ents = CT.select(t, "R", 1, 100)
    assert tile < first(ents) < 3 * tile
    check(torch_dev, s, ents, k)
    s.close()
    T.close()


def whole_read(name, s, label, k):
    return (name, s, b"N" * min(len(s), k - 1) + label * max(len(s) - k + 1, 0))


def rnd_reads(seed, n, length):
    rng = np.random.default_rng(seed)
    return [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]) for _ in range(n)]


def test_first_and_last_bucket(torch_dev):
    k = 40
    last = b"T" * 12 + b"ACGTACGTACGTACGA" + b"A" * 12       # its reverse complement begins T x 12 too and is larger
    assert O.canon(last) == last
    seqs = [b"A" * k, last] + rnd_reads(8, 3, 200)
    recs = [whole_read(b"r%d" % i, s, l, k) for i, (s, l) in enumerate(zip(seqs, [b"E", b"R", b"H", b"D", b"H"]))]
    t, _ = CO.table(recs, k, True)
    T = table_of(torch_dev, recs, k)
    for label in CLASSES:
        s = T.sorted(label)
        ents = CT.select(t, label)
        assert ents
        check(torch_dev, s, ents, k)
        if label == "E":
            assert len(s) == 1 and (int(s.hi[0]), int(s.lo[0])) == (0, 0)
        if label == "R":
            assert len(s) == 1 and ((int(s.hi[0]) << 63) | int(s.lo[0])) == KO.key_of(last)
            assert int(s.ktab()[1][-2]) == 0 and KO.prefix(KO.key_of(last), k) == 0xFFFFFF
        s.close()
    T.close()


@pytest.fixture(scope="module")
def clamped(torch_dev):
    """A x 1000 and T x 1000 reads, ten of each label: one key with 9610 per label and a total of 38 440."""
    k = 40
    recs = [whole_read(b"a", b"A" * 1000, l, k) for l in (b"E", b"H", b"D", b"R") for _ in range(5)]
    recs += [whole_read(b"t", b"T" * 1000, l, k) for l in (b"E", b"H", b"D", b"R") for _ in range(5)]
    recs += [whole_read(b"x", b"ACGT" * 20, b"H", k), whole_read(b"y", b"ACGT" * 20, b"E", k)]
    t, _ = CO.table(recs, k, True)
    assert t[0] == [9610] * 4
    T = table_of(torch_dev, recs, k)
    yield T, t, k
    T.close()


def test_count_clamp(torch_dev, clamped):
    T, t, k = clamped
    for label, mt in ((None, 1), ("R", 1), ("R", 32767), (None, 32767)):
        s = T.sorted(label, mt)
        ents = CT.select(t, label, mt)
        assert ents[0] == (0, 38440)
        rec = check(torch_dev, s, ents, k)
        assert int(s.counts[0]) == 38440 and rec[7:9] == b"\xff\x7f"      # 7 suffix bytes, then the clamped count
        assert len(s) == (1 if mt > 1 or label else len(t))
        s.close()
    s = T.sorted("R", 1, 26)                                              # 25 % agreement and not a point more
    assert len(s) == 0
    s.close()


def test_class_hist(torch_dev, clamped):
    T, t, k = clamped
    h, il, ih = T.class_hist()
    wh, wil, wih = CT.class_hist(t)
    assert np.array_equal(h, wh) and np.array_equal(il, wil) and np.array_equal(ih, wih)
    assert h[3, 32766] == 1 and ih.tolist() == [0, 0, 0, 38440] and h.dtype == np.int64 and h.shape == (4, 32767)
    recs = one_kmer_records(mixed_spec(21, 9) + [(b"ACGT" * 5 + b"A", [300, 0, 1, 0]), (b"C" * 21, [0, 0, 0, 257])], 21)
    t2, _ = CO.table(recs, 21, True)
    T2 = table_of(torch_dev, recs, 21)
    h, il, ih = T2.class_hist()
    wh, wil, wih = CT.class_hist(t2)
    assert np.array_equal(h, wh) and np.array_equal(il, wil) and np.array_equal(ih, wih)
    assert h[0, 300] == 1 and h[3, 256] == 1 and il.sum() > 0 and all(h[l].sum() > 0 for l in range(4))
    T2.close()


def _labels(rng, n, k):
    return b"N" * min(n, k - 1) + bytes(rng.choice(b"EHDR") for _ in range(max(0, n - k + 1)))


def labelled_reads(k, seed):
    """Reads with a label per position, repeats (totals above 1, mixed labels), an N, a short read, an empty one."""
    rng = random.Random(seed * 100 + k)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    a, b, c = rnd(300 + k), rnd(900), rnd(1500)
    rc = lambda s: s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
    seqs = [a, b, c, b[100:500], rc(c[:700]), c[200:600], rnd(200) + b"N" + rnd(2 * k), rnd(k - 1), b"", b"A" * (k + 5),
            b"T" * (k + 2), rc(b)]
    return [(b"r%d" % i, s, _labels(rng, len(s), k)) for i, s in enumerate(seqs)]


@pytest.mark.parametrize("k", [21, 40])
def test_forward_table(torch_dev, k):
    recs = labelled_reads(k, 1)
    t, skipped = CO.table(recs, k, False)
    tc, _ = CO.table(recs, k, True)
    assert skipped > 0 and len(tc) < len(t)
    T = table_of(torch_dev, recs, k, canonical=False)
    for label, mt, pct in [(l, 1, 0) for l in CLASSES] + [(None, 2, 0), ("D", 1, 67), ("R", 2, 50)]:
        s = T.sorted(label, mt, pct)
        check(torch_dev, s, CT.select(t, label, mt, pct), k)
        s.close()
    T.close()


def merged(torch, parts):
    """The entries of several snapshots in key order: two stable sorts, lo and then hi."""
    hi, lo, c = (torch.cat([getattr(p, f) for p in parts]) for f in ("hi", "lo", "counts"))
    o = torch.sort(lo, stable=True)[1]
    hi, lo, c = hi[o], lo[o], c[o]
    o = torch.sort(hi, stable=True)[1]
    return hi[o], lo[o], c[o]


def check_identities(torch, T, Cn, cns_total):
    """The four class snapshots partition the label = -1 snapshot, which is the count table's snapshot; the four class
    histograms sum to the count table's."""
    parts = [T.sorted(l) for l in CT.LABELS]
    every, cnt = T.sorted(), Cn.sorted(1)
    assert sum(len(p) for p in parts) == len(every) == len(cnt) > 0 and all(len(p) > 0 for p in parts)
    assert [int(p.counts.sum()) for p in parts] == cns_total
    hi, lo, c = merged(torch, parts)
    for a, b in ((hi, every.hi), (lo, every.lo), (c, every.counts), (every.hi, cnt.hi), (every.lo, cnt.lo),
                 (every.counts, cnt.counts)):
        assert torch.equal(a, b)
    (r1, i1), (r2, i2) = every.ktab(), cnt.ktab()
    assert torch.equal(r1, r2) and torch.equal(i1, i2)
    ip = [p.ktab(0, 0)[1] for p in parts]
    assert torch.equal(ip[0] + ip[1] + ip[2] + ip[3], i1)
    h, il, ih = T.class_hist()
    low, high, ilow, ihigh, want = Cn.hist()
    assert np.array_equal(h.sum(0), want) and int(il.sum()) == ilow and int(ih.sum()) == ihigh
    assert [int(x.sum()) for x in h] == [len(p) for p in parts]
    for p in parts + [every, cnt]:
        p.close()


def test_identities_on_classifier_labels(torch_dev):
    """The 60 kbp / 30x set labelled by the classifier."""
    from classpro_amd import synth
    from classpro_amd.api import Batch, Classifier, KmerCounts, KmerTable, hist_covs
    k = 40
    ds = synth.make_dataset(genome_len=60000, cov=30, read_len=6000, seed=11)
    low, high, il, ih, h = ds["hist"]
    hc, dc = hist_covs(h, low, high, il, ih, 0)
    clf = Classifier(K=k, read_len=20000, hcov=hc, dcov=dc)
    b = Batch.from_reads(ds["seqs"], ds["profiles"])
    clf.classify(b)
    clf.close()
    T, Cn = KmerTable(k, canonical=True), KmerCounts(k)
    T.add(b)
    Cn.add(b)
    st = T.stats()
    assert st["n_distinct"] == Cn.stats()["n_distinct"] > 50000
    check_identities(torch_dev, T, Cn, st["cns_total"])
    T.close()
    Cn.close()


def test_identities_at_9_mbases(torch_dev):
    """DeviceSynth reads with labels drawn from the position: the table only counts, so they need not mean anything."""
    torch = torch_dev
    from classpro_amd.synth_dev import DeviceSynth
    from classpro_amd.api import KmerCounts, KmerTable
    k = 40
    ds = DeviceSynth(genome_len=3_000_000, cov=3, read_len=20000, K=k, seed=5)
    rd = ds.reads(0, ds.n_reads)
    seq, seq_off, total = rd["seq"], rd["seq_off"], rd["total_bases"]
    pos = torch.arange(total, device=seq.device)
    rid = torch.searchsorted(seq_off, pos, right=True) - 1
    letters = torch.tensor(list(b"EHDR"), dtype=torch.uint8, device=seq.device)
    lab = letters[((pos * 2654435761) >> 13) % 4]
    lab[pos < seq_off[rid] + k - 1] = ord("N")
    T, Cn = KmerTable(k, canonical=True), KmerCounts(k)
    T.add_tensors(seq, seq_off, lab)
    Cn.add_tensors(seq, seq_off)
    st = T.stats()
    assert st["n_distinct"] > 2_000_000 and st["n_kmers"] == Cn.stats()["n_kmers"] and min(st["cns_total"]) > 100_000
    check_identities(torch, T, Cn, st["cns_total"])
    T.close()
    Cn.close()


def test_table_is_only_read_and_snapshots_stay(torch_dev):
    k = 31
    recs = labelled_reads(k, 3)
    more = labelled_reads(k, 4)[:3] + [recs[0]]
    T = table_of(torch_dev, recs, k)
    st0, e0 = T.stats(), T.entries()
    s1 = T.sorted("H")
    s2 = T.sorted("H")
    h0 = T.class_hist()
    st1, e1 = T.stats(), T.entries()
    assert st0 == st1 and all(np.array_equal(x, y) for x, y in zip(e0, e1))
    t, _ = CO.table(recs, k, True)
    old = CT.select(t, "H")
    assert check(torch_dev, s1, old, k) == check(torch_dev, s2, old, k)
    s2.close()
    T.add_tensors(*flat(torch_dev, more))
    t2, _ = CO.table(recs + more, k, True)
    new = CT.select(t2, "H")
    assert new != old
    s3 = T.sorted("H")
    check(torch_dev, s3, new, k)
    check(torch_dev, s1, old, k)                           # the old snapshot did not follow
    assert not all(np.array_equal(x, y) for x, y in zip(h0, T.class_hist()))
    s1.close()
    s3.close()
    T.close()


def test_growth_and_batching(torch_dev):
    k = 40
    rng = random.Random(23)
    seqs = rnd_reads(23, 42, 1500)
    seqs += [s[100:900] for s in seqs[:10]]
    recs = [(b"g%d" % i, s, _labels(rng, len(s), k)) for i, s in enumerate(seqs)]
    t, _ = CO.table(recs, k, True)
    got = []
    for nb in (1, 3, 7):
        order = list(range(len(recs)))
        random.Random(nb).shuffle(order)
        sh = [recs[i] for i in order]
        batches = [sh[i * len(sh) // nb:(i + 1) * len(sh) // nb] for i in range(nb)]
        T = table_of(torch_dev, sh, k, batches=batches, initial_slots=64)
        assert T.stats()["growths"] >= 1
        out = []
        for label in CLASSES:
            s = T.sorted(label)
            out.append(check(torch_dev, s, CT.select(t, label), k, whole_index=True))
            s.close()
        got.append(out)
        T.close()
    assert got[0] == got[1] == got[2]


def test_bad_arguments(torch_dev):
    from classpro_amd._lib import ClassProError, lib
    k = 21
    recs = labelled_reads(k, 8)
    t, _ = CO.table(recs, k, True)
    T = table_of(torch_dev, recs, k)
    st0 = T.stats()
    L = lib()
    for label, mt, pct in ((-2, 1, 0), (4, 1, 0), (0, 0, 0), (0, 32768, 0), (0, 1, -1), (0, 1, 101), (-1, -5, 0)):
        s = C.c_void_p(1)
        assert L.cp_kmer_table_sort(T.t, label, mt, pct, None, C.byref(s)) == EINVAL, (label, mt, pct)
        assert s.value is None and b"cp_kmer_table_sort" in L.cp_last_error()
    s = C.c_void_p()
    assert L.cp_kmer_table_sort(None, 0, 1, 0, None, C.byref(s)) == EINVAL
    assert L.cp_kmer_table_sort(T.t, 0, 1, 0, None, None) == EINVAL
    h = np.zeros((4, 32767), np.int64)
    assert L.cp_kmer_table_class_hist(T.t, h.ctypes.data, None, None) == EINVAL
    for mt, pct in ((0, 0), (32768, 0), (1, -1), (1, 101)):
        with pytest.raises(ClassProError) as e:
            T.sorted("H", mt, pct)
        assert e.value.code == EINVAL
    for bad in ("X", "EH", 1, ""):
        with pytest.raises(ValueError):
            T.sorted(bad)
    assert T.stats() == st0                                # the table is still good
    s = T.sorted("D", 32767, 100)
    assert len(s) == 0 and s.hi.numel() == 0
    s.close()
    s = T.sorted("D")
    check(torch_dev, s, CT.select(t, "D"), k)
    s.close()
    T.close()
    T = table_of(torch_dev, one_kmer_records(mixed_spec(4), 4), 4)           # K < 5: a snapshot, but no .ktab
    s = T.sorted("R")
    assert len(s) > 0
    with pytest.raises(ClassProError) as e:
        s.ktab()
    assert e.value.code == EINVAL
    s.close()
    T.close()

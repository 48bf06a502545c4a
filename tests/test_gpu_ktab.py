"""The sorted snapshot of a count table (cp_kmer_counts_sort, cp_kmer_sorted_*, KmerCounts.sorted) on a real MI355X
(`-m gpu`), against the brute-force restatement in tests/ktab_oracle.py: keys, exact counts, .ktab records and prefix
index for every prefix width, dense buckets, sizes around the sort's tile and past it, the first and the last bucket,
the count clamp, ranges, snapshots against later adds, growth and batching, filtered tables, bad arguments, and a few
million keys against torch.  Everything is integers and bytes: the tolerance is zero."""
import random

import numpy as np
import pytest

import kprof_oracle as O
import ktab_oracle as KO
from test_ktab_host import KS

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def flat(torch, seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    x = b"".join(seqs)
    dev = torch.device("cuda:0")
    seq = torch.from_numpy(np.frombuffer(x, np.uint8).copy() if x else np.zeros(1, np.uint8)).to(dev)
    return seq, torch.from_numpy(off).to(dev)


def table_of(torch, seqs, k, batches=None, **kw):
    from classpro_amd.api import KmerCounts
    T = KmerCounts(k, **kw)
    if kw.get("filter_bits"):
        for b in batches or [seqs]:
            T.mark_tensors(*flat(torch, b))
    for b in batches or [seqs]:
        T.add_tensors(*flat(torch, b))
    return T


def check(s, ents, k, ktab=True):
    """A snapshot against the oracle's entries; returns the snapshot's bytes (records, index) for comparisons."""
    hi, lo, cnt = KO.hi_lo_cnt(ents)
    assert len(s) == len(ents)
    assert s.hi.cpu().tolist() == hi and s.lo.cpu().tolist() == lo and s.counts.cpu().tolist() == cnt
    if not ktab:
        return None
    rec, idx = s.ktab()
    rec, idx = rec.cpu().numpy().tobytes(), idx.cpu().numpy()
    assert rec == KO.records_fast(ents, k)
    assert np.array_equal(idx, KO.index(ents, k))
    return rec, idx.tobytes()


def rnd_reads(seed, n, length):
    rng = np.random.default_rng(seed)
    return [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]) for _ in range(n)]


def mixed_reads(k, seed=5):
    """A few hundred bases to a few kilobases; repeats for counts 2 and 3, an N, a read shorter than K, an empty one."""
    rng = random.Random(seed * 100 + k)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    a, b, c = rnd(300 + k), rnd(900), rnd(2500)
    return [a, b, c, b[100:500], c[:700], c[200:600], rnd(200) + b"N" + rnd(2 * k), rnd(k - 1), b"", b"A" * (k + 5),
            b"T" * (k + 2)]


@pytest.mark.parametrize("k", [3] + KS)
def test_against_oracle(torch_dev, k):
    seqs = mixed_reads(k)
    cnt = O.count(seqs, k)[0]
    T = table_of(torch_dev, seqs, k)
    top = max(cnt.values())
    assert top >= 3
    for minc in (1, 2, 3, top + 1):
        ents = KO.entries(cnt, minc)
        assert (len(ents) == 0) == (minc == top + 1)
        s = T.sorted(minc)
        check(s, ents, k, ktab=k >= 5)
        s.close()
    T.close()


def test_dense_buckets(torch_dev):
    """K = 12: two prefix bytes, 65 536 buckets, tens of entries in every one that a canonical k-mer can fall into."""
    k = 12
    seqs = rnd_reads(12, 200, 10000)
    keys, counts = KO.table_np(seqs, k)                    # the numpy form of the oracle: 1.8 M entries
    T = table_of(torch_dev, seqs, k)
    s = T.sorted()
    assert len(s) == len(keys) and bool((s.hi == 0).all())
    assert np.array_equal(s.lo.cpu().numpy().astype(np.uint64), keys) and np.array_equal(s.counts.cpu().numpy(), counts)
    rec, idx = s.ktab()
    assert rec.cpu().numpy().tobytes() == KO.records_np(keys, counts, k)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx, KO.index_np(keys, k))
    per = np.diff(idx, prepend=0)
    # a canonical 12-mer begins with A with probability 7/16 and with C with 5/16: about 50 and 36 entries in each of
    # those buckets; the buckets of the prefixes from T on are nearly empty
    assert per[:1 << 15].min() >= 5 and per.mean() > 20 and per[-1] == 0
    s.close()
    T.close()


def bucket0_reads(n, seed):
    """n distinct reads of one 40-mer each, all behind the prefix A x 12, the forward strand canonical (it ends in C, so
    the reverse complement begins with G)."""
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add(b"A" * 12 + bytes(rng.choice(b"ACGT") for _ in range(27)) + b"C")
    return sorted(out)


@pytest.mark.parametrize("where", ["tile-1", "tile", "tile+1", "3*tile+5"])
def test_tile_edges(torch_dev, where):
    from classpro_amd.api import ktab_tile
    tile = ktab_tile()
    assert tile >= 64
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "3*tile+5": 3 * tile + 5}[where]
    k = 40
    seqs = bucket0_reads(n, n) + rnd_reads(40, 3, 150)
    random.Random(1).shuffle(seqs)
    ents = KO.table(seqs, k)
    T = table_of(torch_dev, seqs, k)
    s = T.sorted()
    _, idx = check(s, ents, k)
    assert np.frombuffer(idx, np.int64)[0] == n            # they all sit in bucket 0
    s.close()
    T.close()


def test_two_oversize_buckets_and_neighbours(torch_dev):
    """Two buckets past the tile with an ordinary bucket between and after them: the tiles skip exactly the two."""
    from classpro_amd.api import ktab_tile
    tile = ktab_tile()
    k = 40
    rng = random.Random(2)
    tail = lambda: bytes(rng.choice(b"ACGT") for _ in range(27)) + b"C"
    seqs = list({b"A" * 12 + tail() for _ in range(tile + 300)})
    seqs += list({b"A" * 11 + b"C" + tail() for _ in range(50)})
    seqs += list({b"A" * 11 + b"G" + tail() for _ in range(2 * tile + 1)})
    seqs += list({b"A" * 11 + b"T" + tail() for _ in range(tile)})
    rng.shuffle(seqs)
    ents = KO.table(seqs, k)
    T = table_of(torch_dev, seqs, k)
    s = T.sorted()
    check(s, ents, k)
    s.close()
    T.close()


def test_first_and_last_bucket(torch_dev):
    k = 40
    last = b"T" * 12 + b"ACGTACGTACGTACGA" + b"A" * 12       # its reverse complement begins T x 12 too and is larger
    assert O.canon(last) == last
    seqs = [b"A" * k, last] + rnd_reads(8, 3, 200)
    ents = KO.table(seqs, k)
    T = table_of(torch_dev, seqs, k)
    s = T.sorted()
    _, idx = check(s, ents, k)
    idx = np.frombuffer(idx, np.int64)
    assert idx[0] == 1 and idx[-1] == len(ents) and idx[-2] == len(ents) - 1
    assert (int(s.hi[0]), int(s.lo[0])) == (0, 0)
    assert ((int(s.hi[-1]) << 63) | int(s.lo[-1])) == KO.key_of(last) and KO.prefix(KO.key_of(last), k) == 0xFFFFFF
    s.close()
    T.close()


def test_one_entry(torch_dev):
    k = 21
    seqs = [b"ACGTTGCATGCATGCAAGTCA"]
    T = table_of(torch_dev, seqs, k)
    s = T.sorted()
    check(s, KO.table(seqs, k), k)
    assert len(s) == 1
    s.close()
    T.close()


def test_a_tensor_keeps_its_snapshot(torch_dev):
    """`T.sorted().hi`: the tensor outlives every name of the SortedKmers and still reads the snapshot's memory."""
    import gc
    k = 31
    seqs = mixed_reads(k, 2)
    ents = KO.table(seqs, k)
    T = table_of(torch_dev, seqs, k)
    lo, cnt = T.sorted().lo, T.sorted().counts[5:]
    gc.collect()
    junk = [T.sorted() for _ in range(3)]                  # allocations that would reuse freed memory
    assert lo.cpu().tolist() == KO.hi_lo_cnt(ents)[1] and cnt.cpu().tolist() == KO.hi_lo_cnt(ents)[2][5:]
    s = junk[0]
    s.close()
    with pytest.raises(ValueError):
        s.hi
    for x in junk:
        x.close()
    T.close()


def test_count_clamp(torch_dev):
    k = 40
    seqs = [b"A" * 1000] * 20 + [b"T" * 1000] * 20 + [b"ACGT" * 20]
    ents = KO.table(seqs, k)
    assert ents[0] == (0, 38440)
    T = table_of(torch_dev, seqs, k)
    s = T.sorted()
    rec, _ = check(s, ents, k)
    assert int(s.counts[0]) == 38440 and rec[7:9] == b"\xff\x7f"          # 7 suffix bytes, then the clamped count
    s.close()
    T.close()


def test_ranges(torch_dev):
    """K = 21: records of 5 bytes, so the ranges begin at every alignment."""
    import ctypes as C
    torch = torch_dev
    k = 21
    seqs = mixed_reads(k, 9)
    ents = KO.table(seqs, k)
    n = len(ents)
    T = table_of(torch, seqs, k)
    s = T.sorted()
    whole, idx = check(s, ents, k)
    for a, b in ((1, 2), (3, 258), (257, 600), (n - 1, n)):
        parts = [s.ktab(0, a), s.ktab(a, b - a), s.ktab(b, None)]
        assert b"".join(r.cpu().numpy().tobytes() for r, _ in parts) == whole
        assert all(i.cpu().numpy().tobytes() == idx for _, i in parts)
    assert b"".join(s.ktab(i, 1)[0].cpu().numpy().tobytes() for i in range(0, 40)) == whole[:200]
    r, i = s.ktab(7, 0)
    assert r.numel() == 0 and i.cpu().numpy().tobytes() == idx
    r, i = s.ktab(n, 0)
    assert r.numel() == 0
    out = torch.full((5 * 10 + 3,), 0xEE, dtype=torch.uint8, device="cuda:0")           # no index, an odd address
    rc = s.L.cp_kmer_sorted_ktab(s.s, 11, 10, C.c_void_p(out.data_ptr() + 3), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and out.cpu().numpy().tobytes() == b"\xee" * 3 + whole[55:105]
    s.close()
    T.close()


def test_table_is_only_read_and_snapshots_stay(torch_dev):
    k = 31
    seqs = mixed_reads(k, 3)
    more = rnd_reads(77, 2, 400) + [seqs[0]]
    T = table_of(torch_dev, seqs, k)
    h0, st0 = T.hist(), T.stats()
    s1 = T.sorted()
    s2 = T.sorted()
    h1, st1 = T.hist(), T.stats()
    assert h0[:4] == h1[:4] and np.array_equal(h0[4], h1[4]) and st0 == st1
    old = KO.table(seqs, k)
    assert check(s1, old, k) == check(s2, old, k)
    s2.close()
    T.add_tensors(*flat(torch_dev, more))
    s3 = T.sorted()
    check(s3, KO.table(seqs + more, k), k)
    check(s1, old, k)                                      # the old snapshot did not follow
    s1.close()
    s3.close()
    T.close()


def test_consistent_with_the_histogram(torch_dev):
    k = 16
    seqs = mixed_reads(k, 4) + [b"ACGT" * 300]
    T = table_of(torch_dev, seqs, k)
    hist = T.hist()[4]
    s = T.sorted()
    c = s.counts.cpu().numpy()
    assert c.max() < 32767 and c.max() > 50
    assert np.array_equal(np.bincount(c, minlength=32768)[1:32767], hist[:32766])
    s.close()
    T.close()


def test_growth_and_batching(torch_dev):
    k = 40
    seqs = rnd_reads(23, 42, 1500)
    ents = KO.table(seqs, k)
    got = []
    for nb in (1, 3, 7):
        order = list(range(len(seqs)))
        random.Random(nb).shuffle(order)
        sh = [seqs[i] for i in order]
        batches = [sh[i * len(sh) // nb:(i + 1) * len(sh) // nb] for i in range(nb)]
        T = table_of(torch_dev, sh, k, batches=batches, initial_slots=64)
        assert T.stats()["growths"] >= 1
        s = T.sorted()
        got.append(check(s, ents, k))
        s.close()
        T.close()
    assert got[0] == got[1] == got[2]


def test_filtered_table(torch_dev):
    from classpro_amd._lib import ClassProError
    k = 40
    seqs = mixed_reads(k, 6) + rnd_reads(6, 4, 800)
    cnt = O.count(seqs, k)[0]
    T = table_of(torch_dev, seqs, k, filter_bits=1 << 20)
    with pytest.raises(ClassProError) as e:
        T.sorted(1)
    assert e.value.code == EINVAL
    assert T.stats()["n_distinct"] == len(cnt)             # still usable
    U = table_of(torch_dev, seqs, k)
    for minc in (2, 3):
        s, u = T.sorted(minc), U.sorted(minc)
        assert check(s, KO.entries(cnt, minc), k) == check(u, KO.entries(cnt, minc), k)
        s.close()
        u.close()
    T.close()
    U.close()
    from classpro_amd.api import KmerCounts
    T = KmerCounts(k, filter_bits=1 << 20)
    T.mark_tensors(*flat(torch_dev, seqs))
    T.add_tensors(*flat(torch_dev, seqs[:3]))
    with pytest.raises(ClassProError) as e:
        T.sorted(2)
    assert e.value.code == EINVAL and "cp_kmer_counts_sort" in str(e.value)
    T.close()


def test_bad_arguments(torch_dev):
    from classpro_amd._lib import ClassProError
    seqs = mixed_reads(21, 8)
    T = table_of(torch_dev, seqs, 21)
    for minc in (0, 32768, -1):
        with pytest.raises(ClassProError) as e:
            T.sorted(minc)
        assert e.value.code == EINVAL
    s = T.sorted()
    n = len(s)
    for first, m in ((-1, 2), (0, n + 1), (n, 1), (n + 1, 0), (2, -1)):
        with pytest.raises(ClassProError) as e:
            s.ktab(first, m)
        assert e.value.code == EINVAL, (first, m)
    check(s, KO.table(seqs, 21), 21)                       # nothing was harmed
    s.close()
    T.close()
    T = table_of(torch_dev, seqs, 4)
    s = T.sorted()
    check(s, KO.table(seqs, 4), 4, ktab=False)
    with pytest.raises(ClassProError) as e:
        s.ktab()
    assert e.value.code == EINVAL
    s.close()
    T.close()


def test_millions_of_keys_against_torch(torch_dev):
    """9 Mbases of DeviceSynth.  K = 31: the keys fit 62 bits, so torch.unique over independently packed canonical keys
    gives the whole expected snapshot.  K = 40: the snapshot's own keys, shuffled, sorted by torch in two stable passes
    (lo, then hi) give the snapshot's order back, the counts moving with them."""
    torch = torch_dev
    from classpro_amd.synth_dev import DeviceSynth
    from classpro_amd.api import KmerCounts
    ds = DeviceSynth(genome_len=3_000_000, cov=3, read_len=20000, K=40, seed=5)
    rd = ds.reads(0, ds.n_reads)
    seq, seq_off, total = rd["seq"], rd["seq_off"], rd["total_bases"]
    k = 31
    T = KmerCounts(k)
    T.add_tensors(seq, seq_off)
    s = T.sorted()
    code = torch.full((256,), -1, dtype=torch.int64, device=seq.device)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
    base = code[seq[:total].long()]
    assert bool((base >= 0).all())
    pos = torch.arange(total, device=seq.device)
    rid = torch.searchsorted(seq_off, pos, right=True) - 1
    ends = pos[pos >= seq_off[rid] + k - 1]
    fw = torch.zeros_like(ends)
    rc = torch.zeros_like(ends)
    for j in range(k):
        bj = base[ends - (k - 1) + j]
        fw = fw * 4 + bj
        rc = rc + ((3 - bj) << (2 * j))
    keys, cnt = torch.unique(torch.minimum(fw, rc), return_counts=True)
    assert keys.numel() > 2_000_000 and len(s) == keys.numel()
    assert bool((s.hi == 0).all()) and bool((s.lo == keys).all()) and bool((s.counts == cnt).all())
    two = T.sorted(2)
    keep = cnt >= 2
    assert len(two) == int(keep.sum()) and bool((two.lo == keys[keep]).all()) and bool((two.counts == cnt[keep]).all())
    two.close()
    s.close()
    T.close()
    del fw, rc, keys, cnt, pos, rid, ends, base
    k = 40
    T = KmerCounts(k)
    T.add_tensors(seq, seq_off)
    st = T.stats()
    s = T.sorted()
    n = len(s)
    assert n == st["n_distinct"] > 2_000_000 and int(s.counts.sum()) == st["n_kmers"]
    assert bool((s.hi > 0).any())
    perm = torch.randperm(n, device=seq.device)
    hi, lo, c = s.hi[perm], s.lo[perm], s.counts[perm]
    o = torch.sort(lo, stable=True)[1]
    hi, lo, c = hi[o], lo[o], c[o]
    o = torch.sort(hi, stable=True)[1]
    assert bool((hi[o] == s.hi).all()) and bool((lo[o] == s.lo).all()) and bool((c[o] == s.counts).all())
    same = (s.hi[1:] == s.hi[:-1]) & (s.lo[1:] == s.lo[:-1])
    assert not bool(same.any())
    s.close()
    T.close()

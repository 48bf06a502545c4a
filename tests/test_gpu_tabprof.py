"""Sorted snapshots as input (cp_kmer_sorted_load_*, _find, _profiles; SortedKmers.from_records, .find, .profiles) on a
real MI355X (`-m gpu`), against the brute-force lookups of tests/tabprof_oracle.py: the load as the inverse of the
encode, key lookups on hand-written tables around every edge of a bucket, profiles relative to a table for canonical and
forward keys with their tally, the count clamp, the load protocol, that a snapshot is only read, and millions of keys
against torch.searchsorted.  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import kprof_oracle as O
import ktab_oracle as KO
import tabprof_oracle as TO
from test_gpu_ktab import flat, mixed_reads, table_of
from test_ktab_host import KS

pytestmark = pytest.mark.gpu
EINVAL = -1
M63 = (1 << 63) - 1


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def i64(torch, xs):
    """Python ints below 2^63 as an int64 device tensor."""
    return torch.tensor([int(x) for x in xs], dtype=torch.int64, device="cuda:0")


def u8(b):
    return np.frombuffer(b, np.uint8).copy()


def load(torch, ents, k, piece=None):
    from classpro_amd.api import SortedKmers
    return SortedKmers.from_records(k, KO.index(ents, k), u8(KO.records_fast(ents, k)), piece=piece)


# ---- the load is the inverse of the encode ----

@pytest.mark.parametrize("k", KS)
def test_round_trip(torch_dev, k):
    torch = torch_dev
    from classpro_amd.api import SortedKmers
    T = table_of(torch, mixed_reads(k), k)
    s = T.sorted(1)
    rec, idx = s.ktab()
    n = len(s)
    assert n > 256 or k < 8
    buf = torch.zeros(rec.numel() + 1, dtype=torch.uint8, device="cuda:0")
    buf[1:] = rec
    odd = buf[1:]
    assert odd.data_ptr() % 2 == 1
    for piece in (1, 255, 256, 257, None):
        L = SortedKmers.from_records(k, idx, odd, piece=piece)
        assert len(L) == n and L.nbytes == s.nbytes
        assert torch.equal(L.hi, s.hi) and torch.equal(L.lo, s.lo) and torch.equal(L.counts, s.counts.clamp(max=KO.MAXC))
        rec2, idx2 = L.ktab()
        assert torch.equal(rec2, rec) and torch.equal(idx2, idx)
        L.close()
    L = SortedKmers.from_records(k, idx.cpu().numpy(), rec.cpu().numpy(), piece=100)        # host arrays as well
    assert torch.equal(L.lo, s.lo)
    L.close()
    s.close()
    T.close()


def test_round_trip_of_an_empty_table(torch_dev):
    torch = torch_dev
    L = load(torch, [], 21)
    assert len(L) == 0 and L.hi.numel() == 0
    assert L.find(i64(torch, [0, 5]), i64(torch, [0, 7])).tolist() == [-1, -1]
    seq, off = flat(torch, [b"ACGT" * 20, b"ACG"])
    tally = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    assert L.profiles((seq, off), tally=tally).cpu().numpy().tolist() == [0] * 60 and tally.tolist() == [0, 60, 0]
    rec, idx = L.ktab()
    assert rec.numel() == 0 and not bool(idx.any())
    L.close()


# ---- find ----

def hand_table(k, tile):
    """Entries around every edge: the first bucket with the first key, an empty bucket, buckets of 1, 2 and 3 entries,
    one of tile+1 (where a bucket has room for it), one whose entries differ only in hi or only in lo (where a bucket
    reaches into hi), the last bucket with the last key."""
    rng = random.Random(k)
    pbits = 8 * KO.ibyte_of(k)
    shift = 2 * k - pbits
    nb, room = 1 << pbits, 1 << shift

    def pick(m):
        out = set()
        while len(out) < min(m, room):
            out.add(rng.randrange(room))
        return sorted(out)

    suf = {0: sorted({0, room - 1}), 2: pick(1), 3: pick(3), 4: pick(2), nb - 1: sorted({room - 1, room // 2})}
    if room > tile + 1:
        suf[6] = pick(tile + 1)
    if shift > 63:                                         # K >= 44: the low bits of hi lie in the suffix
        los = [5, 9, (1 << 62) + 1]
        his = sorted({0, 1, (room >> 63) - 1})
        suf[9] = sorted((h << 63) | l for h in his for l in los)
    elif shift > 8:
        suf[9] = [5, 9, room - 7]
    keys = sorted((b << shift) | x for b, xs in suf.items() for x in xs)
    assert keys[0] == 0 and keys[-1] == (1 << (2 * k)) - 1 and len(set(keys)) == len(keys)
    return [(x, 1 + (i * 7919) % 40000) for i, x in enumerate(keys)], shift, nb, room


def queries(ents, k, shift, nb, room):
    top = 1 << (2 * k)
    qs = set()
    for x, _ in ents:
        qs |= {x, x - 1, x + 1}
    for b in (1, 5, 7, nb - 2):                            # empty buckets: their first and last key
        qs |= {b << shift, (b << shift) | (room - 1), (b << shift) | (room // 3)}
    for b in (0, 2, 3, 4, 6, 9, nb - 1):                   # below the first and above the last entry of a bucket
        qs |= {b << shift, (b << shift) | (room - 1)}
    return sorted(q for q in qs if 0 <= q < top)


@pytest.mark.parametrize("k", [5, 8, 12, 13, 21, 31, 32, 43, 44, 63])
def test_find_on_hand_written_tables(torch_dev, tmp_path, k):
    """K = 31 and 43 compare lo alone (2K-63 <= 24: every bit of hi lies in the prefix), K = 44 and 63 (hi, lo)."""
    torch = torch_dev
    from classpro_amd import fastk
    from classpro_amd.api import ktab_tile
    ents, shift, nb, room = hand_table(k, ktab_tile())
    if k in (21, 31, 43, 44, 63):
        assert len(ents) > ktab_tile()
    if k in (44, 63):
        lo_of = lambda x: x & M63
        pairs = [(a, b) for a, _ in ents for b, _ in ents if a < b and a >> shift == b >> shift == 9]
        assert any(lo_of(a) == lo_of(b) for a, b in pairs) and any(a >> 63 == b >> 63 for a, b in pairs)
    L = load(torch, ents, k, piece=1000)
    qs = queries(ents, k, shift, nb, room)
    want = TO.find(ents, qs)
    assert want.count(-1) > 10 and len(want) - want.count(-1) == len(ents)
    got = L.find(i64(torch, [q >> 63 for q in qs]), i64(torch, [q & M63 for q in qs])).tolist()
    assert got == want
    if k < 63:                                             # keys that no k-mer of this K has
        assert L.find(i64(torch, [(1 << (2 * k)) >> 63, 0]), i64(torch, [(1 << (2 * k)) & M63, -1])).tolist() == [-1, -1]
    assert L.find(i64(torch, []), i64(torch, [])).numel() == 0
    ref = KO.ref_lib()
    if ref is not None:                                    # Find_Kmer takes the canonical k-mer of its argument itself
        fastk.write_fastk_ktab(str(tmp_path), "tab", k, 1, [x for x, _ in ents], [c for _, c in ents], 3)
        R = KO.RefTable(ref, str(tmp_path / "tab"))
        canonical = [(q, w) for q, w in zip(qs, want) if KO.key_of(O.canon(KO.text_of(q, k).upper().encode())) == q]
        assert len(canonical) > 20
        for q, w in canonical:
            at = R.find(KO.text_of(q, k))
            assert (at if at >= 0 else -1) == w
        R.close()
    L.close()


def test_find_below_five(torch_dev):
    """K = 3: a bucket is the whole key; the snapshot comes from a count table, there is no .ktab to load."""
    torch = torch_dev
    seqs = [b"ACGTTGCA", b"AAAA", b"GGNCC"]
    ents = KO.table(seqs, 3)
    assert 0 < len(ents) < 32
    T = table_of(torch, seqs, 3)
    s = T.sorted()
    qs = list(range(64)) + [64, 200]
    assert s.find(i64(torch, [0] * len(qs)), i64(torch, qs)).tolist() == TO.find(ents, qs)
    s.close()
    T.close()


# ---- profiles ----

def batch_reads(k):
    rng = random.Random(31 * k)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    long = rnd(20000)
    return mixed_reads(k) + [rnd(k), rnd(k + 63), rnd(k + 64), rnd(k + 65), long + rnd(10000) + long]


@pytest.mark.parametrize("k", [3] + KS)
def test_profiles_against_the_oracle(torch_dev, k):
    torch = torch_dev
    from classpro_amd.api import Batch, KmerTable
    seqs = batch_reads(k)
    assert {len(s) for s in seqs} >= {0, k - 1, k, k + 63, k + 64, k + 65, 50000} and any(b"N" in s for s in seqs)
    cnt = O.count(seqs, k)[0]
    B = Batch.from_seqs(seqs, k)
    T = table_of(torch, seqs, k)
    own = T.profiles(B).view(torch.int16).clone()          # cells are at most 32767: compared as int16
    keys = TO.keys_of(seqs, k)
    for minc in (1, 2, 3):
        ents = KO.entries(cnt, minc)
        want, tally = TO.cells(ents, seqs, k, keys=keys)
        s = T.sorted(minc)
        t = torch.zeros(3, dtype=torch.int64, device="cuda:0")
        got = s.profiles(B, tally=t)
        assert got.data_ptr() == B.prof.data_ptr()         # the batch's own tensor, filled in place
        assert np.array_equal(got.cpu().numpy(), TO.flat(want))
        assert torch.equal(got.view(torch.int16), torch.where(own >= minc, own, torch.zeros_like(own)))
        assert t.tolist() == tally and sum(tally) == B.total_kmers and tally[2] > 0
        assert tally[1] == 0 if minc == 1 else (tally[1] > 0 or k < 9)
        again = s.profiles((B.seq, B.seq_off), tally=t)    # the tuple form; the tally goes on adding
        assert torch.equal(again.view(torch.int16), got.view(torch.int16)) and t.tolist() == [2 * x for x in tally]
        s.close()
    T.close()
    other = mixed_reads(k, 7) + [seqs[2][:400], seqs[-1][100:3000]]                          # a table of another read set
    ents = KO.table(other, k)
    want, tally = TO.cells(ents, seqs, k, keys=keys)
    assert tally[0] > 0 and (tally[1] > 0 or k < 9)
    U = table_of(torch, other, k)
    s = U.sorted()
    assert np.array_equal(s.profiles(B).cpu().numpy(), TO.flat(want))
    if k >= 5:                                             # and the same table loaded from its records
        L = load(torch, ents, k, piece=999)
        assert np.array_equal(L.profiles(B).cpu().numpy(), TO.flat(want))
        L.close()
    s.close()
    U.close()
    fw = {}                                                # forward keys: a forward label table of the same reads
    for s_ in other:
        for key in TO.read_keys(s_, k, canonical=False):
            if key is not None:
                fw[key] = fw.get(key, 0) + 1
    ents = sorted(fw.items())
    want, tally = TO.cells(ents, seqs, k, canonical=False)
    F = KmerTable(k, canonical=False)
    seq, off = flat(torch, other)
    F.add_tensors(seq, off, torch.full_like(seq, ord("H")))
    s = F.sorted()
    assert len(s) == len(ents)
    t = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    assert np.array_equal(s.profiles(B, canonical=False, tally=t).cpu().numpy(), TO.flat(want)) and t.tolist() == tally
    if k >= 12:
        assert not np.array_equal(s.profiles(B, canonical=True).cpu().numpy(), TO.flat(want))
    s.close()
    F.close()


def test_clamp(torch_dev):
    torch = torch_dev
    from classpro_amd.api import Batch
    k = 40
    seqs = [b"A" * 40000]
    T = table_of(torch, seqs, k)
    s = T.sorted()
    assert len(s) == 1 and int(s.counts[0]) == 40000 - k + 1
    got = s.profiles(Batch.from_seqs(seqs, k))
    assert got.numel() == 40000 - k + 1 and bool((got.view(torch.int16) == 32767).all())
    s.close()
    T.close()


# ---- the load protocol ----

def test_protocol(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import ClassProError, lib
    from classpro_amd.api import SortedKmers
    L = lib()
    k = 21
    shift = 2 * k - 24
    keys = [(2 << shift) | 5, (7 << shift) | 1, (7 << shift) | 6, (7 << shift) | 9, (9 << shift) | 3]
    ents = [(x, i + 1) for i, x in enumerate(keys)]
    index = KO.index(ents, k)
    rec = KO.records_fast(ents, k)
    pbyte = len(rec) // len(ents)
    d_rec = torch.from_numpy(u8(rec)).cuda()
    err = lambda: L.cp_last_error().decode()
    h = C.c_void_p()
    begin = lambda kk, idx: L.cp_kmer_sorted_load_begin(kk, idx.ctypes.data if idx is not None else None, C.byref(h))
    down = index.copy()
    down[300] = down[299] - 1 if down[299] > 0 else -1
    neg = index.copy()
    neg[0] = -1
    for kk, idx in ((k, down), (k, neg), (4, index), (64, index), (k, None)):
        assert begin(kk, idx) == EINVAL and h.value is None, (kk, err())
    assert "prefix 300" in (begin(k, down), err())[1]
    assert L.cp_kmer_sorted_load_begin(k, index.ctypes.data, None) == EINVAL
    assert begin(k, index) == 0 and h.value
    q = i64(torch, [0])
    pos = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    seq, off = flat(torch, [b"ACGT" * 10])
    poff = torch.tensor([0, 40 - k + 1], dtype=torch.int64, device="cuda:0")
    prof = torch.zeros(64, dtype=torch.int16, device="cuda:0")
    p3 = [C.c_void_p() for _ in range(3)]

    def not_ready():
        assert L.cp_kmer_sorted_find(h, q.data_ptr(), q.data_ptr(), 1, pos.data_ptr(), None) == EINVAL
        assert L.cp_kmer_sorted_profiles(h, 1, seq.data_ptr(), off.data_ptr(), poff.data_ptr(), 1, 40, prof.data_ptr(), None,
                                         None) == EINVAL
        assert L.cp_kmer_sorted_ktab(h, 0, 0, None, None, None) == EINVAL
        assert L.cp_kmer_sorted_arrays(h, *[C.byref(x) for x in p3]) == EINVAL
        assert L.cp_kmer_sorted_size(h) == len(ents)

    not_ready()
    assert L.cp_kmer_sorted_load_end(h, None) == EINVAL and "0 of 5" in err()             # too early
    assert L.cp_kmer_sorted_load_records(h, 6, d_rec.data_ptr(), None) == EINVAL          # past n
    assert L.cp_kmer_sorted_load_records(h, 2, None, None) == EINVAL
    assert L.cp_kmer_sorted_load_records(h, -1, d_rec.data_ptr(), None) == EINVAL
    assert L.cp_kmer_sorted_load_records(h, 2, d_rec.data_ptr(), None) == 0
    assert L.cp_kmer_sorted_load_records(h, 4, d_rec.data_ptr() + 2 * pbyte, None) == EINVAL and "past" in err()
    not_ready()
    assert L.cp_kmer_sorted_load_end(h, None) == EINVAL and "2 of 5" in err()
    assert L.cp_kmer_sorted_load_records(h, 0, None, None) == 0
    assert L.cp_kmer_sorted_load_records(h, 3, d_rec.data_ptr() + 2 * pbyte, None) == 0
    assert L.cp_kmer_sorted_load_end(h, None) == 0
    assert L.cp_kmer_sorted_load_end(h, None) == EINVAL                                    # ready: not being loaded
    assert L.cp_kmer_sorted_load_records(h, 0, None, None) == EINVAL
    assert L.cp_kmer_sorted_find(h, q.data_ptr(), q.data_ptr(), 1, pos.data_ptr(), None) == 0
    L.cp_kmer_sorted_destroy(h)
    for null in range(3):                                  # NULL arguments
        a = [q.data_ptr(), q.data_ptr(), pos.data_ptr()]
        a[null] = None
        s = load(torch, ents, k)
        assert L.cp_kmer_sorted_find(s.s, a[0], a[1], 1, a[2], None) == EINVAL
        s.close()
    assert L.cp_kmer_sorted_find(None, q.data_ptr(), q.data_ptr(), 1, pos.data_ptr(), None) == EINVAL
    assert L.cp_kmer_sorted_profiles(None, 1, seq.data_ptr(), off.data_ptr(), poff.data_ptr(), 1, 40, prof.data_ptr(), None,
                                     None) == EINVAL
    s = load(torch, ents, k)
    for null in range(4):
        a = [seq.data_ptr(), off.data_ptr(), poff.data_ptr(), prof.data_ptr()]
        a[null] = None
        assert L.cp_kmer_sorted_profiles(s.s, 1, a[0], a[1], a[2], 1, 40, a[3], None, None) == EINVAL
    s.close()
    assert L.cp_kmer_sorted_load_records(None, 0, None, None) == EINVAL and L.cp_kmer_sorted_load_end(None, None) == EINVAL
    swapped = [ents[0], ents[1], ents[3], ents[2], ents[4]]                                # inside bucket 7: the index is the same
    with pytest.raises(ClassProError) as e:
        SortedKmers.from_records(k, index, u8(KO.records_fast(swapped, k)))
    assert e.value.code == EINVAL and "entry 3 " in str(e.value)
    twice = [ents[0], ents[1], ents[2], ents[2], ents[4]]
    with pytest.raises(ClassProError) as e:
        SortedKmers.from_records(k, index, u8(KO.records_fast(twice, k)), piece=2)
    assert e.value.code == EINVAL and "entry 3 " in str(e.value)
    with pytest.raises(ClassProError) as e:                # a record more than the index says
        SortedKmers.from_records(k, index, u8(rec + rec[:pbyte]))
    assert e.value.code == EINVAL
    with pytest.raises(ClassProError) as e:                # a record fewer
        SortedKmers.from_records(k, index, u8(rec[pbyte:]))
    assert e.value.code == EINVAL
    for bad in (down, neg):
        with pytest.raises(ClassProError) as e:
            SortedKmers.from_records(k, bad, u8(rec))
        assert e.value.code == EINVAL
    s = load(torch, ents, k)                               # a good load and lookup in the same process afterwards
    assert s.find(i64(torch, [x >> 63 for x in keys] + [0]), i64(torch, [x & M63 for x in keys] + [4])).tolist() == [0, 1, 2, 3, 4, -1]
    assert s.counts.tolist() == [1, 2, 3, 4, 5]
    s.close()


def test_snapshot_is_only_read(torch_dev):
    torch = torch_dev
    from classpro_amd.api import Batch
    k = 40
    seqs = mixed_reads(k, 3)
    T = table_of(torch, seqs, k)
    for s in (T.sorted(), load(torch, KO.table(seqs, k), k)):
        before = [x.clone() for x in (s.hi, s.lo, s.counts)]
        rec0, idx0 = s.ktab()
        s.profiles(Batch.from_seqs(batch_reads(k), k))
        s.profiles(Batch.from_seqs(seqs, k), canonical=False)
        s.find(s.hi.clone(), s.lo.clone() ^ 1)
        assert s.find(s.hi.clone(), s.lo.clone()).tolist() == list(range(len(s)))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (s.hi, s.lo, s.counts)))
        rec1, idx1 = s.ktab()
        assert torch.equal(rec0, rec1) and torch.equal(idx0, idx1)
        s.close()
    T.close()


def test_millions_of_keys_against_torch(torch_dev):
    """K = 31: a key fits an int64.  2 M random distinct keys with random counts, their records and index made by torch,
    loaded in pieces; 4 M queries, half of them present, against torch.searchsorted."""
    torch = torch_dev
    from classpro_amd.api import SortedKmers
    k, n, m = 31, 2_000_000, 4_000_000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(31)
    keys = torch.unique(torch.randint(0, 1 << 62, (n + n // 8,), device=dev, generator=g))
    keys = keys[torch.randperm(keys.numel(), device=dev, generator=g)[:n]].sort()[0]
    assert keys.numel() == n
    cnt = torch.randint(1, 32768, (n,), device=dev, generator=g)
    left = keys << 2                                       # 62 bits left-aligned in 8 bytes; 3 prefix bytes, 5 in the record
    rec = torch.empty((n, 7), dtype=torch.uint8, device=dev)
    for b in range(5):
        rec[:, b] = ((left >> (8 * (4 - b))) & 255).to(torch.uint8)
    rec[:, 5] = (cnt & 255).to(torch.uint8)
    rec[:, 6] = (cnt >> 8).to(torch.uint8)
    index = torch.cumsum(torch.bincount(keys >> 38, minlength=1 << 24), 0)
    s = SortedKmers.from_records(k, index, rec.reshape(-1), piece=300_001)
    assert len(s) == n and not bool(s.hi.any()) and torch.equal(s.lo, keys) and torch.equal(s.counts, cnt)
    present = keys[torch.randint(0, n, (m // 2,), device=dev, generator=g)]
    q = torch.cat([present, torch.randint(0, 1 << 62, (m // 2,), device=dev, generator=g)])
    q = q[torch.randperm(m, device=dev, generator=g)]
    at = torch.searchsorted(keys, q)
    hit = keys[at.clamp(max=n - 1)] == q
    want = torch.where(hit, at, torch.full_like(at, -1))
    assert int(hit.sum()) >= m // 2
    got = s.find(torch.zeros_like(q), q)
    assert torch.equal(got, want)
    s.close()

"""cp_kmer_sorted_read_hits (SortedKmers.read_hits) on a real MI355X (`-m gpu`), against the plain loops of
tests/readhits_oracle.py: reads whose markers are written out, reads packed into the chunks of single lanes, a read over
five blocks with whole blocks that hold no marker, random read sets for lookups with and without hi[], canonical and
forward keys and count ranges on either side, the identities with `profiles` and `combine`, batching, and that both
tables are only read.  Everything is integers: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import ktab_oracle as KO
import readhits_oracle as RO
import tabprof_oracle as TO
from test_gpu_ktab import flat, mixed_reads, table_of
from test_gpu_tabprof import load

pytestmark = pytest.mark.gpu
EINVAL = -1
BLOCK = 16384                                              # base positions per block of the kernel
RANGES = (None, (2, None), (None, 1), (2, 3))


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def rnd(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def hits(torch, A, B, seqs, **kw):
    return A.read_hits(B, flat(torch, seqs), **kw).cpu().tolist()


def tables_for(seqs, K, marks):
    """Two entry lists that give the reads the marker strings written in `marks` ('A', 'B', '2' or '.' per k-mer position,
    'o' where the k-mer holds another byte); the oracle confirms that they do."""
    a, b = set(), set()
    for s, m in zip(seqs, marks):
        keys = TO.read_keys(s, K)
        assert len(keys) == len(m)
        for key, x in zip(keys, m):
            assert (key is None) == (x == "o")
            if x in "A2":
                a.add(key)
            if x in "B2":
                b.add(key)
    a, b = [(k, 1) for k in sorted(a)], [(k, 1) for k in sorted(b)]
    assert [RO.markers(s, K, RO.present(a, None), RO.present(b, None)) for s in seqs] == list(marks)
    return a, b


# ---- 1. reads whose markers are written here ----

def hand_case():
    K = 5
    rng = random.Random(10)
    r0, r1, r4a, r4b, r8 = rnd(rng, 11), rnd(rng, K), rnd(rng, 6), rnd(rng, 6), rnd(rng, 12)
    seqs = [r0, r1, rnd(rng, 3), b"", r4a + b"N" + r4b, r0.lower(), b"", rnd(rng, 2), r8, rnd(rng, K - 1)]
    marks = ["AA.B2BA", "B", "", "", "A.ooooo.B", "ooooooo", "", "", "BABAB..A", ""]
    want = [[3, 2, 1, 0, 2], [0, 1, 0, 0, 0], [0] * 5, [0] * 5, [1, 1, 0, 5, 1], [0, 0, 0, 7, 0], [0] * 5, [0] * 5,
            [3, 3, 0, 0, 5], [0] * 5]
    return K, seqs, marks, want


def test_hand_made(torch_dev):
    torch = torch_dev
    K, seqs, marks, want = hand_case()
    a, b = tables_for(seqs, K, marks)
    assert [RO.row_of(m) for m in marks] == want
    A, B, E = load(torch, a, K), load(torch, b, K), load(torch, [], K)
    assert hits(torch, A, B, seqs) == want
    assert hits(torch, B, A, seqs) == [[r[1], r[0]] + r[2:] for r in want]
    none = A.read_hits(B, flat(torch, []))
    assert tuple(none.shape) == (0, 5) and none.dtype == torch.int64
    assert hits(torch, A, B, [b"", b"ACG", b""]) == [[0] * 5] * 3
    in_a = [[m.count("A") + m.count("2"), 0, 0, m.count("o"), 0] for m in marks]
    assert hits(torch, A, E, seqs) == in_a                                             # an empty B: A and BOTH mark A
    assert hits(torch, E, A, seqs) == [[0, r[0], 0, r[3], 0] for r in in_a]            # an empty A
    assert hits(torch, E, E, seqs) == [[0, 0, 0, m.count("o"), 0] for m in marks]
    assert hits(torch, A, A, seqs) == [[0, 0, r[0], r[3], 0] for r in in_a]            # a is b: every hit is BOTH
    assert hits(torch, A, B, seqs + seqs) == want + want                               # the same reads twice in one batch
    for s in (A, B, E):
        s.close()


# ---- 2. many reads inside one lane's chunk ----

def lane_case(K, n=100):
    rng = random.Random(K)
    seen, reads = set(), []
    while len(reads) < n:
        r = rnd(rng, K)
        key = TO.read_keys(r, K)[0]
        if key not in seen:
            seen.add(key)
            reads.append(r)
    a = sorted((TO.read_keys(r, K)[0], 1) for r in reads[0::2])
    b = sorted((TO.read_keys(r, K)[0], 1) for r in reads[1::2])
    return reads, a, b


@pytest.mark.parametrize("K", [5, 21])
def test_reads_of_exactly_k_bases_in_a_row(torch_dev, K):
    """100 reads of K bases: at K = 5 twelve of them lie in the 64 positions of one lane.  Each has one k-mer and no
    switch; the same bases as one read switch at every alternation (at K = 21 the k-mers across the joins are in neither
    table, so that is 99 times; at K = 5 the oracle says how often)."""
    torch = torch_dev
    reads, a, b = lane_case(K)
    A, B = load(torch, a, K), load(torch, b, K)
    assert hits(torch, A, B, reads) == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0]] * (len(reads) // 2)
    one = b"".join(reads)
    want = RO.rows(a, b, [one], K)
    assert want == [[50, 50, 0, 0, 99]] if K == 21 else want[0][4] > 30
    assert hits(torch, A, B, [one]) == want
    mixed = reads[:70] + [one] + reads[70:] + [b"", one[:K - 1], one[3:]]
    assert hits(torch, A, B, mixed) == RO.rows(a, b, mixed, K)
    A.close()
    B.close()


# ---- 3. a read over five blocks, whole blocks without a marker ----

def block_case(nblocks, last, same):
    """One random read of nblocks * BLOCK + 200 bases at K = 21.  The k-mers that end within K + 70 bases of base BLOCK and
    of base last * BLOCK of the read alternate A B A B ..., and no other k-mer is in a table; with `same` the second run
    starts with the marker the first one ended on."""
    K = 21
    read = bytes(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(77).integers(0, 4, nblocks * BLOCK + 200)])
    keys = TO.read_keys(read, K)
    runs = [[j - (K - 1) for j in range(c * BLOCK - (K + 70), c * BLOCK + (K + 70) + 1)] for c in (1, last)]
    marks = {}
    for t, i in enumerate(runs[0]):
        marks[i] = "AB"[t % 2]
    end = marks[runs[0][-1]]
    first = "AB".index(end) if same else 1 - "AB".index(end)
    for t, i in enumerate(runs[1]):
        marks[i] = "AB"[(first + t) % 2]
    a = sorted((keys[i], 1) for i, m in marks.items() if m == "A")
    b = sorted((keys[i], 1) for i, m in marks.items() if m == "B")
    got = RO.markers(read, K, RO.present(a, None), RO.present(b, None), keys=keys)
    assert got == "".join(marks.get(i, ".") for i in range(len(keys)))                # no k-mer of the read repeats a marked one
    return K, read, a, b, RO.row_of(got)


def prefix_of(rng, total, K):
    """Short reads of `total` bases in all, some of them shorter than K."""
    out = []
    while total > 0:
        n = min(total, rng.choice([40, 40, 40, K, K - 1, 7]))
        out.append(rnd(rng, n))
        total -= n
    return out


@pytest.mark.parametrize("nblocks,last", [(5, 4), (7, 6)])
def test_block_edges(torch_dev, nblocks, last):
    """A read of 5 blocks and 200 bases with markers round its bases 16384 and 65536, and one of 7 blocks with markers round
    16384 and 98304.  A run of markers reaches K + 70 bases into the blocks on either side of it, so the gap of the first
    read crosses two block edges and holds one whole block of the batch without a marker, the gap of the second crosses
    four edges and holds three; the prefixes move the edges to other places of the read.  Every lane and block in the gap
    has to hand the last marker on unchanged: with it the two variants differ by the one switch across the gap."""
    torch = torch_dev
    rows = {}
    rng = random.Random(nblocks)
    for same in (False, True):
        K, read, a, b, row = block_case(nblocks, last, same)
        rows[same] = row
        A, B = load(torch, a, K), load(torch, b, K)
        for total in (0, 37, 16379):
            pre = prefix_of(rng, total, K)
            assert sum(len(p) for p in pre) == total
            lo, hi = total + BLOCK + K + 70, total + last * BLOCK - (K + 70)          # the gap, in bases of the batch
            assert hi // BLOCK - (lo + BLOCK) // BLOCK == (1 if nblocks == 5 else 3)   # whole blocks between lo and hi
            seqs = pre + [read, rnd(rng, 30)]
            want = RO.rows(a, b, pre, K) + [row] + RO.rows(a, b, seqs[-1:], K)
            assert hits(torch, A, B, seqs) == want, (same, total)
        A.close()
        B.close()
    n = 2 * (K + 70) + 1                                   # markers per run, an odd number: a run ends as it begins
    assert rows[False] == [n, n, 0, 0, 2 * n - 1] and rows[True] == [n + 1, n - 1, 0, 0, 2 * n - 2]
    assert rows[False][4] == rows[True][4] + 1             # the gap itself is the one switch


# ---- 4. random reads, every kind of lookup ----

def random_case(K):
    ra, rb = mixed_reads(K, 5), mixed_reads(K, 7)
    rng = random.Random(K)
    third = [ra[2][:900] + rb[2][300:1500] + ra[1][:400], rb[0] + ra[0], rnd(rng, 500), ra[6], rb[3][:K], b"", rb[1][:K - 1],
             ra[2][1000:] + b"N" + rb[2][2000:], ra[9] + rb[10].lower() + rb[9]]
    return KO.table(ra, K), KO.table(rb, K), ra[:3] + third + rb[:2]


@pytest.mark.parametrize("K", [5, 12, 21, 31, 32, 40, 44, 63])
def test_random_reads(torch_dev, K):
    """Up to K = 40 a lookup compares lo alone (every bit of hi lies in the prefix); K = 44 and 63 compare (hi, lo)."""
    torch = torch_dev
    a, b, seqs = random_case(K)
    assert K == 5 or ({c for _, c in a} >= {1, 2, 3} and {c for _, c in b} >= {1, 2, 3})
    A, B = load(torch, a, K, piece=999), load(torch, b, K)
    batch = flat(torch, seqs)
    seen = set()
    for canonical in (True, False):
        keys = TO.keys_of(seqs, K, canonical)
        for ar in RANGES:
            for br in RANGES:
                want = RO.rows(a, b, seqs, K, canonical, ar, br, keys=keys)
                got = A.read_hits(B, batch, canonical=canonical, a_range=ar, b_range=br).cpu().tolist()
                assert got == want, (canonical, ar, br)
                seen.add(tuple(map(tuple, want)))
    tot = [sum(r[c] for r in RO.rows(a, b, seqs, K)) for c in range(5)]
    assert tot[3] > 0 and (tot[2] > 100 if K == 5 else tot[0] > 100 and tot[1] > 100 and tot[4] > 0)
    assert len(seen) > 16                                  # the ranges and the strand change the rows
    A.close()
    B.close()


# ---- 5. against code that exists ----

def nonzero_per_read(torch, prof, seq_off, K):
    n = (seq_off[1:] - seq_off[:-1] - (K - 1)).clamp(min=0)
    off = torch.zeros(n.numel() + 1, dtype=torch.int64, device=n.device)
    torch.cumsum(n, 0, out=off[1:])
    csum = torch.zeros(prof.numel() + 1, dtype=torch.int64, device=n.device)
    torch.cumsum((prof.view(torch.int16) != 0).to(torch.int64), 0, out=csum[1:])
    return (csum[off[1:]] - csum[off[:-1]]).cpu().tolist()


@pytest.mark.parametrize("K", [21, 40])
def test_against_profiles_and_combine(torch_dev, K):
    """Snapshots sorted here (exact counts), not loaded ones."""
    torch = torch_dev
    ra, rb = mixed_reads(K, 5), mixed_reads(K, 7)
    _, _, seqs = random_case(K)
    TA, TB = table_of(torch, ra + seqs[3:5], K), table_of(torch, rb + seqs[3:4], K)
    A, B = TA.sorted(), TB.sorted()
    seq, off = flat(torch, seqs)
    in_a = nonzero_per_read(torch, A.profiles((seq, off)).clone(), off, K)
    assert sum(in_a) > 1000
    for ar, br in ((None, None), (None, (2, None)), ((2, None), None), ((None, 1), (2, 3)), ((2, 3), (None, 1))):
        h = A.read_hits(B, (seq, off), a_range=ar, b_range=br).cpu().tolist()
        if ar is None:
            assert [r[0] + r[2] for r in h] == in_a, (ar, br)
        D = A.combine(B, "sub", a_range=ar, b_range=br)
        assert [r[0] for r in h] == nonzero_per_read(torch, D.profiles((seq, off)).clone(), off, K), (ar, br)
        assert sum(r[0] for r in h) > 0
        D.close()
    for s in (A, B, TA, TB):
        s.close()


# ---- 6. batching ----

def test_batching(torch_dev):
    torch = torch_dev
    from classpro_amd.api import Batch
    K = 21
    a, b, seqs = random_case(K)
    long_k, long_read, la, lb, long_row = block_case(5, 4, False)
    assert long_k == K
    a, b = sorted({**dict(la), **dict(a)}.items()), sorted({**dict(lb), **dict(b)}.items())
    seqs = seqs[:6] + [long_read] + seqs[6:]
    A, B = load(torch, a, K), load(torch, b, K)
    whole = hits(torch, A, B, seqs)
    assert whole == RO.rows(a, b, seqs, K) and whole[6] == long_row
    assert [hits(torch, A, B, [s])[0] for s in seqs] == whole
    assert hits(torch, A, B, seqs[::-1]) == whole[::-1]
    assert A.read_hits(B, Batch.from_seqs(seqs, K)).cpu().tolist() == whole            # a Batch as well as the tuple
    A.close()
    B.close()


# ---- 7. the tables are only read; arguments ----

def test_tables_are_only_read(torch_dev):
    torch = torch_dev
    K = 40
    a, b, seqs = random_case(K)
    TA = table_of(torch, mixed_reads(K, 5), K)
    for A, B in ((load(torch, a, K), load(torch, b, K)), (TA.sorted(), load(torch, b, K))):
        before = [[x.clone() for x in s.ktab()] for s in (A, B)]
        A.read_hits(B, flat(torch, seqs))
        A.read_hits(B, flat(torch, seqs), canonical=False, a_range=(2, None), b_range=(None, 2))
        B.read_hits(A, flat(torch, seqs[::-1]))
        A.read_hits(A, flat(torch, seqs))
        torch.cuda.synchronize()
        after = [s.ktab() for s in (A, B)]
        assert all(torch.equal(x, y) for s0, s1 in zip(before, after) for x, y in zip(s0, s1))
        A.close()
        B.close()
    TA.close()


def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import ClassProError, lib
    L = lib()
    K = 21
    a, b, seqs = random_case(K)
    A, B, B12 = load(torch, a, K), load(torch, b, K), load(torch, KO.table(mixed_reads(12), 12), 12)
    seq, off = flat(torch, seqs)
    n, total = len(seqs), int(off[-1])
    out = torch.full((n, 5), -7, dtype=torch.int64, device="cuda:0")
    go = lambda x, y, rng, s, o, nr, tb, h: L.cp_kmer_sorted_read_hits(x, y, 1, rng, s, o, nr, tb, h, None)
    r4 = lambda *v: (C.c_int64 * 4)(*v)
    assert go(None, B.s, None, seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    assert go(A.s, None, None, seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    assert go(A.s, B12.s, None, seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    assert b"21-mers and 12-mers" in L.cp_last_error()
    for bad in (r4(0, 5, 1, 5), r4(3, 2, 1, 5), r4(1, 5, 0, 5), r4(1, 5, 4, 3), r4(-1, -1, 1, 1)):
        assert go(A.s, B.s, bad, seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    assert go(A.s, B.s, None, seq.data_ptr(), off.data_ptr(), -1, total, out.data_ptr()) == EINVAL
    assert go(A.s, B.s, None, seq.data_ptr(), off.data_ptr(), n, -1, out.data_ptr()) == EINVAL
    assert go(A.s, B.s, None, None, off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    assert go(A.s, B.s, None, seq.data_ptr(), None, n, total, out.data_ptr()) == EINVAL
    assert go(A.s, B.s, None, seq.data_ptr(), off.data_ptr(), n, total, None) == EINVAL
    h, index = C.c_void_p(), KO.index(a, K)               # a snapshot that is still being loaded
    assert L.cp_kmer_sorted_load_begin(K, index.ctypes.data, C.byref(h)) == 0
    assert go(h, B.s, None, seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    assert go(A.s, h, None, seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == EINVAL
    L.cp_kmer_sorted_destroy(h)
    torch.cuda.synchronize()
    assert bool((out == -7).all())                         # no call above launched anything
    assert go(A.s, B.s, None, None, None, 0, 0, None) == 0                             # no reads: no work, no error
    assert go(A.s, B.s, r4(1, 1, 1, 1), seq.data_ptr(), off.data_ptr(), n, total, out.data_ptr()) == 0
    assert out.cpu().tolist() == RO.rows(a, b, seqs, K, True, (1, 1), (1, 1))
    with pytest.raises(ValueError):
        A.read_hits(B12, (seq, off))
    with pytest.raises(ValueError):
        A.read_hits(None, (seq, off))
    with pytest.raises(ClassProError):
        A.read_hits(B, (seq, off), a_range=(0, None))
    B.close()
    with pytest.raises(ValueError):
        A.read_hits(B, (seq, off))
    A.close()
    B12.close()

"""The 2-D count comparison of two sorted snapshots (cp_kmer_sorted_compare_hist; SortedKmers.compare_hist) on a real
MI355X (`-m gpu`), against the dict restatement of tests/cmphist_oracle.py: hand-written tables with equal pairs on tile
cuts, sizes around a tile, every weight and several matrix shapes, counts at the fold and past the record's clamp, count
ranges, empty operands, the identities that tie it to compare and hist, the grid and on-chip knobs, that operands are only
read, the argument checks, and millions of keys against torch.  Everything is integers: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import cmphist_oracle as CO
import ktab_oracle as KO
from test_gpu_ktab import mixed_reads, table_of
from test_gpu_setop import clamped, rnd_entries
from test_gpu_tabprof import hand_table, load

pytestmark = pytest.mark.gpu
EINVAL = -1
WEIGHTS = ("keys", "a", "b")
SHAPES = ((1, 1), (8, 1000), (300, 300), (32767, 127))


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def tile(torch_dev):
    from classpro_amd.api import ktab_tile
    return ktab_tile()


def check_hist(A, B, a, b, shapes=((8, 1000),), weights=WEIGHTS, a_range=None, b_range=None):
    """A.compare_hist(B) against the oracle over the entries a and b; returns the last "keys" matrix."""
    keys = None
    for xmax, ymax in shapes:
        for w in weights:
            got = A.compare_hist(B, xmax, ymax, w, a_range, b_range)
            want = CO.matrix(a, b, xmax, ymax, w, a_range, b_range)
            assert got.shape == want.shape and got.dtype == np.int64
            assert np.array_equal(got, want), (xmax, ymax, w, np.argwhere(got != want)[:5].tolist())
            assert got[0, 0] == 0
            if w == "keys":
                keys = got
    return keys


def mixed_counts(ents, mod):
    """Every second entry gets a low count, so that the low corner and the far cells both fill."""
    return [(x, c if i % 2 else 1 + i % mod) for i, (x, c) in enumerate(ents)]


# ---- 1. hand-written tables ----

@pytest.mark.parametrize("k", [5, 13, 31, 32, 44, 63])
def test_hand_written_tables(torch_dev, tile, k):
    """2K <= 63 runs the form without hi[], K = 32, 44 and 63 the one with it.  B shares every second key of A and has
    the neighbours of every third, so equal pairs fall on tile cuts."""
    torch = torch_dev
    a, shift, nb, room = hand_table(k, tile)
    top = 1 << (2 * k)
    akeys = [x for x, _ in a]
    bkeys = set(akeys[::2])
    for x in akeys[1::3]:
        bkeys |= {y for y in (x - 1, x + 1) if 0 <= y < top}
    b = mixed_counts([(x, 1 + (i * 104729) % 30011) for i, x in enumerate(sorted(bkeys))], 5)
    a = mixed_counts(clamped(a), 7)
    assert set(akeys) & bkeys and bkeys - set(akeys) and set(akeys) - bkeys
    if k >= 31:
        assert len(a) > tile and len(a) + len(b) > 2 * tile
    A, B = load(torch, a, k), load(torch, b, k, piece=777)
    keys = check_hist(A, B, a, b, shapes=SHAPES)
    assert CO.tally(keys) == A.compare(B)
    A.close()
    B.close()


# ---- 2. sizes around a tile ----

@pytest.mark.parametrize("which", [-1, 0, 1, 2])
def test_sizes_around_a_tile(torch_dev, tile, which):
    """tile-1, tile, tile+1 and 2*tile+1 entries on either side: every weight and every shape at every pair of sizes."""
    torch = torch_dev
    k = 21
    pool = mixed_counts(clamped(rnd_entries(random.Random(3), 2 * tile + 2, k)), 6)
    size = lambda w: 2 * tile + 1 if w == 2 else tile + w
    part = lambda n, side: sorted(random.Random(n * 2 + side).sample(pool, n))
    a = part(size(which), 0)
    A = load(torch, a, k)
    for other in (-1, 0, 1, 2):
        b = part(size(other), 1)
        assert {x for x, _ in a} & {x for x, _ in b}
        B = load(torch, b, k)
        check_hist(A, B, a, b, shapes=SHAPES)
        B.close()
    A.close()


def test_pairs_across_tile_cuts(torch_dev, tile):
    """Every key of B is a pair; 0 to 3 extra keys of A below them shift every pair against the cuts."""
    torch = torch_dev
    k = 21
    s = rnd_entries(random.Random(tile), 3 * tile + 5, k, lo=100, hi=(1 << 42) - 100)
    s2 = [(x, 1 + c % 11) for x, c in s]
    S2 = load(torch, s2, k)
    for np_ in (0, 1, 2, 3):
        ps = clamped(sorted([(7 * i + 3, 5 + i) for i in range(np_)] + s))
        PS = load(torch, ps, k)
        keys = check_hist(PS, S2, ps, s2, shapes=((300, 300),))
        assert CO.tally(keys) == (np_, 0, len(s))
        keys = check_hist(S2, PS, s2, ps, shapes=((300, 300),))
        assert CO.tally(keys) == (0, np_, len(s))
        PS.close()
    S2.close()


# ---- 3. counts ----

def test_counts_at_the_fold(torch_dev):
    """Counts at xmax-1, xmax and xmax+1 on either side, alone and paired."""
    torch = torch_dev
    k = 21
    for xmax, ymax in ((8, 8), (8, 300), (63, 7), (7, 64), (1, 1)):
        cs = sorted({1, xmax - 1, xmax, xmax + 1, ymax - 1, ymax, ymax + 1} - {0})
        a = [(10 * i + 1, c) for i, c in enumerate(cs)] + [(1000 + 10 * i * len(cs) + 10 * j, c) for i, c in enumerate(cs) for j in range(len(cs))]
        b = [(10 * i + 2, c) for i, c in enumerate(cs)] + [(1000 + 10 * i * len(cs) + 10 * j, c) for i in range(len(cs)) for j, c in enumerate(cs)]
        A, B = load(torch, sorted(a), k), load(torch, sorted(b), k)
        keys = check_hist(A, B, sorted(a), sorted(b), shapes=((xmax, ymax),))
        assert keys[xmax, ymax] == sum(c >= xmax for c in cs) * sum(c >= ymax for c in cs)
        assert keys[xmax, 0] == sum(c >= xmax for c in cs) and keys[0, ymax] == sum(c >= ymax for c in cs)
        A.close()
        B.close()


def test_counts_past_the_clamp_and_ranges(torch_dev):
    """A snapshot sorted here holds the exact count of the one read added many times over; the loaded one 32767."""
    torch = torch_dev
    k = 40
    seqs = [b"A" * (40000 + k - 1)] + mixed_reads(k, 3)
    exact = KO.table(seqs, k)
    big = exact[0][1]
    assert exact[0][0] == 0 and 40000 <= big < 40100 and max(c for _, c in exact[1:]) < 100
    T = table_of(torch, seqs, k)
    S = T.sorted()
    held = clamped(exact)
    Ld = load(torch, held, k)
    m = S.compare_hist(Ld, 32767, 127, "a")
    assert m[32767, 127] == big                            # the exact count is what is summed, not the fold
    assert Ld.compare_hist(S, 127, 32767, "b")[127, 32767] == big and Ld.compare_hist(S, 127, 32767, "a")[127, 32767] == 32767
    check_hist(S, Ld, exact, held, shapes=((32767, 127), (8, 1000)))
    n = len(exact)
    # ranges that push paired keys into row 0 or column 0
    for rng_ in ((2, None), (None, 1), (big, big), (big + 1, None), (3, 50)):
        keys = check_hist(S, Ld, exact, held, a_range=rng_)
        assert CO.tally(keys) == S.compare(Ld, a_range=rng_) and keys[0, :].sum() > 0
        keys = check_hist(S, Ld, exact, held, b_range=rng_)
        assert CO.tally(keys) == S.compare(Ld, b_range=rng_)
    keys = check_hist(S, Ld, exact, held, a_range=(2, 40), b_range=(3, None))
    assert CO.tally(keys) == S.compare(Ld, (2, 40), (3, None)) and sum(CO.tally(keys)) < n
    for s in (S, Ld, T):
        s.close()


# ---- 4. empty operands, a == b, K < 5 ----

def test_empty_operands_and_self(torch_dev):
    torch = torch_dev
    k = 21
    x = mixed_counts(clamped(rnd_entries(random.Random(6), 300, k)), 9)
    X, E, E2 = load(torch, x, k), load(torch, [], k), load(torch, [], k)
    for A, a, B, b in ((E, [], X, x), (X, x, E, []), (E, [], E2, []), (E, [], E, [])):
        keys = check_hist(A, B, a, b, shapes=((8, 1000), (1, 1)))
        if not a and not b:
            assert not keys.any()
    for xmax, ymax in ((8, 1000), (300, 5)):
        for w in WEIGHTS:
            m = X.compare_hist(X, xmax, ymax, w)
            assert np.array_equal(m, CO.matrix(x, x, xmax, ymax, w))
            on = {(min(c, xmax), min(c, ymax)) for _, c in x}
            assert {tuple(p) for p in np.argwhere(m).tolist()} == on
    for s in (X, E, E2):
        s.close()


def test_below_five(torch_dev):
    torch = torch_dev
    x, y = [b"ACGTTGCA", b"AAAA", b"GGNCC"], [b"ACGTT", b"TTTTT", b"CCGGA"]
    TX, TY = table_of(torch, x, 3), table_of(torch, y, 3)
    sx, sy = TX.sorted(), TY.sorted()
    check_hist(sx, sy, KO.table(x, 3), KO.table(y, 3), shapes=((2, 2), (8, 1000)))
    for s in (sx, sy, TX, TY):
        s.close()


# ---- 5. identities ----

@pytest.mark.parametrize("k", [13, 40])
def test_identities(torch_dev, k):
    torch = torch_dev
    X, Y = mixed_reads(k, 5), mixed_reads(k, 7) + mixed_reads(k, 5)[1:3] + [b"C" * (40000 + k - 1)]
    TX, TY = table_of(torch, X, k), table_of(torch, Y, k)
    A, B = TX.sorted(1), TY.sorted(1)
    xmax, ymax = 5, 40
    for ra, rb in ((None, None), ((2, None), None), (None, (None, 2)), ((1, 2), (2, 3))):
        m = A.compare_hist(B, xmax, ymax, "keys", ra, rb)
        assert (int(m[:, 0].sum()), int(m[0, :].sum()), int(m[1:, 1:].sum())) == A.compare(B, ra, rb)
    m = A.compare_hist(B, xmax, ymax)
    assert m[1:, 1:].sum() > 100 and m[0, ymax] >= 1
    h = B.hist()[4]
    fold = np.concatenate([h[:ymax - 1], [h[ymax - 1:].sum()]])
    assert np.array_equal(m[:, 1:].sum(axis=0), fold)      # the y margin is B's histogram folded at ymax
    ha = A.hist()
    wa = A.compare_hist(B, xmax, ymax, "a")
    assert int(wa.sum()) == int((np.arange(1, 32767) * ha[4][:32766]).sum()) + ha[3]
    hb = B.hist()
    assert hb[3] >= 40000                                  # B holds a count past the clamp: the sum is over exact counts
    assert int(A.compare_hist(B, xmax, ymax, "b").sum()) == int((np.arange(1, 32767) * hb[4][:32766]).sum()) + hb[3]
    for w, wt in (("keys", "keys"), ("a", "b"), ("b", "a")):
        for ra, rb in ((None, None), ((2, None), (None, 3))):
            assert np.array_equal(B.compare_hist(A, ymax, xmax, wt, rb, ra), A.compare_hist(B, xmax, ymax, w, ra, rb).T)
    for s in (A, B, TX, TY):
        s.close()


# ---- 6. the knobs change nothing ----

def test_grid_and_on_chip_knobs(torch_dev, tile, monkeypatch):
    """Seven tiles and more: one block takes all of them, three blocks two or three each, and every cell straight to
    device memory gives the same matrices."""
    torch = torch_dev
    k = 32
    rng = random.Random(11)
    a = mixed_counts(clamped(rnd_entries(rng, 3 * tile + 5, k)), 5)
    b = mixed_counts(clamped(rnd_entries(rng, 3 * tile + 40, k)), 9)
    b = sorted(dict(b + [(x, 1 + c % 4) for x, c in a[::3]]).items())
    assert (len(a) + len(b)) // tile >= 6
    A, B = load(torch, a, k), load(torch, b, k)
    for env in ({}, {"CLASSPRO_CMP_GRID": "1"}, {"CLASSPRO_CMP_GRID": "3"}, {"CLASSPRO_CMP_LDS": "0"},
                {"CLASSPRO_CMP_GRID": "2", "CLASSPRO_CMP_LDS": "0"}, {"CLASSPRO_CMP_GRID": "0"}, {"CLASSPRO_CMP_GRID": "1000000"}):
        monkeypatch.delenv("CLASSPRO_CMP_GRID", raising=False)
        monkeypatch.delenv("CLASSPRO_CMP_LDS", raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        check_hist(A, B, a, b, shapes=((8, 1000), (300, 300), (3, 5)))
    A.close()
    B.close()


# ---- 7. operands are only read ----

def test_operands_are_only_read(torch_dev, tile):
    torch = torch_dev
    k = 32
    rng = random.Random(8)
    a, b = clamped(rnd_entries(rng, tile + 50, k)), clamped(rnd_entries(rng, tile + 90, k))
    b = sorted(set(b) | set(a[::3]))
    A, B = load(torch, a, k), load(torch, b, k)
    before = [(s.ktab()[0].clone(), s.ktab()[1].clone()) for s in (A, B)]
    for w in WEIGHTS:
        A.compare_hist(B, 8, 1000, w)
        A.compare_hist(A, 300, 300, w)
    torch.cuda.synchronize()
    for s, (rec, idx) in zip((A, B), before):
        rec1, idx1 = s.ktab()
        assert torch.equal(rec, rec1) and torch.equal(idx, idx1)
    A.close()
    B.close()


# ---- 8. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    k = 21
    a = clamped(rnd_entries(random.Random(9), 500, k))
    A, B, A13 = load(torch, a, k), load(torch, a[::2], k), load(torch, [(5, 1)], 13)
    half = C.c_void_p()                                    # between load_begin and load_end
    assert L.cp_kmer_sorted_load_begin(k, KO.index(a, k).ctypes.data, C.byref(half)) == 0
    mat = np.full(1 << 22, -7, np.int64)
    call = lambda x, y, rng=None, w=0, xmax=8, ymax=1000, m=mat.ctypes.data: L.cp_kmer_sorted_compare_hist(x, y, rng, w, xmax, ymax, m, None)
    r4 = lambda *v: (C.c_int64 * 4)(*v)
    bad = [call(None, B.s), call(A.s, None), call(A.s, B.s, m=None), call(half, B.s), call(A.s, half), call(A.s, A13.s),
           call(A13.s, A.s), call(A.s, B.s, rng=r4(0, 5, 1, 5)), call(A.s, B.s, rng=r4(1, 5, 0, 5)),
           call(A.s, B.s, rng=r4(5, 4, 1, 5)), call(A.s, B.s, rng=r4(1, 5, 7, 6)), call(A.s, B.s, w=-1), call(A.s, B.s, w=3),
           call(A.s, B.s, xmax=0), call(A.s, B.s, ymax=0), call(A.s, B.s, xmax=-1), call(A.s, B.s, xmax=32768, ymax=1),
           call(A.s, B.s, xmax=1, ymax=32768), call(A.s, B.s, xmax=2047, ymax=2048), call(A.s, B.s, xmax=32767, ymax=32767)]
    assert bad == [EINVAL] * len(bad)
    assert bool((mat == -7).all())                         # nothing was written
    L.cp_kmer_sorted_destroy(half)
    assert call(A.s, B.s, xmax=2047, ymax=2047) == 0       # exactly 2^22 cells
    assert np.array_equal(mat.reshape(2048, 2048), CO.matrix(a, a[::2], 2047, 2047))
    for kw in ({"weight": "sum"}, {"weight": 0}, {"xmax": 0}, {"ymax": 40000}, {"xmax": 4000, "ymax": 4000}):
        with pytest.raises(ValueError):
            A.compare_hist(B, **kw)
    with pytest.raises(ValueError):
        A.compare_hist(A13)
    check_hist(A, B, a, a[::2])                            # the library is as usable as before
    for s in (A, B, A13):
        s.close()
    with pytest.raises(ValueError):
        A.compare_hist(B)                                  # closed


# ---- 9. scale against torch ----

def table_21(torch, keys, cnt):
    """A loaded snapshot of sorted distinct 42-bit keys (K = 21) with counts below 32768, records made by torch."""
    from classpro_amd.api import SortedKmers
    left = keys << 6
    rec = torch.empty((keys.numel(), 5), dtype=torch.uint8, device=keys.device)
    for b in range(3):
        rec[:, b] = ((left >> (8 * (2 - b))) & 255).to(torch.uint8)
    rec[:, 3] = (cnt & 255).to(torch.uint8)
    rec[:, 4] = (cnt >> 8).to(torch.uint8)
    index = torch.cumsum(torch.bincount(keys >> 18, minlength=1 << 24), 0)
    return SortedKmers.from_records(21, index, rec.reshape(-1), piece=1 << 20)


def test_millions_of_keys_against_torch(torch_dev):
    """K = 21: 2 M random keys per side that share a quarter, most counts low and a tail up to 32767; every weight and
    two shapes against a scatter-add of torch, with the default grid (every block takes several tiles)."""
    torch = torch_dev
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(210)
    pool = torch.unique(torch.randint(0, 1 << 42, (3_700_000,), device=dev, generator=g))
    pool = pool[torch.randperm(pool.numel(), device=dev, generator=g)[:3_500_000]]
    ka, kb = pool[:2_000_000].sort()[0], pool[1_500_000:].sort()[0]        # 0.5 M shared

    def counts(n):
        low = torch.randint(1, 4, (n,), device=dev, generator=g)
        mid = torch.randint(1, 400, (n,), device=dev, generator=g)
        top = torch.randint(1, 32768, (n,), device=dev, generator=g)
        pick = torch.rand(n, device=dev, generator=g)
        return torch.where(pick < 0.7, low, torch.where(pick < 0.97, mid, top))

    ca, cb = counts(ka.numel()), counts(kb.numel())
    A, B = table_21(torch, ka, ca), table_21(torch, kb, cb)
    assert torch.equal(A.lo, ka) and torch.equal(B.counts, cb)
    union = torch.unique(torch.cat([ka, kb]))
    sa = torch.zeros_like(union).scatter_add_(0, torch.searchsorted(union, ka), ca)
    sb = torch.zeros_like(union).scatter_add_(0, torch.searchsorted(union, kb), cb)
    for xmax, ymax in ((8, 1000), (300, 300)):
        cell = sa.clamp(max=xmax) * (ymax + 1) + sb.clamp(max=ymax)
        for w, v in (("keys", torch.ones_like(sa)), ("a", sa), ("b", sb)):
            want = torch.zeros((xmax + 1) * (ymax + 1), dtype=torch.int64, device=dev).scatter_add_(0, cell, v)
            got = A.compare_hist(B, xmax, ymax, w)
            assert np.array_equal(got.reshape(-1), want.cpu().numpy()), (xmax, ymax, w)
    A.close()
    B.close()

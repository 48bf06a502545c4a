"""The heterozygous pairs of a sorted snapshot (cp_kmer_sorted_het_pairs; SortedKmers.het_pairs) on a real MI355X
(`-m gpu`), against the set restatement of tests/hetpairs_oracle.py: the complete canonical sets of small K, planted sparse
tables with the centre inside, at the edge of and behind the prefix bytes and on the word boundary of the key, families and
the even-K chain, sizes around a tile, counts at the fold and past the record's clamp, ranges, empty and single-key tables,
both modes, the result snapshot, the two knobs, that the operand is only read, the argument checks, and millions of keys against
torch.  Everything is integers: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import hetpairs_oracle as HO
import ktab_oracle as KO
from test_gpu_ktab import table_of
from test_gpu_setop import check as check_snapshot
from test_gpu_tabprof import i64, load

pytestmark = pytest.mark.gpu
EINVAL = -1
SHAPES = ((1000, 1000), (3, 5))


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


def check_het(torch, S, ents, K, shapes=SHAPES, count_range=None, modes=(True, False), table=True):
    """S.het_pairs against the oracle over the entries: matrix, tally, degrees entry by entry and the result's keys,
    counts, records and index, in both modes.  Returns the tally of the last mode."""
    deg_want = HO.degrees(ents, K, count_range)
    t = None
    for unique in modes:
        want_t = HO.tally(ents, K, count_range, unique)
        mem = HO.members(ents, K, count_range, unique)
        for n, (xmax, ymax) in enumerate(shapes):
            want = HO.matrix(ents, K, xmax, ymax, count_range, unique)
            res = S.het_pairs(xmax, ymax, unique, count_range, degrees=True, table=table and n == 0)
            mat, t, deg = res[:3]
            assert mat.shape == want.shape and mat.dtype == np.int64
            assert np.array_equal(mat, want), (K, unique, xmax, ymax, np.argwhere(mat != want)[:5].tolist())
            assert not mat[0, :].any() and not mat[:, 0].any()
            assert t == want_t, (K, unique)
            assert deg.dtype == torch.uint8 and deg.cpu().tolist() == deg_want, (K, unique)
            assert int(mat.sum()) == (t["unique"] if unique else t["pairs"]) and 2 * t["pairs"] == sum(deg_want)
            if table and n == 0:
                R = res[3]
                check_snapshot(torch, R, mem, K)
                if mem:
                    hi, lo, _ = KO.hi_lo_cnt(mem)
                    assert R.find(i64(torch, hi), i64(torch, lo)).tolist() == list(range(len(mem)))
                R.close()
        m2, t2 = S.het_pairs(8, 8, unique, count_range)    # the matrix alone: no degrees kept, nothing built
        assert t2 == want_t and np.array_equal(m2, HO.matrix(ents, K, 8, 8, count_range, unique))
    return t


def with_counts(keys, seed, top=30):
    rng = random.Random(seed)
    return [(x, rng.randint(1, top)) for x in sorted(keys)]


# ---- 1. the complete canonical sets ----

@pytest.mark.parametrize("K", [5, 6, 7, 8])
def test_every_canonical_kmer(torch_dev, K, monkeypatch):
    """Every key with palindromic flanks is here, and for K < 13 partners lie in other buckets."""
    torch = torch_dev
    ents = with_counts({HO.canon(x, K) for x in range(1 << (2 * K))}, K)
    S = load(torch, ents, K)
    t = check_het(torch, S, ents, K, shapes=((1000, 1000),))
    assert t["paired"] == t["keys"] == len(ents) and (t["multi"] < t["keys"]) == (K % 2 == 1)    # palindromic flanks: one sibling
    t = check_het(torch, S, ents, K, shapes=((40, 40),), count_range=(11, 20))     # a third of the keys: all degrees occur
    assert t["unique"] > 0 and t["multi"] > 0
    monkeypatch.setenv("CLASSPRO_HET_STAGE", "1")
    check_het(torch, S, ents, K, shapes=((40, 40),), count_range=(11, 20))
    S.close()


@pytest.mark.parametrize("K", [3, 4])
def test_every_canonical_kmer_below_five(torch_dev, K):
    torch = torch_dev
    rng = random.Random(K)
    seq = bytes(rng.choice(b"ACGT") for _ in range(6000))
    ents = KO.table([seq], K)
    assert {x for x, _ in ents} == {HO.canon(x, K) for x in range(1 << (2 * K))}
    T = table_of(torch, [seq], K)
    S = T.sorted(1)
    check_het(torch, S, ents, K, shapes=((1000, 1000), (30, 40)))
    lo = sorted(c for _, c in ents)[len(ents) // 2]
    check_het(torch, S, ents, K, shapes=((1000, 1000),), count_range=(lo, None))
    S.close()
    T.close()


# ---- 2. planted sparse tables ----

@pytest.mark.parametrize("K", [13, 21, 24, 25, 31, 32, 40, 43, 44, 62, 63])
def test_planted_sparse_tables(torch_dev, K, monkeypatch):
    """The centre inside the three prefix bytes (13, 21, 24), at their edge (24, 25) and behind them; hi[] never loaded
    (2K - 63 <= 24: up to 43) and loaded (44, 62, 63); the substituted base across the two words of a key (62, 63)."""
    torch = torch_dev
    ents = HO.planted(random.Random(100 + K), K, 2000)
    S = load(torch, ents, K, piece=999)
    t = check_het(torch, S, ents, K)
    assert t["pairs"] > 0 and t["unique"] > 0 and t["multi"] > 0
    t = check_het(torch, S, ents, K, shapes=((1000, 1000),), count_range=(5, 25))
    assert t["pairs"] > 0 and t["unique"] > 0
    monkeypatch.setenv("CLASSPRO_HET_STAGE", "1")          # the staged form: partners inside and outside the block's tile
    check_het(torch, S, ents, K, shapes=((1000, 1000),))
    S.close()


# ---- 3. families and the even-K chain ----

def test_families_and_the_chain(torch_dev):
    torch = torch_dev
    key = lambda s: KO.key_of(s.encode())
    for K in (5, 21, 63):
        m = K // 2
        base = HO.canon(random.Random(K).getrandbits(2 * K), K)
        sub = lambda c: HO.canon((base & ~(3 << (2 * (K - 1 - m)))) | (c << (2 * (K - 1 - m))), K)
        for n in (3, 4):
            fam = sorted({sub(c) for c in range(n)})
            assert len(fam) == n
            ents = [(x, 3 + 2 * i) for i, x in enumerate(fam)]
            S = load(torch, ents, K)
            t = check_het(torch, S, ents, K)
            assert (t["pairs"], t["unique"], t["multi"], t["paired"]) == (n * (n - 1) // 2, 0, n, n)
            S.close()
    ents = [(key(s), c) for s, c in (("AAAAA", 4), ("AACAA", 9), ("AAGAA", 2))]
    S = load(torch, ents, 5)
    assert check_het(torch, S, ents, 5)["pairs"] == 3
    assert check_het(torch, S, ents, 5, count_range=(3, None))["unique"] == 1
    S.close()
    ents = [(key("ACAGT"), 7), (key("ACCGT"), 9)]          # palindromic flanks: one candidate, one unique pair
    S = load(torch, ents, 5)
    assert S.het_pairs(10, 10)[0][7, 9] == 1
    check_het(torch, S, ents, 5)
    S.close()
    seq = b"AACAAAAACAA"                                   # K = 4: AACA ~ AAAA ~ ACAA and nothing else pairs them
    T = table_of(torch, [seq], 4)
    S = T.sorted(1)
    ents = KO.table([seq], 4)
    assert {key("AACA"), key("AAAA"), key("ACAA")} <= {x for x, _ in ents}
    deg = dict(zip([x for x, _ in ents], S.het_pairs(degrees=True)[2].tolist()))
    assert deg[key("AAAA")] >= 2 and key("ACAA") not in HO.candidates(key("AACA"), 4)
    check_het(torch, S, ents, 4)
    S.close()
    T.close()


# ---- 4. sizes around a tile ----

def far_and_near(K, n, seed):
    """n entries at K = 13.  Most keys are AAAAAA followed by seven random bases: they fill one stretch of the table, and
    replacing the centre base (position 6, the first base behind that prefix) moves a key by a quarter to three quarters
    of the stretch.  The others are planted pairs under other prefixes, whose partners are their neighbours."""
    rng = random.Random(seed)
    near = {x: c for x, c in HO.planted(rng, K, 60) if x >> (2 * (K - 6))}
    pool = [x for x in range(1 << (2 * (K - 6))) if HO.canon(x, K) == x]
    keys = set(rng.sample(pool, n - len(near))) | set(near)
    assert len(keys) == n
    return with_counts(keys, seed)


@pytest.mark.parametrize("stage", ["0", "1"])
@pytest.mark.parametrize("which", [-1, 0, 1, 2])
def test_sizes_around_a_tile(torch_dev, tile, which, stage, monkeypatch):
    """tile-1, tile, tile+1 and 2*tile+1 entries, in the default form and in the staged one, which has to decide between
    the tile in LDS and the bucket search.  K = 13 (far_and_near): partners more than half the table apart -- more than a
    whole tile in the table of 2*tile+1 entries -- beside partners that are neighbours.  K = 40: every partner is among
    the next few entries."""
    torch = torch_dev
    n = 2 * tile + 1 if which == 2 else tile + which
    for K in (13, 40):
        ents = far_and_near(K, n, n) if K == 13 else HO.planted(random.Random(K * 10 + which), K, n)[:n]
        assert len(ents) == n
        pos = {x: i for i, (x, _) in enumerate(ents)}
        gaps = [abs(pos[x] - pos[y]) for x, y in HO.pairs(ents, K, unique=False)]
        if K == 13:
            assert sum(g > n // 2 for g in gaps) > 30 and sum(g < 10 for g in gaps) > 10      # n // 2 is 1023 or more
            assert which != 2 or (max(gaps) > tile and sum(g > tile for g in gaps) > 100)
        else:
            assert max(gaps) < 10
        monkeypatch.setenv("CLASSPRO_HET_STAGE", stage)
        S = load(torch, ents, K)
        t = check_het(torch, S, ents, K, shapes=((1000, 1000),))
        assert t["unique"] > 0 and t["multi"] > 0
        S.close()


# ---- 5. counts ----

def test_counts_at_the_fold(torch_dev):
    torch = torch_dev
    K = 31
    m = K // 2
    rng = random.Random(31)
    for xmax, ymax in ((8, 8), (8, 300), (63, 7), (1, 1)):
        cs = sorted({1, xmax - 1, xmax, xmax + 1, ymax - 1, ymax, ymax + 1} - {0})
        ents = {}
        for ca in cs:
            for cb in cs:
                x = HO.canon(rng.getrandbits(2 * K), K)
                ents[x] = ca
                ents[HO.canon(x ^ (1 << (2 * (K - 1 - m))), K)] = cb
        ents = sorted(ents.items())
        S = load(torch, ents, K)
        t = check_het(torch, S, ents, K, shapes=((xmax, ymax),))
        assert t["unique"] == len(cs) ** 2
        S.close()


def test_counts_past_the_clamp(torch_dev):
    """A snapshot sorted here holds exact counts: 40000 A's and 33000 of its sibling go to the last cell as they are."""
    torch = torch_dev
    K = 21
    a, b = b"A" * K, b"A" * 10 + b"C" + b"A" * 10
    seqs = [b"A" * (40000 + K - 1)] + [b] * 33000 + [a[:10] + b"G" + a[11:]] * 3
    T = table_of(torch, seqs, K)
    S = T.sorted(1)
    ents = KO.table(seqs, K)
    assert dict(ents)[0] == 40000 and dict(ents)[KO.key_of(b)] == 33000 and len(ents) == 3
    mat, t = S.het_pairs(32767, 127, unique=False)
    assert mat[32767, 127] == 1 and mat[3, 127] == 2 and t["pairs"] == 3
    check_het(torch, S, ents, K, shapes=((32767, 127), (1000, 1000)))
    t = check_het(torch, S, ents, K, shapes=((1000, 1000),), count_range=(32768, None))
    assert t == {"keys": 2, "paired": 2, "multi": 0, "pairs": 1, "unique": 1, "out": 2}
    S.close()
    T.close()


def test_ranges_change_degrees(torch_dev):
    torch = torch_dev
    K = 40
    ents = HO.planted(random.Random(7), K, 1500)
    S = load(torch, ents, K)
    seen = set()
    for rng_ in (None, (2, None), (None, 15), (10, 20), (30, 30), (31, None)):
        t = check_het(torch, S, ents, K, shapes=((40, 40),), count_range=rng_)
        seen.add((t["keys"], t["pairs"], t["unique"]))
    assert len(seen) == 6 and (0, 0, 0) in seen
    S.close()


# ---- 6. empty and single ----

def test_empty_and_single(torch_dev):
    torch = torch_dev
    for K in (13, 44):
        E = load(torch, [], K)
        t = check_het(torch, E, [], K)
        assert t == dict.fromkeys(("keys", "paired", "multi", "pairs", "unique", "out"), 0)
        E.close()
        one = [(HO.canon(12345, K), 9)]
        S = load(torch, one, K)
        t = check_het(torch, S, one, K)
        assert t["keys"] == 1 and t["paired"] == 0
        S.close()


# ---- 7. the result lives on its own; the operand is only read; the knob ----

def test_result_survives_and_operand_is_only_read(torch_dev, tile, monkeypatch):
    torch = torch_dev
    K = 32
    ents = HO.planted(random.Random(32), K, 3 * tile)
    assert len(ents) > 3 * tile
    S = load(torch, ents, K)
    rec0, idx0 = [x.clone() for x in S.ktab()]
    base = S.het_pairs(300, 300, True, None, degrees=True, table=True)
    knobs = ("CLASSPRO_HET_LDS", "CLASSPRO_HET_STAGE")
    for env in ({"CLASSPRO_HET_LDS": "0"}, {"CLASSPRO_HET_LDS": "1"}, {"CLASSPRO_HET_STAGE": "1"}, {"CLASSPRO_HET_STAGE": "0"},
                {"CLASSPRO_HET_LDS": "0", "CLASSPRO_HET_STAGE": "1"}):
        for unique in (True, False):
            for name in knobs:
                monkeypatch.delenv(name, raising=False)
            want = S.het_pairs(300, 300, unique, (2, 29), degrees=True)
            for name, v in env.items():
                monkeypatch.setenv(name, v)
            got = S.het_pairs(300, 300, unique, (2, 29), degrees=True)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and torch.equal(got[2], want[2])
    for env in ({"CLASSPRO_HET_LDS": "0"}, {"CLASSPRO_HET_STAGE": "1"}):
        for name in knobs:
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        check_het(torch, S, ents, K, shapes=((300, 300), (3, 5)))
    for name in knobs:
        monkeypatch.delenv(name, raising=False)
    torch.cuda.synchronize()
    rec1, idx1 = S.ktab()
    assert torch.equal(rec0, rec1) and torch.equal(idx0, idx1)
    S.close()
    R = base[3]
    mem = HO.members(ents, K)
    check_snapshot(torch, R, mem, K)                       # after the operand is gone
    both = R.combine(R, "and")
    assert len(both) == len(mem)
    both.close()
    R.close()


# ---- 8. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K = 21
    ents = HO.planted(random.Random(9), K, 300)
    S = load(torch, ents, K)
    half = C.c_void_p()
    assert L.cp_kmer_sorted_load_begin(K, KO.index(ents, K).ctypes.data, C.byref(half)) == 0
    mat, tal = np.full(1 << 22, -7, np.int64), np.full(6, -7, np.int64)
    r2 = lambda *v: (C.c_int64 * 2)(*v)

    def call(s, rng=None, xmax=8, ymax=8, m=mat.ctypes.data, t=tal.ctypes.data):
        return L.cp_kmer_sorted_het_pairs(s, rng, 1, xmax, ymax, m, t, None, None, None)

    bad = [call(None), call(half), call(S.s, m=None, t=None), call(S.s, rng=r2(0, 5)), call(S.s, rng=r2(5, 4)),
           call(S.s, rng=r2(-1, -1)), call(S.s, xmax=0), call(S.s, ymax=0), call(S.s, xmax=32768, ymax=1),
           call(S.s, xmax=1, ymax=32768), call(S.s, xmax=2047, ymax=2048)]
    assert bad == [EINVAL] * len(bad)
    assert bool((mat == -7).all()) and bool((tal == -7).all())
    L.cp_kmer_sorted_destroy(half)
    assert call(S.s, xmax=0, ymax=0, m=None) == 0          # the bounds are checked only with a matrix
    assert tal.tolist() == [HO.tally(ents, K)[n] for n in ("keys", "paired", "multi", "pairs", "unique", "out")]
    assert call(S.s, xmax=2047, ymax=2047) == 0            # exactly 2^22 cells
    assert np.array_equal(mat.reshape(2048, 2048), HO.matrix(ents, K, 2047, 2047))
    for kw in ({"xmax": 0}, {"ymax": 40000}, {"xmax": 4000, "ymax": 4000}):
        with pytest.raises(ValueError):
            S.het_pairs(**kw)
    check_het(torch, S, ents, K)
    S.close()
    with pytest.raises(ValueError):
        S.het_pairs()


# ---- 9. scale against torch ----

def test_millions_of_keys_against_torch(torch_dev):
    """K = 21: 3 M random canonical keys, a third with a planted partner at the centre and some with two; degrees, both
    matrices, the tally and the result against a searchsorted restatement in torch."""
    torch = torch_dev
    from test_gpu_cmphist import table_21
    dev = torch.device("cuda:0")
    K, m = 21, 10
    sh = 2 * (K - 1 - m)
    g = torch.Generator(device=dev)
    g.manual_seed(21)

    def revcomp(x):
        r = torch.zeros_like(x)
        for _ in range(K):
            r = r * 4 + 3 - (x & 3)
            x = x >> 2
        return r

    canon = lambda x: torch.minimum(x, revcomp(x))
    sub = lambda x, c: (x & ~(3 << sh)) | (c << sh)
    seeds = canon(torch.randint(0, 1 << 42, (3_000_000,), device=dev, generator=g))
    flip = lambda x: canon(x ^ (torch.randint(1, 4, (x.numel(),), device=dev, generator=g) << sh))
    keys = torch.unique(torch.cat([seeds, flip(seeds[:1_000_000]), flip(seeds[:100_000])]))
    n = keys.numel()
    low = torch.randint(1, 60, (n,), device=dev, generator=g)
    top = torch.randint(1, 32768, (n,), device=dev, generator=g)
    cnt = torch.where(torch.rand(n, device=dev, generator=g) < 0.95, low, top)
    S = table_21(torch, keys, cnt)
    assert torch.equal(S.lo, keys) and torch.equal(S.counts, cnt)
    for rng_ in (None, (3, 50)):
        live = torch.ones(n, dtype=torch.bool, device=dev) if rng_ is None else (cnt >= rng_[0]) & (cnt <= rng_[1])
        cur = (keys >> sh) & 3
        part = []                                          # per c: the partner's ordinal, or -1
        for c in range(4):
            y = canon(sub(keys, c))
            at = torch.searchsorted(keys, y).clamp(max=n - 1)
            ok = live & (cur != c) & (y != keys) & (keys[at] == y) & live[at]
            for prev in part:
                ok &= prev != at                           # a repeat of an earlier candidate
            part.append(torch.where(ok, at, torch.full_like(at, -1)))
        deg = sum((p >= 0).to(torch.int64) for p in part)
        want_t = {"keys": int(live.sum()), "paired": int((deg >= 1).sum()), "multi": int((deg >= 2).sum()),
                  "pairs": int(deg.sum()) // 2}
        for unique in (True, False):
            xmax, ymax = 300, 1000
            want = torch.zeros((xmax + 1) * (ymax + 1), dtype=torch.int64, device=dev)
            member = torch.zeros(n, dtype=torch.bool, device=dev)
            nuniq = 0
            for p in part:
                i = torch.nonzero(p >= 0).reshape(-1)
                j = p[i]
                uq = (deg[i] == 1) & (deg[j] == 1)
                nuniq += int((uq & (i < j)).sum())
                keep = uq if unique else torch.ones_like(uq)
                member[i[keep]] = True
                first = keep & (i < j)
                a, b = torch.minimum(cnt[i], cnt[j])[first], torch.maximum(cnt[i], cnt[j])[first]
                want.scatter_add_(0, a.clamp(max=xmax) * (ymax + 1) + b.clamp(max=ymax), torch.ones_like(a))
            mat, t, d, R = S.het_pairs(xmax, ymax, unique, rng_, degrees=True, table=True)
            assert torch.equal(d.to(torch.int64), deg)
            assert np.array_equal(mat.reshape(-1), want.cpu().numpy())
            assert t == dict(want_t, unique=nuniq, out=int(member.sum()))
            assert torch.equal(R.lo, keys[member]) and torch.equal(R.counts, cnt[member]) and not bool(R.hi.any())
            assert bool((R.find(R.hi, R.lo) == torch.arange(len(R), device=dev)).all())
            R.close()
        if rng_ is None:
            assert want_t["pairs"] > 900_000 and nuniq > 700_000 and want_t["multi"] > 50_000
    S.close()

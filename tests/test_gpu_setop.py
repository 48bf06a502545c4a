"""Set algebra on sorted snapshots (cp_kmer_sorted_combine, cp_kmer_sorted_hist; SortedKmers.combine, .compare, .hist) on
a real MI355X (`-m gpu`), against the dict-and-set restatement of tests/setop_oracle.py: every operator and count rule on
hand-written tables, equal pairs across tile cuts, sizes around a tile, empty operands, a dense bucket, counts past the
record's clamp and count ranges, the identities that tie it to the rest of the project, that operands are only read,
the argument checks, and millions of keys against torch.  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import ktab_oracle as KO
import setop_oracle as SO
import tabprof_oracle as TO
from test_gpu_ktab import flat, mixed_reads, table_of
from test_gpu_tabprof import hand_table, i64, load, queries

pytestmark = pytest.mark.gpu
EINVAL = -1
M63 = (1 << 63) - 1
OPS, RULES = ("and", "or", "sub", "xor"), ("left", "sum", "min", "max")


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def tile(torch_dev):
    from classpro_amd.api import ktab_tile
    t = ktab_tile()
    assert t >= 64
    return t


def index_of(torch, ents, k):
    """The prefix index of the entries as a device tensor: a bincount of the keys' top 8 * ibyte bits."""
    ib = KO.ibyte_of(k)
    pre = torch.tensor([x >> (2 * k - 8 * ib) for x, _ in ents], dtype=torch.int64, device="cuda:0")
    return torch.cumsum(torch.bincount(pre, minlength=1 << (8 * ib)), 0)


def check(torch, s, ents, k, idx=None):
    """A snapshot against the oracle's entries: keys, exact counts and, for K >= 5, records and index (`idx`: the wanted
    index as a device tensor where the caller has it already)."""
    hi, lo, cnt = KO.hi_lo_cnt(ents)
    assert len(s) == len(ents)
    assert s.hi.tolist() == hi and s.lo.tolist() == lo and s.counts.tolist() == cnt
    if k >= 5:
        rec, got = s.ktab()
        assert rec.cpu().numpy().tobytes() == KO.records_fast(ents, k)
        assert torch.equal(got, index_of(torch, ents, k) if idx is None else idx)


def check_ops(torch, A, B, a, b, k, ops=OPS, rules=("sum",), a_range=None, b_range=None, index=None):
    """A.combine(B) against the oracle over the entries a and b, for every op and rule given (`index`: how the wanted
    index is made, index_of unless given); returns the results' entries by (op, rule)."""
    out = {}
    for op in ops:
        idx = None
        for rule in rules:
            want, tally = SO.combine(a, b, op, rule, a_range, b_range)
            if idx is None and k >= 5:                     # the keys, and so the index, do not depend on the rule
                idx = (index or index_of)(torch, want, k)
            r = A.combine(B, op, rule, a_range, b_range)
            assert r.tally == tally, (op, rule)
            check(torch, r, want, k, idx)
            r.close()
            out[op, rule] = want
        assert A.compare(B, a_range, b_range) == tally[:3]
    return out


def rnd_entries(rng, n, k, lo=None, hi=None, top=60000):
    lo, hi = 0 if lo is None else lo, (1 << (2 * k)) if hi is None else hi
    keys = set()
    while len(keys) < n:
        keys.add(rng.randrange(lo, hi))
    return [(x, rng.randint(1, top)) for x in sorted(keys)]


def clamped(ents):
    """What a table loaded from records holds of these entries."""
    return [(x, min(c, KO.MAXC)) for x, c in ents]


# ---- 1. hand-written tables, every op and rule ----

@pytest.mark.parametrize("k", [5, 8, 12, 13, 21, 31, 32, 43, 44, 63])
def test_every_op_and_rule_on_hand_written_tables(torch_dev, tile, k):
    torch = torch_dev
    a, shift, nb, room = hand_table(k, tile)
    top = 1 << (2 * k)
    akeys = [x for x, _ in a]
    bkeys = set(akeys[::2])
    for x in akeys[1::3]:
        bkeys |= {y for y in (x - 1, x + 1) if 0 <= y < top}
    b = [(x, 1 + (i * 104729) % 30011) for i, x in enumerate(sorted(bkeys))]
    a = clamped(a)
    assert set(akeys) & bkeys and bkeys - set(akeys) and set(akeys) - bkeys
    if k in (21, 31, 43, 44, 63):
        assert len(a) > tile and len(a) + len(b) > 2 * tile
    if k in (44, 63):
        for ents in (a, b):
            pairs = [(x, y) for x, _ in ents for y, _ in ents if x < y and x >> shift == y >> shift == 9]
            assert any(x & M63 == y & M63 for x, y in pairs) and any(x >> 63 == y >> 63 for x, y in pairs)
    A, B = load(torch, a, k), load(torch, b, k, piece=777)
    res = check_ops(torch, A, B, a, b, k, rules=RULES, index=lambda t, ents, kk: t.from_numpy(KO.index(ents, kk)).cuda())
    for op in OPS:
        want = res[op, "left"]
        r = A.combine(B, op)
        qs = queries(want or a, k, shift, nb, room)
        got = r.find(i64(torch, [q >> 63 for q in qs]), i64(torch, [q & M63 for q in qs])).tolist()
        assert got == TO.find(want, qs)
        r.close()
    A.close()
    B.close()


# ---- 2. equal pairs across tile cuts ----

@pytest.mark.parametrize("where", ["below", "above"])
def test_pairs_across_tile_cuts(torch_dev, tile, where):
    """The partition hazard: the merged sequence is cut every `tile` entries, an A entry before the B entry of the same
    key.  With A = P + S and B = S every key of S is a pair; 0 to 3 extra keys below S shift every pair against the
    cuts, so that a cut falls inside a pair at either parity and would split it; extra keys above S leave the cuts
    where they are and end the last tile differently.  Both orders of the operands, all four ops."""
    torch = torch_dev
    k = 21
    rng = random.Random(tile)
    s = rnd_entries(rng, 3 * tile + 5, k, lo=100, hi=(1 << 42) - 100)
    s2 = [(x, 1 + c % 977) for x, c in s]
    S2 = load(torch, s2, k)
    for np_ in (0, 1, 2, 3):
        extra = [(7 * i + 3, 5 + i) for i in range(np_)] if where == "below" else [((1 << 42) - 50 + 9 * i, 5 + i) for i in range(np_)]
        ps = clamped(sorted(extra + s))
        PS = load(torch, ps, k)
        res = check_ops(torch, PS, S2, ps, s2, k)
        assert len(res["and", "sum"]) == len(s) and len(res["sub", "sum"]) == np_
        res = check_ops(torch, S2, PS, s2, ps, k)
        assert len(res["and", "sum"]) == len(s) and len(res["sub", "sum"]) == 0 and len(res["xor", "sum"]) == np_
        PS.close()
    S2.close()


# ---- 3. sizes around a tile ----

def test_sizes_around_a_tile(torch_dev, tile):
    torch = torch_dev
    k = 21
    rng = random.Random(3)
    pool = rnd_entries(rng, 2 * tile + 2, k)
    made = {}

    def part(n, which):
        if (n, which) not in made:
            r = random.Random(n * 2 + which)
            ents = clamped(sorted(r.sample(pool, n)))
            made[n, which] = (load(torch, ents, k), ents)
        return made[n, which]

    for n in (tile - 1, tile, tile + 1):
        for m in (tile - 1, tile, tile + 1):
            (A, a), (B, b) = part(n, 0), part(m, 1)
            assert {x for x, _ in a} & {x for x, _ in b}
            check_ops(torch, A, B, a, b, k)
    for s, _ in made.values():
        s.close()


def test_one_entry_against_three_tiles(torch_dev, tile):
    torch = torch_dev
    k = 21
    big = clamped(rnd_entries(random.Random(4), 3 * tile, k, lo=1000, hi=(1 << 42) - 1000))
    Big = load(torch, big, k)
    mid = (big[len(big) // 2][0] + big[len(big) // 2 + 1][0]) // 2
    assert mid not in {x for x, _ in big}
    for x in (5, mid, big[0][0], big[-1][0], big[tile - 1][0], big[tile][0], (1 << 42) - 5):
        one = [(x, 77)]
        One = load(torch, one, k)
        check_ops(torch, Big, One, big, one, k)
        check_ops(torch, One, Big, one, big, k)
        One.close()
    Big.close()


def test_disjoint_ranges_of_keys(torch_dev, tile):
    """All of A below all of B, and the reverse: every cut but one has only one side."""
    torch = torch_dev
    k = 21
    rng = random.Random(5)
    lo = clamped(rnd_entries(rng, tile + 7, k, hi=1 << 30))
    hi = clamped(rnd_entries(rng, 2 * tile + 1, k, lo=1 << 30))
    Lo, Hi = load(torch, lo, k), load(torch, hi, k)
    res = check_ops(torch, Lo, Hi, lo, hi, k)
    assert res["and", "sum"] == [] and res["or", "sum"] == lo + hi
    check_ops(torch, Hi, Lo, hi, lo, k)
    Lo.close()
    Hi.close()


# ---- 4. empty operands ----

def test_empty_operands(torch_dev):
    torch = torch_dev
    k = 21
    x = clamped(rnd_entries(random.Random(6), 300, k))
    X, E, E2 = load(torch, x, k), load(torch, [], k), load(torch, [], k)
    for A, a, B, b in ((E, [], X, x), (X, x, E, []), (E, [], E2, []), (E, [], E, [])):
        res = check_ops(torch, A, B, a, b, k, rules=RULES)
        for op in OPS:
            if res[op, "left"] == []:
                r = A.combine(B, op)
                rec, idx = r.ktab()
                assert len(r) == 0 and r.hi.numel() == 0 and rec.numel() == 0 and not bool(idx.any())
                assert r.find(i64(torch, [0]), i64(torch, [x[0][0]])).tolist() == [-1]
                r.close()
    for s in (X, E, E2):
        s.close()


# ---- 5. a dense bucket ----

def test_dense_bucket(torch_dev, tile):
    """K = 21: bucket 0 is the keys below 2^18.  Both operands hold more than a tile of them, so whole tiles lie inside
    one bucket, and both hold entries in the last bucket."""
    torch = torch_dev
    k, shift = 21, 18
    rng = random.Random(7)
    last = ((1 << 24) - 1) << shift
    a = clamped(rnd_entries(rng, tile + 300, k, hi=1 << shift) + rnd_entries(rng, 40, k, lo=last))
    b = clamped(rnd_entries(rng, 2 * tile + 11, k, hi=1 << shift) + rnd_entries(rng, 40, k, lo=last + 5))
    A, B = load(torch, a, k), load(torch, b, k)
    res = check_ops(torch, A, B, a, b, k)
    idx = KO.index(res["or", "sum"], k)
    assert idx[0] > 3 * tile and idx[1] == idx[-2] == idx[0] and idx[-1] - idx[-2] > 40
    assert len(res["and", "sum"]) > 10
    A.close()
    B.close()


# ---- 6. counts ----

def test_counts_past_the_clamp_and_ranges(torch_dev):
    torch = torch_dev
    k = 40
    seqs = [b"A" * (40000 + k - 1)] + mixed_reads(k, 3)
    exact = KO.table(seqs, k)
    big = exact[0][1]                                      # A x 40, and T x 40 with it
    assert exact[0][0] == 0 and 40000 <= big < 40100 and max(c for _, c in exact[1:]) < 100
    T = table_of(torch, seqs, k)
    S = T.sorted()
    held = clamped(exact)
    Ld = load(torch, held, k)
    check(torch, S, exact, k)
    check(torch, Ld, held, k)
    n = len(exact)
    for A, a, top, B, b in ((S, exact, big, Ld, held), (Ld, held, 32767, S, exact)):      # ranges that take or leave that entry
        for rng_, na in (((top, top), 1), ((top, None), 1), ((top + 1, None), 0), ((None, top - 1), n - 1), ((None, top), n)):
            res = check_ops(torch, A, B, a, b, k, ops=("and", "sub"), a_range=rng_)
            assert len(res["and", "sum"]) == na
            res = check_ops(torch, B, A, b, a, k, ops=("and", "xor"), b_range=rng_)
            assert len(res["and", "sum"]) == na and len(res["xor", "sum"]) == n - na
    r = S.combine(Ld, "or", "sum")                          # the sum is exact, the record clamps
    assert int(r.counts[0]) == big + 32767 and r.tally == (0, 0, n, n)
    rec, _ = r.ktab(0, 1)
    assert rec.cpu().numpy().tobytes()[-2:] == b"\xff\x7f"
    r.close()
    check_ops(torch, S, Ld, exact, held, k, rules=RULES)
    r = S.combine(S, "and", "sum")
    assert int(r.counts[0]) == 2 * big
    r.close()
    for rng_ in ((50000, None), (big + 1, 10 ** 18)):        # a range that empties one side
        res = check_ops(torch, S, Ld, exact, held, k, ops=("and", "or"), rules=RULES, a_range=rng_)
        assert res["and", "left"] == [] and res["or", "left"] == held
        assert S.compare(Ld, a_range=rng_) == (0, n, 0)
        res = check_ops(torch, Ld, S, held, exact, k, ops=("and", "or", "sub"), b_range=rng_)
        assert res["and", "sum"] == [] and res["or", "sum"] == res["sub", "sum"] == held
        assert Ld.compare(S, b_range=rng_) == (n, 0, 0)
    for s in (S, Ld, T):
        s.close()


# ---- 7. against the rest of the project ----

def same(torch, x, y, ktab=True):
    assert len(x) == len(y) and torch.equal(x.hi, y.hi) and torch.equal(x.lo, y.lo) and torch.equal(x.counts, y.counts)
    if ktab:
        (r0, i0), (r1, i1) = x.ktab(), y.ktab()
        assert torch.equal(r0, r1) and torch.equal(i0, i1)


@pytest.mark.parametrize("k", [13, 40, 63])
def test_against_the_rest_of_the_project(torch_dev, k):
    torch = torch_dev
    from classpro_amd.api import KmerTable
    X, Y = mixed_reads(k, 5), mixed_reads(k, 7) + mixed_reads(k, 5)[1:3]
    TX, TY, TXY = table_of(torch, X, k), table_of(torch, Y, k), table_of(torch, X + Y, k)
    sx, sy, sxy = TX.sorted(1), TY.sorted(1), TXY.sorted(1)
    u = sx.combine(sy, "or", "sum")
    same(torch, u, sxy)
    assert u.tally[2] > 100 and u.tally[0] > 100 and u.tally[1] > 100 and u.tally[3] == len(sxy)
    aa = sx.combine(sx, "and")
    same(torch, aa, sx)
    none = sx.combine(sx, "sub")
    assert len(none) == 0 and none.tally == (0, 0, len(sx), 0)
    for s, T in ((sx, TX), (sxy, TXY), (u, TXY)):
        got, want = s.hist(), T.hist()
        assert got[:4] == want[:4] and np.array_equal(got[4], want[4]) and got[4].sum() == len(s)
    for s in (u, aa, none, sy, sxy, TY, TXY):
        s.close()
    # the four class snapshots of a canonical label table, OR-ed together, are the snapshot of every key
    seq, off = flat(torch, X)
    labels = torch.from_numpy(np.frombuffer(b"EHDR", np.uint8)[np.random.default_rng(k).integers(0, 4, seq.numel())]).cuda()
    L = KmerTable(k, canonical=True)
    L.add_tensors(seq, off, labels)
    cls = [L.sorted(c) for c in "EHDR"]
    assert all(len(c) > 0 for c in cls)
    acc = cls[0]
    for c in cls[1:]:
        nxt = acc.combine(c, "or", "left")
        assert nxt.tally[2] == 0                            # the classes are disjoint
        acc = nxt
    whole = L.sorted()
    same(torch, acc, whole)
    same(torch, acc, sx)
    for s in cls + [acc, whole, sx, TX, L]:
        s.close()


def test_below_five(torch_dev):
    """K = 3: no .ktab, a bucket is the whole key."""
    torch = torch_dev
    x, y = [b"ACGTTGCA", b"AAAA", b"GGNCC"], [b"ACGTT", b"TTTTT", b"CCGGA"]
    TX, TY = table_of(torch, x, 3), table_of(torch, y, 3)
    sx, sy = TX.sorted(), TY.sorted()
    a, b = KO.table(x, 3), KO.table(y, 3)
    res = check_ops(torch, sx, sy, a, b, 3, rules=RULES)
    r = sx.combine(sy, "or", "sum")
    qs = list(range(64))
    assert r.find(i64(torch, [0] * 64), i64(torch, qs)).tolist() == TO.find(res["or", "sum"], qs)
    for s in (r, sx, sy, TX, TY):
        s.close()


# ---- 8. operands are only read ----

def test_operands_are_only_read(torch_dev, tile):
    torch = torch_dev
    k = 32
    rng = random.Random(8)
    a, b = clamped(rnd_entries(rng, tile + 50, k)), clamped(rnd_entries(rng, tile + 90, k))
    b = sorted(set(b) | set(a[::3]))
    A, B = load(torch, a, k), load(torch, b, k)
    before = [(s.ktab()[0].clone(), s.ktab()[1].clone(), s.hi.clone(), s.lo.clone(), s.counts.clone(), s.nbytes) for s in (A, B)]
    res = {op: A.combine(B, op, "sum") for op in OPS}
    twice = A.combine(A, "or", "sum")                       # a is b
    assert twice.tally == (0, 0, len(a), len(a))
    check(torch, twice, [(x, 2 * c) for x, c in a], k)
    assert A.compare(A) == (0, 0, len(a))
    torch.cuda.synchronize()
    for s, (rec, idx, hi, lo, cnt, nbytes) in zip((A, B), before):
        rec1, idx1 = s.ktab()
        assert torch.equal(rec, rec1) and torch.equal(idx, idx1) and s.nbytes == nbytes
        assert torch.equal(hi, s.hi) and torch.equal(lo, s.lo) and torch.equal(cnt, s.counts)
    A.close()
    B.close()
    junk = torch.full((1 << 22,), -1, dtype=torch.int64, device="cuda:0")      # something else takes the freed memory
    for op in OPS:                                         # the results have memory of their own
        check(torch, res[op], SO.combine(a, b, op, "sum")[0], k)
        res[op].close()
    twice.close()
    del junk


# ---- 9. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    k = 21
    a = clamped(rnd_entries(random.Random(9), 500, k))
    A, B, A13 = load(torch, a, k), load(torch, a[::2], k), load(torch, [(5, 1)], 13)
    half = C.c_void_p()                                    # between load_begin and load_end
    assert L.cp_kmer_sorted_load_begin(k, KO.index(a, k).ctypes.data, C.byref(half)) == 0
    out, tally = C.c_void_p(), (C.c_int64 * 4)()
    call = lambda x, y, op=0, rule=0, rng=None, t=tally, o=C.byref(out): L.cp_kmer_sorted_combine(x, y, op, rule, rng, t, None, o)
    r4 = lambda *v: (C.c_int64 * 4)(*v)
    bad = [call(None, B.s), call(A.s, None), call(A.s, B.s, t=None, o=None), call(half, B.s), call(A.s, half),
           call(A.s, A13.s), call(A13.s, A.s), call(A.s, B.s, op=-1), call(A.s, B.s, op=4), call(A.s, B.s, rule=-1),
           call(A.s, B.s, rule=4), call(A.s, B.s, rng=r4(0, 5, 1, 5)), call(A.s, B.s, rng=r4(1, 5, 0, 5)),
           call(A.s, B.s, rng=r4(5, 4, 1, 5)), call(A.s, B.s, rng=r4(1, 5, 7, 6)), call(A.s, B.s, rng=r4(-3, -1, 1, 5))]
    assert bad == [EINVAL] * len(bad) and out.value is None
    h = np.zeros(32767, np.int64)
    il, ih = C.c_int64(), C.c_int64()
    assert L.cp_kmer_sorted_hist(half, h.ctypes.data, C.byref(il), C.byref(ih)) == EINVAL
    assert L.cp_kmer_sorted_hist(None, h.ctypes.data, C.byref(il), C.byref(ih)) == EINVAL
    assert L.cp_kmer_sorted_hist(A.s, None, C.byref(il), C.byref(ih)) == EINVAL
    L.cp_kmer_sorted_destroy(half)
    for kw in ({"op": "nand"}, {"op": "AND"}, {"op": "and", "count": "avg"}, {"op": 0}):
        with pytest.raises(ValueError):
            A.combine(B, **kw)
    # out alone and tally alone are both legal; compare builds nothing and leaves the operands as they are
    assert call(A.s, B.s, op=2, t=None) == 0 and out.value
    assert L.cp_kmer_sorted_size(out) == len(a) - len(a[::2])
    L.cp_kmer_sorted_destroy(out)
    nbytes = (A.nbytes, B.nbytes)
    assert call(A.s, B.s, op=2, o=None) == 0 and list(tally) == [len(a) - len(a[::2]), 0, len(a[::2]), len(a) - len(a[::2])]
    assert A.compare(B) == (len(a) - len(a[::2]), 0, len(a[::2])) and B.compare(A, b_range=(None, None)) == (0, len(a) - len(a[::2]), len(a[::2]))
    assert (A.nbytes, B.nbytes) == nbytes
    check(torch, A, a, k)                                         # nothing was harmed
    check(torch, B, a[::2], k)
    got = A.hist()
    want = SO.hist(a)
    assert got[:4] == want[:4] and np.array_equal(got[4], want[4])
    for s in (A, B, A13):
        s.close()
    with pytest.raises(ValueError):
        A.combine(B, "and")                                # closed


# ---- 10. scale against torch ----

def table_31(torch, keys, cnt):
    """A loaded snapshot of sorted distinct 62-bit keys (K = 31) with counts below 32768, records made by torch."""
    from classpro_amd.api import SortedKmers
    n = keys.numel()
    left = keys << 2
    rec = torch.empty((n, 7), dtype=torch.uint8, device=keys.device)
    for b in range(5):
        rec[:, b] = ((left >> (8 * (4 - b))) & 255).to(torch.uint8)
    rec[:, 5] = (cnt & 255).to(torch.uint8)
    rec[:, 6] = (cnt >> 8).to(torch.uint8)
    index = torch.cumsum(torch.bincount(keys >> 38, minlength=1 << 24), 0)
    return SortedKmers.from_records(31, index, rec.reshape(-1), piece=1 << 20)


def test_millions_of_keys_against_torch(torch_dev):
    """K = 31: hi is zero and a key is an int64.  Two sets of about 3 M random keys that share about a third; the four
    ops against torch.unique / torch.isin, the summed counts against a scatter-add, the index against a bincount."""
    torch = torch_dev
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(310)
    pool = torch.unique(torch.randint(0, 1 << 62, (5_200_000,), device=dev, generator=g))
    pool = pool[torch.randperm(pool.numel(), device=dev, generator=g)[:5_000_000]]
    ka, kb = pool[:3_000_000].sort()[0], pool[2_000_000:].sort()[0]        # 1 M shared
    ca = torch.randint(1, 32768, (ka.numel(),), device=dev, generator=g)
    cb = torch.randint(1, 32768, (kb.numel(),), device=dev, generator=g)
    A, B = table_31(torch, ka, ca), table_31(torch, kb, cb)
    assert torch.equal(A.lo, ka) and torch.equal(B.counts, cb)
    union = torch.unique(torch.cat([ka, kb]))
    in_a, in_b = torch.isin(union, ka), torch.isin(union, kb)
    sa = torch.zeros_like(union).scatter_add_(0, torch.searchsorted(union, ka), ca)
    sb = torch.zeros_like(union).scatter_add_(0, torch.searchsorted(union, kb), cb)
    both = int((in_a & in_b).sum())
    assert 900_000 < both < 1_100_000
    tally = (ka.numel() - both, kb.numel() - both, both)
    assert A.compare(B) == tally
    for op, keep, rule, cnt in (("and", in_a & in_b, "left", sa), ("or", in_a | in_b, "left", torch.where(in_a, sa, sb)),
                                ("sub", in_a & ~in_b, "left", sa), ("xor", in_a ^ in_b, "left", sa + sb),
                                ("or", in_a | in_b, "sum", sa + sb), ("and", in_a & in_b, "min", torch.minimum(sa, sb)),
                                ("and", in_a & in_b, "max", torch.maximum(sa, sb))):
        r = A.combine(B, op, rule)
        want = union[keep]
        assert r.tally == tally + (want.numel(),) and len(r) == want.numel()
        assert not bool(r.hi.any()) and torch.equal(r.lo, want) and torch.equal(r.counts, cnt[keep])
        _, idx = r.ktab(0, 0)
        assert torch.equal(idx, torch.cumsum(torch.bincount(want >> 38, minlength=1 << 24), 0))
        at = r.find(torch.zeros_like(ka[::7]), ka[::7])
        assert torch.equal(at >= 0, torch.isin(ka[::7], want))
        r.close()
    A.close()
    B.close()

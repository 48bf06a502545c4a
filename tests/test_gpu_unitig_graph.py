"""The links between the unitigs of a sorted snapshot and the components of their graph (cp_kmer_sorted_unitig_links;
SortedKmers.unitigs(links=, components=)) on a real MI355X (`-m gpu`), against tests/unitig_graph_oracle.py: loff, link,
base, comp and the tally on the empty table and one key, the hand cases, closed chains, K at the prefix bytes, at the word
boundary of a key and at the largest keys, the complete canonical sets of K = 5 and 6, unitig counts around the tile of
the scan, a comb whose long component needs several label rounds, a range that cuts a unitig and a component, every
selection of outputs, that the operands are only read, the argument checks, and 1.8 million keys against a union-find
on the host.  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import ktab_oracle as KO
import unitig_graph_oracle as GO
import unitig_oracle as UO
from test_gpu_tabprof import load
from test_gpu_unitigs import circle, closed_table, mixed_graph, with_counts
from test_unitig_host import clean, key, rcs, rnd, simple

pytestmark = pytest.mark.gpu
EINVAL = -1
FIELDS = GO.TALLY


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


def check_graph(torch, S, ents, K, count_range=None):
    """S.unitigs with links and components against the oracle over the entries.  Returns (the library's link tally, the
    oracle)."""
    L = GO.Links(ents, K, count_range)
    U = S.unitigs(count_range, links=True, components=True)
    assert len(U) == L.n and U.strings() == [u[1] for u in L.utgs], (K, count_range)
    assert U.loff.dtype == U.link.dtype == U.comp.dtype == torch.int64 and U.base.dtype == torch.uint8
    assert U.loff.cpu().tolist() == L.loff(), (K, count_range)
    assert U.link.cpu().tolist() == [y for _, _, y in L.arcs], (K, count_range)
    assert U.base.cpu().tolist() == [c for _, c, _ in L.arcs], (K, count_range)
    assert U.comp.cpu().tolist() == L.comp, (K, count_range)
    assert U.links() == L.arcs
    t = dict(U.link_tally)
    assert {k: t[k] for k in FIELDS} == L.tally(), (K, count_range)
    assert t["links"] == U.tally["arcs"] - 2 * (U.tally["keys"] - U.tally["unitigs"])
    assert U.utg is None and U.at is None and U.adj is None
    U.close()
    return t, L


# ---- 1. empty and single, the hand cases ----

def test_empty_and_single(torch_dev):
    torch = torch_dev
    for K in (13, 44):
        E = load(torch, [], K)
        t, _ = check_graph(torch, E, [], K)
        assert all(t[k] == 0 for k in FIELDS) and t["rounds"] == 0
        U = E.unitigs(links=True, components=True)
        assert U.loff.tolist() == [0] and U.link.numel() == 0 and U.base.numel() == 0 and U.comp.numel() == 0 and U.links() == []
        U.close()
        E.close()
        one = [(UO.canon(12345, K), 9)]
        S = load(torch, one, K)
        t, _ = check_graph(torch, S, one, K)
        assert (t["links"], t["dead_ends"], t["isolated_unitigs"], t["components"], t["largest_bases"], t["rounds"]) == (0, 2, 1, 1, K, 0)
        S.close()


def hand_cases():
    rng = random.Random(3)
    K = 7
    while True:
        left, right = rnd(rng, 12), rnd(rng, 12)
        h1, h2 = left + "A" + right, left + "C" + right
        if len(UO.table([h1, h2], K)) == 26 and clean([h1, h2], K, 20 + K - 1):
            break
    s = simple(random.Random(5), 30, 5)
    return [("single", [(key("ACCGT"), 7)], 5), ("homopolymer", UO.table(["A" * 60], 21), 21),
            ("hairpin", UO.table(["AT" * 30], 21), 21), ("palindrome", UO.table(["AT" * 30], 20), 20),
            ("k plus one", UO.table(["ACGGTC"], 5), 5), ("bubble", UO.table([h1, h2], K), K),
            ("closed", closed_table(random.Random(5), 40, 7), 7), ("joined", UO.table([s + rcs(s)], 5), 5)]


@pytest.mark.parametrize("which", range(8))
def test_hand_cases(torch_dev, which):
    torch = torch_dev
    name, ents, K = hand_cases()[which]
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    if name == "homopolymer":
        assert L.arcs == [(0, 0, 0), (1, 3, 1)]
    if name == "hairpin":
        assert L.arcs == [(0, 3, 1), (1, 0, 0)]
    if name == "palindrome":
        assert L.arcs == [(0, 0, 2), (1, 0, 2), (2, 3, 0), (3, 3, 0)]
    if name == "bubble":
        assert (t["links"], t["components"], L.n) == (8, 1, 4)
    if name == "closed":
        assert [(x, y) for x, _, y in L.arcs] == [(0, 0), (1, 1)]
    if name == "joined":
        assert any(y == x ^ 1 for x, _, y in L.arcs)
    S.close()


# ---- 2. closed chains ----

@pytest.mark.parametrize("n", [2, 3, 64])
def test_closed_chains_alone_and_beside_paths(torch_dev, n):
    torch = torch_dev
    K = 21
    ents = closed_table(random.Random(n), n, K)
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    assert [(x, y) for x, _, y in L.arcs] == [(0, 0), (1, 1)] and (t["self"], t["components"]) == (2, 1)
    S.close()
    rng = random.Random(100 + n)
    seqs = [circle(rnd(rng, n), K), rnd(rng, 400), circle(rnd(rng, 77), K), rnd(rng, K)]
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    assert (t["self"], t["components"], t["links"]) == (4, 4, 4)
    S.close()


# ---- 3. K at the prefix bytes, at the word boundary and at the largest keys ----

@pytest.mark.parametrize("K", [13, 21, 24, 25, 31, 32, 40, 62, 63])
def test_k_at_every_boundary(torch_dev, K):
    """The end k-mer packed from bytes at every width of a key: one word, across the two words, the largest."""
    torch = torch_dev
    rng = random.Random(100 + K)
    ents = UO.table(mixed_graph(rng, K), K)
    S = load(torch, ents, K, piece=999)
    t, L = check_graph(torch, S, ents, K)
    assert t["components"] >= 6 and t["self"] >= 4 and t["links"] > 8 and t["tip_unitigs"] > 0
    t, _ = check_graph(torch, S, ents, K, (1, 1))
    assert t["dead_ends"] > 0
    S.close()


# ---- 4. the complete canonical sets ----

@pytest.mark.parametrize("K", [5, 6])
def test_every_canonical_kmer(torch_dev, K):
    """Every end has four arcs; K = 6 holds palindromes, whose two orientations carry the same arcs."""
    torch = torch_dev
    ents = with_counts({UO.canon(x, K) for x in range(1 << (2 * K))}, K)
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    assert t["links"] == 8 * len(ents) and (t["dead_ends"], t["components"]) == (0, 1)
    t, L = check_graph(torch, S, ents, K, (11, 20))
    assert t["dead_ends"] > 0 and t["components"] > 1 and t["links"] > 0
    S.close()


# ---- 5. unitig counts around the tile of the scan ----

def bubbles(rng, target, K):
    """A table whose graph has `target` unitigs: two haplotypes with b SNPs K+1 apart (3b+1 unitigs: every k-mer spans at most
    one SNP), topped up with single k-mers.  At K = 21 no two of these random K-1-mers coincide; the test asserts the count."""
    b = (target - 1) // 3
    h1 = rnd(rng, (K + 1) * b + K)
    h2 = list(h1)
    for p in range(K, len(h1) - K, K + 1):
        h2[p] = "ACGT"[("ACGT".index(h2[p]) + 1 + p % 3) % 4]
    return UO.table([h1, "".join(h2)] + [rnd(rng, K) for _ in range(target - 3 * b - 1)], K)


@pytest.mark.parametrize("which", [-1, 0, 1, 2])
def test_unitig_counts_around_a_tile(torch_dev, tile, which):
    """tile-1, tile, tile+1 and 2*tile+1 unitigs: the arc counts of twice as many oriented unitigs are scanned in chunks
    of 2*tile, so these put a unitig's two orientations on either side of every cut and one past it."""
    torch = torch_dev
    K = 21
    target = 2 * tile + 1 if which == 2 else tile + which
    ents = bubbles(random.Random(target), target, K)
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    assert L.n == target and t["links"] == 8 * ((target - 1) // 3) and t["isolated_unitigs"] == (target - 1) % 3
    S.close()


# ---- 6. a comb: one long component whose labels are in random order ----

def test_comb(torch_dev):
    """One sequence of 20 000 bases with a spur of 5 bases every 20 positions: about 2 000 unitigs in a line, numbered by
    their keys, that is in random order along the line, so that the smallest label needs several rounds to reach every
    unitig; 300 small components beside it.  ROUNDS has no upper bound here: it depends on scheduling."""
    torch = torch_dev
    K = 21
    rng = random.Random(21)
    main = rnd(rng, 20000)
    seqs = [main]
    for p in range(100, 19900, 20):
        c = "ACGT"[("ACGT".index(main[p]) + 1 + p % 3) % 4]
        seqs.append(main[p - K + 1:p] + c + rnd(rng, 4))
    seqs += [rnd(rng, K + 3) for _ in range(300)]
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    big = max(L.comp.count(c) for c in set(L.comp))
    assert big > 1900 and t["components"] >= 301 and t["rounds"] >= 1 and t["tip_unitigs"] > 900
    S.close()


# ---- 7. a range that cuts a unitig and a component in two ----

def test_a_range_cuts_a_unitig_and_a_component(torch_dev):
    """A path and a bubble, with one k-mer of the path and one of either arm seen three times: the range 1-2 cuts the path
    and both arms, and with the arms the bubble's component, in two."""
    torch = torch_dev
    K = 21
    rng = random.Random(8)
    s = simple(rng, 400, K)
    left, right = rnd(rng, 3 * K), rnd(rng, 3 * K)
    bub = [left + "A" + right, left + "G" + right]
    ents = UO.table([s] + bub + [s[200:200 + K], bub[0][3 * K - 10:4 * K - 10], bub[1][3 * K - 10:4 * K - 10]] * 2, K)
    S = load(torch, ents, K)
    t, L = check_graph(torch, S, ents, K)
    assert (L.n, t["components"], t["links"], t["dead_ends"]) == (5, 2, 8, 4)
    t, L = check_graph(torch, S, ents, K, (1, 2))
    assert (L.n, t["components"], t["links"], t["dead_ends"]) == (8, 4, 8, 10)
    t, L = check_graph(torch, S, ents, K, (3, None))       # the three k-mers alone
    assert (L.n, t["components"], t["links"], t["isolated_unitigs"]) == (3, 3, 0, 3)
    t, L = check_graph(torch, S, ents, K, (4, None))
    assert all(t[k] == 0 for k in FIELDS)
    S.close()


# ---- 8. every selection of outputs; the operands are only read; the result lives on its own ----

def test_output_selection_and_operands_are_only_read(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    Lb = lib()
    K = 32
    rng = random.Random(32)
    ents = UO.table(mixed_graph(rng, K) + [rnd(rng, 3000)], K)
    S = load(torch, ents, K)
    rec0, idx0 = [x.clone() for x in S.ktab()]
    for rng_ in (None, (1, 1)):
        want = GO.Links(ents, K, rng_)
        r2 = None if rng_ is None else (C.c_int64 * 2)(*rng_)
        U = S.unitigs(rng_, where=True)
        before = [x.clone() for x in (U.seq, U.off, U.kc, U.flag, U.utg, U.at)]
        args = (S.s, r2, U.u, U.utg.data_ptr(), U.at.data_ptr())
        # the tally alone, with and without components
        tal = np.full(8, -7, np.int64)
        assert Lb.cp_kmer_sorted_unitig_links(*args, tal.ctypes.data, 1, None, None) == 0
        assert dict(zip(FIELDS, tal[:7].tolist())) == want.tally() and tal[7] >= 1
        assert Lb.cp_kmer_sorted_unitig_links(*args, tal.ctypes.data, 0, None, None) == 0
        assert dict(zip(FIELDS, tal[:7].tolist())) == dict(want.tally(), components=0, largest_bases=0) and tal[7] == 0
        # the object alone, with and without components
        for comp in (0, 1):
            h = C.c_void_p()
            assert Lb.cp_kmer_sorted_unitig_links(*args, None, comp, None, C.byref(h)) == 0 and h.value
            assert Lb.cp_unitig_graph_links(h) == len(want.arcs)
            p = [C.c_void_p() for _ in range(4)]
            assert Lb.cp_unitig_graph_arrays(h, *[C.byref(x) for x in p]) == 0
            assert p[0].value and p[1].value and p[2].value and bool(p[3].value) == bool(comp)
            Lb.cp_unitig_graph_destroy(h)
        # through the Python surface: links without components
        V = S.unitigs(rng_, links=True)
        assert V.links() == want.arcs and V.link_tally["components"] == 0 and V.link_tally["links"] == len(want.arcs)
        with pytest.raises(ValueError):
            V.comp
        V.close()
        with pytest.raises(ValueError):
            V.loff
        W = S.unitigs(rng_, components=True, where=True, adjacency=True)
        assert W.comp.cpu().tolist() == want.comp and torch.equal(W.utg, U.utg) and torch.equal(W.at, U.at) and W.adj is not None
        W.close()
        torch.cuda.synchronize()
        after = (U.seq, U.off, U.kc, U.flag, U.utg, U.at)
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        U.close()
    with pytest.raises(ValueError):
        S.unitigs(links=True, sequences=False)
    rec1, idx1 = S.ktab()
    assert torch.equal(rec0, rec1) and torch.equal(idx0, idx1)
    want = GO.Links(ents, K)
    U = S.unitigs(links=True, components=True)
    S.close()                                              # the result lives on its own
    assert U.links() == want.arcs and U.comp.cpu().tolist() == want.comp
    U.close()
    O = load(torch, ents, K)                               # the defaults are today's
    D = O.unitigs()
    assert D.g is None and D.link_tally is None
    with pytest.raises(ValueError):
        D.link
    D.close()
    O.close()


# ---- 9. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    Lb = lib()
    K = 21
    ents = UO.table([rnd(random.Random(9), 300)], K)
    S = load(torch, ents, K)
    other = load(torch, UO.table([rnd(random.Random(9), 300)], K + 1), K + 1)
    half = C.c_void_p()
    assert Lb.cp_kmer_sorted_load_begin(K, KO.index(ents, K).ctypes.data, C.byref(half)) == 0
    U, V = S.unitigs(where=True), other.unitigs()
    tal = np.full(8, -7, np.int64)
    r2 = lambda *v: (C.c_int64 * 2)(*v)
    h = C.c_void_p(1)
    utg, at = U.utg.data_ptr(), U.at.data_ptr()

    def call(s, rng=None, u=U.u, d_utg=utg, d_at=at, t=tal.ctypes.data, out=None):
        return Lb.cp_kmer_sorted_unitig_links(s, rng, u, d_utg, d_at, t, 1, None, out)

    bad = [call(None), call(S.s, u=None), call(S.s, d_utg=None), call(S.s, d_at=None), call(half), call(S.s, u=V.u),
           call(S.s, rng=r2(0, 5)), call(S.s, rng=r2(5, 4)), call(S.s, rng=r2(-1, -1)), call(S.s, t=None)]
    assert bad == [EINVAL] * len(bad)
    for kw in (dict(s=None), dict(s=half), dict(s=S.s, u=V.u), dict(s=S.s, rng=r2(5, 4)), dict(s=S.s, d_at=None)):
        h = C.c_void_p(1)
        assert call(out=C.byref(h), **kw) == EINVAL and h.value is None
        assert b"cp_kmer_sorted_unitig_links" in Lb.cp_last_error()
    assert bool((tal == -7).all())
    Lb.cp_kmer_sorted_destroy(half)
    assert call(S.s, out=C.byref(h)) == 0 and h.value
    want = GO.Links(ents, K)
    assert dict(zip(FIELDS, tal[:7].tolist())) == want.tally()
    assert Lb.cp_unitig_graph_links(h) == len(want.arcs)
    Lb.cp_unitig_graph_destroy(h)
    # where arrays that are not this call's: any arcs, no access outside the arrays
    wild = torch.randint(-5, 1 << 40, (len(ents),), dtype=torch.int64, device="cuda:0")
    assert call(S.s, d_utg=wild.data_ptr(), d_at=wild.data_ptr(), out=C.byref(h)) == 0
    p = [C.c_void_p() for _ in range(4)]
    assert Lb.cp_unitig_graph_arrays(h, *[C.byref(x) for x in p]) == 0
    assert Lb.cp_unitig_graph_links(h) == len(want.arcs)
    Lb.cp_unitig_graph_destroy(h)
    # no unitigs in range: no arrays are needed
    Z = S.unitigs((1000, None))
    assert call(S.s, rng=r2(1000, 1 << 40), u=Z.u, d_utg=None, d_at=None, out=C.byref(h)) == 0 and h.value
    assert Lb.cp_unitig_graph_links(h) == 0 and tal[:7].tolist() == [0] * 7
    assert Lb.cp_unitig_graph_arrays(h, *[C.byref(x) for x in p]) == 0 and [x.value for x in p] == [None] * 4
    Lb.cp_unitig_graph_destroy(h)
    for x in (Z, U, V, S, other):
        x.close()


# ---- 10. scale, against a union-find on the host ----

def test_two_million_keys(torch_dev):
    """K = 31, two haplotypes of a million bases that differ by a SNP every forty, 1.8 M keys and 75 000 unitigs in bubbles:
    the LINKS identity, the shape of loff, the mirror symmetry (K is odd: no palindromes) and the components against a
    union-find over the arcs that came down."""
    torch = torch_dev
    from classpro_amd.api import KmerCounts
    K, G = 31, 1_000_000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(31)
    code = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    b1 = torch.randint(0, 4, (G,), device=dev, generator=g)
    b2 = b1.clone()
    b2[20::40] = (b2[20::40] + 1 + torch.randint(0, 3, (G // 40,), device=dev, generator=g)) % 4
    seq = code[torch.cat([b1, b2])]
    off = torch.tensor([0, G, 2 * G], dtype=torch.int64, device=dev)
    T = KmerCounts(K)
    T.add_tensors(seq, off)
    S = T.sorted(1)
    assert len(S) > 1_770_000
    U = S.unitigs(links=True, components=True)
    t, lt, n = U.tally, U.link_tally, len(U)
    assert 74000 < n < 76000
    assert lt["links"] == t["arcs"] - 2 * (t["keys"] - t["unitigs"]) == U.link.numel() == U.base.numel()
    loff, link, comp = U.loff.cpu().numpy(), U.link.cpu().numpy(), U.comp.cpu().numpy()
    deg = np.diff(loff)
    assert loff[0] == 0 and loff[-1] == lt["links"] and deg.min() >= 0 and deg.max() <= 4 and len(loff) == 2 * n + 1
    assert lt["dead_ends"] == int((deg == 0).sum())
    assert 0 <= link.min() and link.max() < 2 * n and int(U.base.max()) <= 3
    x = np.repeat(np.arange(2 * n, dtype=np.int64), deg)
    fwd, mirror = x * (2 * n) + link, (link ^ 1) * (2 * n) + (x ^ 1)
    assert np.array_equal(np.sort(fwd), np.sort(mirror))
    assert lt["self"] == int(((x >> 1) == (link >> 1)).sum())
    a, b = x >> 1, link >> 1
    lab = np.arange(n, dtype=np.int64)
    while True:                                            # hook the larger root under the smaller, then flatten
        ra, rb = lab[a], lab[b]
        m = ra != rb
        if not m.any():
            break
        np.minimum.at(lab, np.maximum(ra, rb)[m], np.minimum(ra, rb)[m])
        while not np.array_equal(lab[lab], lab):
            lab = lab[lab]
    assert np.array_equal(comp[comp], comp) and bool((comp <= np.arange(n)).all()) and np.array_equal(comp[a], comp[b])
    assert np.array_equal(comp, lab)
    lens = (U.off[1:] - U.off[:-1]).cpu().numpy()
    assert lt["components"] == int((lab == np.arange(n)).sum())
    assert lt["largest_bases"] == int(np.bincount(lab, lens, n).max())
    assert lt["rounds"] >= 1
    for z in (U, S, T):
        z.close()

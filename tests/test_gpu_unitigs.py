"""The unitigs of a sorted snapshot (cp_kmer_sorted_unitigs; SortedKmers.unitigs) on a real MI355X (`-m gpu`), against
the walking restatement of tests/unitig_oracle.py: adjacency bytes, sequences, offsets, count sums, flags, the where arrays
and the tally, on the complete canonical sets of small K, single paths around every power of two, a path that needs seventeen
doublings, K at the prefix bytes, at the word boundary of a key and at the largest keys, sizes around a tile, closed chains
of every size, haplotypes with SNPs far apart and close, homopolymer and dinucleotide runs, count ranges, every selection of
outputs, that the operand is only read, the argument checks, and two million keys against the library's own counting.
Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import ktab_oracle as KO
import unitig_oracle as UO
from test_gpu_ktab import table_of
from test_gpu_tabprof import load
from test_unitig_host import clean, rcs, rnd, simple

pytestmark = pytest.mark.gpu
EINVAL = -1
FIELDS = UO.TALLY


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


def check_utg(torch, S, ents, K, count_range=None):
    """S.unitigs against the oracle over the entries: everything.  Returns (the library's tally, the oracle's unitigs)."""
    g = UO.Graph(ents, K, count_range)
    utgs, adj = g.unitigs(), g.adjacency()
    want_t = UO.tally(ents, K, count_range, utgs, adj)
    U = S.unitigs(count_range, adjacency=True, where=True)
    assert U.adj.dtype == torch.uint8 and U.adj.cpu().tolist() == adj, (K, count_range)
    assert {k: U.tally[k] for k in FIELDS} == want_t, (K, count_range)
    assert len(U) == len(utgs) and U.strings() == [u[1] for u in utgs]
    off = [0]
    for u in utgs:
        off.append(off[-1] + len(u[1]))
    assert U.off.cpu().tolist() == off and U.seq.numel() == off[-1]
    assert U.kc.cpu().tolist() == [u[3] for u in utgs]
    assert U.flag.cpu().tolist() == [int(u[2]) for u in utgs]
    utg, at = UO.where(ents, K, count_range, utgs)
    assert U.utg.cpu().tolist() == utg and U.at.cpu().tolist() == at
    t = dict(U.tally)
    U.close()
    return t, utgs


def with_counts(keys, seed, top=30):
    rng = random.Random(seed)
    return [(x, rng.randint(1, top)) for x in sorted(keys)]


def circle(s, K):
    """The closed sequence s as a string that holds each of its len(s) k-mers once."""
    reps = s * ((len(s) + K - 1) // len(s) + 1)
    return reps[:len(s) + K - 1]


# ---- 1. the complete canonical sets ----

@pytest.mark.parametrize("K", [5, 6, 7, 8])
def test_every_canonical_kmer(torch_dev, K):
    """Every node branches and even K holds palindromes; a range that keeps a third thins the graph to chains."""
    torch = torch_dev
    ents = with_counts({UO.canon(x, K) for x in range(1 << (2 * K))}, K)
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert t["unitigs"] == t["keys"] == len(ents) and t["branching"] == len(ents) and t["circular"] == 0
    t, utgs = check_utg(torch, S, ents, K, (11, 20))
    assert t["unitigs"] < t["keys"] and t["tips"] > 0 and t["branching"] > 0
    S.close()


@pytest.mark.parametrize("K", [3, 4])
def test_every_canonical_kmer_below_five(torch_dev, K):
    torch = torch_dev
    rng = random.Random(K)
    seq = rnd(rng, 6000)
    ents = UO.table([seq], K)
    assert {x for x, _ in ents} == {UO.canon(x, K) for x in range(1 << (2 * K))}
    T = table_of(torch, [seq.encode()], K)
    S = T.sorted(1)
    t, _ = check_utg(torch, S, ents, K)
    assert t["unitigs"] == len(ents)
    lo = sorted(c for _, c in ents)[len(ents) // 2]
    check_utg(torch, S, ents, K, (lo, None))
    check_utg(torch, S, ents, K, (None, lo))
    S.close()
    T.close()


# ---- 2. single paths ----

def path_table(rng, n, K):
    """The table of one random sequence whose n k-mers form one path."""
    while True:
        s = rnd(rng, n + K - 1)
        if clean([s], K, n + 1):
            return UO.table([s], K)


@pytest.mark.parametrize("r", range(12))
def test_single_paths_around_powers_of_two(torch_dev, r):
    """Paths of 2^r-1, 2^r and 2^r+1 nodes (r = 0, 1: 1, 2 and 3): the distance at which a jump round resolves a state."""
    torch = torch_dev
    K = 17
    rng = random.Random(r)
    for n in sorted({max((1 << r) - 1, 1), 1 << r, (1 << r) + 1}):
        ents = path_table(rng, n, K)
        assert len(ents) == n
        S = load(torch, ents, K)
        t, utgs = check_utg(torch, S, ents, K)
        assert t["unitigs"] == 1 and t["bases"] == n + K - 1 and t["tips"] == (2 if n > 1 else 0)
        assert t["rounds"] <= max(n - 1, 0).bit_length() + 1
        S.close()


def test_a_path_of_seventy_thousand_nodes(torch_dev):
    """2^16 < 70000 <= 2^17: seventeen doublings where every round reads only what the round before left, fewer where a
    round also meets words of its own; never more than one round beyond them."""
    torch = torch_dev
    K, n = 21, 70000
    ents = path_table(random.Random(70), n, K)
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert t["unitigs"] == 1 and t["longest"] == n + K - 1 and 1 <= t["rounds"] <= 18
    S.close()


# ---- 3. K at the prefix bytes, at the word boundary and at the largest keys ----

def mixed_graph(rng, K):
    """A path, a bubble, a closed chain, a homopolymer run inside a sequence, and a sequence joined to its reverse
    complement."""
    left, right = rnd(rng, 3 * K), rnd(rng, 3 * K)
    s = rnd(rng, 200)
    return [rnd(rng, 500), left + "A" + right, left + "G" + right, circle(rnd(rng, 70), K),
            rnd(rng, 40) + "A" * (2 * K) + rnd(rng, 40), s + rcs(s), "AC" * (2 * K)]


@pytest.mark.parametrize("K", [13, 21, 24, 25, 31, 32, 40, 62, 63])
def test_k_at_every_boundary(torch_dev, K):
    """Prefix bytes of 13, 21 and 24 bases against 25; hi[] never loaded (up to 43) and loaded; the shift by one base across
    the two words of a key (32 and above); the largest keys."""
    torch = torch_dev
    rng = random.Random(100 + K)
    ents = UO.table(mixed_graph(rng, K), K)
    S = load(torch, ents, K, piece=999)
    t, utgs = check_utg(torch, S, ents, K)
    assert t["circular"] == 2 and t["branching"] > 0 and t["tips"] > 0 and t["unitigs"] > 8     # the chain of 70 and AC
    t, _ = check_utg(torch, S, ents, K, (1, 1))
    assert t["keys"] < len(ents)
    S.close()


# ---- 4. sizes around a tile ----

@pytest.mark.parametrize("which", [-1, 0, 1, 2])
def test_sizes_around_a_tile(torch_dev, tile, which):
    """tile-1, tile, tile+1 and 2*tile+1 entries in paths of about a hundred nodes: heads on either side of every cut."""
    torch = torch_dev
    K = 21
    n = 2 * tile + 1 if which == 2 else tile + which
    rng = random.Random(n)
    sizes = [100] * (n // 100) + ([n % 100] if n % 100 else [])
    while True:
        seqs = [rnd(rng, m + K - 1) for m in sizes]
        if clean(seqs, K, n + len(sizes)):
            break
    ents = UO.table(seqs, K)
    assert len(ents) == n
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert t["unitigs"] == len(sizes) and t["isolated"] == 0
    S.close()


# ---- 5. closed chains ----

def closed_table(rng, n, K):
    while True:
        s = rnd(rng, n)
        c = circle(s, K)
        if clean([c[:n + K - 2]], K, n):
            return UO.table([c], K)


@pytest.mark.parametrize("n", [2, 3, 64, 65, 5000])
def test_closed_chains(torch_dev, n):
    torch = torch_dev
    K = 21
    ents = closed_table(random.Random(n), n, K)
    assert len(ents) == n
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert (t["unitigs"], t["circular"], t["bases"], t["tips"], t["arcs"]) == (1, 1, n + K - 1, 0, 2 * n)
    assert utgs[0][0] == 0
    S.close()


def test_closed_chains_beside_paths(torch_dev):
    torch = torch_dev
    K = 31
    rng = random.Random(6)
    seqs = [circle(rnd(rng, 300), K), circle(rnd(rng, 77), K), rnd(rng, 400), rnd(rng, 31), rnd(rng, 1500)]
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert (t["unitigs"], t["circular"]) == (5, 2)
    dup = seqs + [seqs[0][100:100 + K]]                    # one node of the first chain twice: the range opens the chain
    ents = UO.table(dup, K)
    S2 = load(torch, ents, K)
    t, _ = check_utg(torch, S2, ents, K, (1, 1))
    assert (t["unitigs"], t["circular"], t["keys"]) == (5, 1, len(ents) - 1)
    S.close()
    S2.close()


# ---- 6. haplotypes ----

def test_two_haplotypes(torch_dev):
    """SNPs farther apart than K: every one is a bubble of two arms of K nodes.  Then closer than K: the arms join."""
    torch = torch_dev
    K = 25
    rng = random.Random(25)
    h1 = rnd(rng, 3000)
    for gap in (150, 7):
        h2 = list(h1)
        for p in range(200, 2800, 200 if gap < K else gap):
            for q in ((p, p + gap) if gap < K else (p,)):
                h2[q] = "ACGT"[("ACGT".index(h2[q]) + 1 + q % 3) % 4]
        ents = UO.table([h1, "".join(h2)], K)
        S = load(torch, ents, K)
        t, utgs = check_utg(torch, S, ents, K)
        arms = [len(u[1]) - K + 1 for u in utgs if u[3] == len(u[1]) - K + 1]        # the unitigs of count 1
        assert arms and set(arms) == ({K} if gap >= K else {K + gap})
        assert t["branching"] > 10
        S.close()


# ---- 7. runs ----

@pytest.mark.parametrize("K", [20, 21])
def test_homopolymer_and_dinucleotide_runs(torch_dev, K):
    """AAAA: the node is its own successor.  ATAT: at odd K the successor is the node's own reverse complement, at even K
    the node is a palindrome.  ACAC: a closed chain of two nodes.  Alone and inside sequences."""
    torch = torch_dev
    rng = random.Random(K)
    for seqs in (["A" * 60], ["AT" * 30], ["AC" * 30], ["A" * 60, "AT" * 30, "AC" * 30, "AG" * 30, "CG" * 30, "C" * 50],
                 [rnd(rng, 50) + "A" * 50 + rnd(rng, 50), rnd(rng, 50) + "AT" * 30 + rnd(rng, 50),
                  rnd(rng, 50) + "AC" * 30 + rnd(rng, 50), rnd(rng, 50) + "CG" * 30 + rnd(rng, 50)]):
        ents = UO.table(seqs, K)
        S = load(torch, ents, K)
        t, utgs = check_utg(torch, S, ents, K)
        if seqs == ["AC" * 30]:
            assert (t["unitigs"], t["circular"], t["keys"]) == (1, 1, 2)
        if seqs in (["A" * 60], ["AT" * 30]):
            assert (t["unitigs"], t["circular"], t["isolated"]) == (len(ents), 0, 0)
        S.close()


# ---- 8. count ranges, empty and single ----

def test_a_node_out_of_range_cuts_a_unitig(torch_dev):
    torch = torch_dev
    K = 21
    s = simple(random.Random(8), 400, K)
    ents = UO.table([s, s[200:200 + K]], K)
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert t["unitigs"] == 1
    t, utgs = check_utg(torch, S, ents, K, (1, 1))
    assert t["unitigs"] == 2 and sorted(len(u[1]) for u in utgs) == sorted([200 + K - 1, 400 - K + 1 - 201 + K - 1])
    t, utgs = check_utg(torch, S, ents, K, (2, None))
    assert (t["keys"], t["unitigs"], t["isolated"]) == (1, 1, 1)
    t, utgs = check_utg(torch, S, ents, K, (3, None))      # every key out of range
    assert all(t[k] == 0 for k in FIELDS)
    U = S.unitigs((3, None))
    assert len(U) == 0 and U.seq.numel() == 0 and U.off.tolist() == [0] and U.kc.numel() == 0 and U.strings() == []
    U.close()
    S.close()


def test_empty_and_single(torch_dev):
    torch = torch_dev
    for K in (13, 44):
        E = load(torch, [], K)
        t, _ = check_utg(torch, E, [], K)
        assert all(t[k] == 0 for k in FIELDS) and t["rounds"] == 0
        E.close()
        one = [(UO.canon(12345, K), 9)]
        S = load(torch, one, K)
        t, utgs = check_utg(torch, S, one, K)
        assert (t["keys"], t["unitigs"], t["bases"], t["isolated"]) == (1, 1, K, 1) and utgs[0][3] == 9
        S.close()


# ---- 9. every selection of outputs; the operand is only read ----

def test_output_selection_and_operand_is_only_read(torch_dev, tile):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K = 32
    rng = random.Random(32)
    seqs = mixed_graph(rng, K) + [rnd(rng, 2 * tile)]
    ents = UO.table(seqs, K)
    assert len(ents) > 2 * tile
    n = len(ents)
    S = load(torch, ents, K)
    rec0, idx0 = [x.clone() for x in S.ktab()]
    for rng_ in (None, (1, 1)):
        full = S.unitigs(rng_, adjacency=True, where=True)
        strings = full.strings()
        r2 = None if rng_ is None else (C.c_int64 * 2)(*rng_)
        # the adjacency pass alone: the tally, the bytes, or both
        A = S.unitigs(rng_, adjacency=True, sequences=False)
        assert torch.equal(A.adj, full.adj) and len(A) == 0
        for k in FIELDS:
            assert A.tally[k] == (0 if k in ("unitigs", "bases", "circular", "longest") else full.tally[k])
        assert A.tally["rounds"] == 0
        B = S.unitigs(rng_, sequences=False)
        assert {k: B.tally[k] for k in FIELDS} == {k: A.tally[k] for k in FIELDS}
        adj = torch.full((n,), 77, dtype=torch.uint8, device="cuda:0")
        assert L.cp_kmer_sorted_unitigs(S.s, r2, None, adj.data_ptr(), None, None, None, None) == 0
        assert torch.equal(adj, full.adj)
        # each output of the chains alone
        for which in ("utg", "at"):
            x = torch.full((n,), 77, dtype=torch.int64, device="cuda:0")
            args = [None, None]
            args[which == "at"] = x.data_ptr()
            assert L.cp_kmer_sorted_unitigs(S.s, r2, None, None, args[0], args[1], None, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(x, getattr(full, which))
        W = S.unitigs(rng_, where=True, sequences=False)   # ranked and numbered, nothing spelled
        assert torch.equal(W.utg, full.utg) and torch.equal(W.at, full.at)
        assert {k: W.tally[k] for k in FIELDS} == {k: full.tally[k] for k in FIELDS}
        O = S.unitigs(rng_)                                # the unitigs alone
        assert O.strings() == strings and torch.equal(O.kc, full.kc) and torch.equal(O.flag, full.flag)
        assert torch.equal(O.off, full.off) and O.adj is None and O.utg is None
        for x in (full, A, B, W, O):
            x.close()
    torch.cuda.synchronize()
    rec1, idx1 = S.ktab()
    assert torch.equal(rec0, rec1) and torch.equal(idx0, idx1)
    U = S.unitigs()
    S.close()                                              # the result lives on its own
    assert len(U.strings()) == len(U) and int(U.off[-1]) == U.seq.numel()
    U.close()
    with pytest.raises(ValueError):
        S.unitigs()
    with pytest.raises(ValueError):
        U.seq


def test_long_paths_and_closed_chains_in_one_graph(torch_dev):
    """Rounds in which paths resolve while closed chains go round: nine thousand nodes beside chains of three thousand, of
    seventy and of two."""
    torch = torch_dev
    K = 24
    rng = random.Random(24)
    ents = UO.table(mixed_graph(rng, K) + [rnd(rng, 9000), circle(rnd(rng, 3000), K)], K)
    S = load(torch, ents, K)
    t, utgs = check_utg(torch, S, ents, K)
    assert t["circular"] == 3 and t["longest"] > 8000 and t["rounds"] >= 1
    check_utg(torch, S, ents, K, (1, 1))
    S.close()


# ---- 10. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K = 21
    ents = UO.table([rnd(random.Random(9), 300)], K)
    S = load(torch, ents, K)
    half = C.c_void_p()
    assert L.cp_kmer_sorted_load_begin(K, KO.index(ents, K).ctypes.data, C.byref(half)) == 0
    tal = np.full(11, -7, np.int64)
    r2 = lambda *v: (C.c_int64 * 2)(*v)
    h = C.c_void_p(1)

    def call(s, rng=None, t=tal.ctypes.data, out=None):
        return L.cp_kmer_sorted_unitigs(s, rng, t, None, None, None, None, out)

    bad = [call(None), call(half), call(S.s, t=None), call(S.s, rng=r2(0, 5)), call(S.s, rng=r2(5, 4)),
           call(S.s, rng=r2(-1, -1)), call(half, out=C.byref(h))]
    assert bad == [EINVAL] * len(bad) and h.value is None
    assert b"cp_kmer_sorted_unitigs" in L.cp_last_error()
    assert bool((tal == -7).all())
    L.cp_kmer_sorted_destroy(half)
    assert call(S.s) == 0
    want = UO.tally(ents, K)
    assert tal[:9].tolist() == [0 if k in ("unitigs", "bases", "circular", "longest") else want[k] for k in FIELDS]
    assert call(S.s, out=C.byref(h)) == 0 and h.value
    assert tal[:9].tolist() == [want[k] for k in FIELDS]
    assert L.cp_unitigs_count(h) == want["unitigs"] and L.cp_unitigs_bases(h) == want["bases"]
    L.cp_unitigs_destroy(h)
    check_utg(torch, S, ents, K)
    S.close()


# ---- 11. scale, against the library's own counting ----

def test_two_million_keys(torch_dev):
    """K = 31, two haplotypes of a million bases that differ by a SNP every forty, 1.8 M keys: the nodes of the unitigs are the in
    keys, the count sums are the counts, and counting the k-mers of the spelled unitigs gives every key of the table once."""
    torch = torch_dev
    from classpro_amd.api import KmerCounts, unitig_n50
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
    n = len(S)
    assert n > 1_770_000
    U = S.unitigs(where=True)
    t = U.tally
    assert t["keys"] == n and t["unitigs"] == len(U) and t["bases"] == U.seq.numel() == int(U.off[-1])
    lens = U.off[1:] - U.off[:-1]
    assert int((lens - (K - 1)).sum()) == n and int(lens.max()) == t["longest"]
    assert int(U.kc.sum()) == int(S.counts.sum())
    assert 74000 < len(U) < 76000 and t["circular"] == 0    # 25000 bubbles: two arms and a stretch between each
    assert unitig_n50(lens) == UO.n50(lens.tolist())
    assert bool((U.utg >= 0).all()) and int(torch.bincount(U.utg, minlength=len(U)).sub(lens - (K - 1)).abs().sum()) == 0
    T2 = KmerCounts(K)
    T2.add_tensors(U.seq, U.off)
    S2 = T2.sorted(1)
    assert S.compare(S2) == (0, 0, n) and bool((S2.counts == 1).all())
    for x in (U, S2, T2, S, T):
        x.close()

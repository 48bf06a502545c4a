"""Pruning the unitig graph (cp_kmer_sorted_unitig_prune; SortedKmers.prune and .clean) on a real MI355X (`-m gpu`), against
tests/prune_oracle.py: the marks, the tally and the keys, counts, records and index of the result on the empty table and one
key, the graphs built by hand, K at the prefix bytes, at the word boundary of a key and at the largest keys, unitig counts
around 4096 and the tile of the scan, weights near 2^62 on arms of 2 and 3 nodes and a product of 2^64, a weight that reverses the counts' choice,
a range that cuts a unitig, every selection of outputs, that the operands are only read, that the result answers find,
ktab and a second unitigs call, the argument checks, the read sets of the host test through `clean` round by round, and
about 50 000 keys from reads with errors.  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import ktab_oracle as KO
import prune_cases as PC
import prune_oracle as PR
import unitig_graph_oracle as GO
import unitig_oracle as UO
from test_gpu_setop import check
from test_gpu_tabprof import load
from test_gpu_unitig_graph import bubbles
from test_gpu_unitigs import mixed_graph
from test_unitig_host import clean, rnd, simple

pytestmark = pytest.mark.gpu
EINVAL = -1
M63 = (1 << 63) - 1


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


def check_prune(torch, S, ents, K, count_range=None, limits=(0, 0, 0), weight=None, L=None):
    """S.prune against the oracle over the entries: the marks, the tally and the result.  Returns the oracle's (out, why,
    tally)."""
    L = GO.Links(ents, K, count_range) if L is None else L
    want = PR.prune(ents, K, count_range, limits, weight, L=L)
    U = S.unitigs(count_range, where=True, links=True)
    assert len(U) == L.n
    w = None if weight is None else torch.tensor(weight, dtype=torch.int64, device="cuda:0")
    out, why, t = S.prune(U, *limits, weight=w)
    assert why.dtype == torch.uint8 and why.tolist() == want[1], (K, count_range, limits)
    assert t == want[2], (K, count_range, limits)
    check(torch, out, want[0], K)
    out.close()
    U.close()
    return want


# ---- 1. empty and single ----

def test_empty_and_single(torch_dev):
    torch = torch_dev
    for K in (13, 44):
        E = load(torch, [], K)
        _, why, t = check_prune(torch, E, [], K, None, (100, 100, 100))
        assert why == [] and all(v == 0 for v in t.values())
        out, tallies = E.clean(None, 100, 100, 100)
        assert len(out) == 0 and len(tallies) == 1
        out.close()
        E.close()
        one = [(UO.canon(12345, K), 9)]
        S = load(torch, one, K)
        assert check_prune(torch, S, one, K, None, (K - 1, 100, 100))[1] == [0]
        out, why, t = check_prune(torch, S, one, K, None, (K, 0, 0))
        assert (out, why, t["islands"], t["removed_keys"], t["removed_bases"], t["kept_keys"]) == ([], [1], 1, 1, K, 0)
        assert check_prune(torch, S, one, K, (10, None), (K, 0, 0))[0] == []          # no unitig in range: nothing in the result
        S.close()


# ---- 2. the graphs built by hand ----

@pytest.mark.parametrize("which", range(len(PC.hand_cases())))
def test_hand_cases(torch_dev, which):
    torch = torch_dev
    name, seqs, K, limits, expect = PC.hand_cases()[which]
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    L = GO.Links(ents, K)
    _, why, _ = check_prune(torch, S, ents, K, None, limits, L=L)
    assert why == PC.expected_why(L.utgs, expect), name
    S.close()


@pytest.mark.parametrize("which", range(4))
def test_nothing_goes_at_self_arcs_and_palindromes(torch_dev, which):
    torch = torch_dev
    name, ents, K = PC.quiet_cases()[which]
    S = load(torch, ents, K)
    out, why, _ = check_prune(torch, S, ents, K, None, (1000, 1000, 1000))
    assert out == ents and not any(why), name
    S.close()


def test_each_limit_at_zero(torch_dev):
    torch = torch_dev
    seqs, K, expect = PC.limit_case()
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    L = GO.Links(ents, K)
    assert not any(check_prune(torch, S, ents, K, None, (0, 0, 0), L=L)[1])
    for r in range(3):
        limits = [0, 0, 0]
        limits[r] = 2 * K
        assert check_prune(torch, S, ents, K, None, tuple(limits), L=L)[1] == PC.expected_why(L.utgs, expect[r])
    assert sum(w != 0 for w in check_prune(torch, S, ents, K, None, (2 * K, 2 * K, 2 * K), L=L)[1]) == 3
    S.close()


# ---- 3. K at the prefix bytes, at the word boundary and at the largest keys ----

@pytest.mark.parametrize("K", [13, 21, 24, 25, 31, 32, 40, 62, 63])
def test_k_at_every_boundary(torch_dev, K):
    """The result's keys, records and bucket starts at every width of a key, hi[] not loaded (2K <= 63) and loaded."""
    torch = torch_dev
    rng = random.Random(200 + K)
    seqs = mixed_graph(rng, K)
    tip = seqs[0][250 - K + 1:250] + PC.other(seqs[0][250]) + rnd(rng, 3)
    ents = UO.table(seqs + [seqs[1], tip, rnd(rng, K + 2)], K)
    S = load(torch, ents, K, piece=999)
    _, why, t = check_prune(torch, S, ents, K, None, (K + 2, 2 * K, 2 * K - 1))
    assert t["islands"] >= 1 and t["tips"] >= 1 and t["bubbles"] >= 1
    check_prune(torch, S, ents, K, (1, 1), (3 * K, 3 * K, 3 * K))
    S.close()


# ---- 4. unitig counts around 4096 and the tile of the scan ----

@pytest.mark.parametrize("which", range(6))
def test_unitig_counts_around_the_cuts(torch_dev, tile, which):
    """tile-1, tile, tile+1, 4095, 4096 and 4097 unitigs in a chain of bubbles topped up with single k-mers: every bubble
    loses an arm and every single k-mer goes, so the kept entries of every tile of the compaction are fewer than its entries."""
    torch = torch_dev
    K = 21
    target = [tile - 1, tile, tile + 1, 4095, 4096, 4097][which]
    ents = bubbles(random.Random(target), target, K)
    S = load(torch, ents, K)
    _, why, t = check_prune(torch, S, ents, K, None, (K, 0, 2 * K - 1))
    assert t["unitigs"] == target and t["bubbles"] == (target - 1) // 3 and t["islands"] == (target - 1) % 3
    S.close()


# ---- 5. weights ----

def run_bubble(K=13, small=2):
    """Two haplotypes that differ by one base of a run of A: arms of small+1 and of small nodes.  (h1, h2)"""
    rng = random.Random(62)
    for _ in range(100):
        left, right = rnd(rng, 3 * K, "CGT"), rnd(rng, 3 * K, "CGT")
        h1, h2 = left + "A" * (K - 1 - small) + right, left + "A" * (K - small) + right
        L = GO.Links(UO.table([h1, h2], K), K)
        if L.n == 4 and sorted(len(u[1]) - K + 1 for u in L.utgs)[:2] == [small, small + 1]:
            return h1, h2
    raise AssertionError("no such pair of haplotypes")


def test_weights_near_2_62_on_arms_of_two_and_three_nodes(torch_dev):
    """w = 2^62 on the arm of 2 nodes, 2^62 - 5 on the arm of 3: 3 * 2^62 against 2 * (2^62 - 5).  The first product does not
    fit a signed 64-bit integer; taken so, it is negative and the other arm goes."""
    torch = torch_dev
    K = 13
    ents = UO.table(run_bubble(K), K)
    L = GO.Links(ents, K)
    nodes = [len(u[1]) - K + 1 for u in L.utgs]
    two, three = nodes.index(2), nodes.index(3)
    weight = [1 << 61] * L.n
    weight[two], weight[three] = 1 << 62, (1 << 62) - 5
    S = load(torch, ents, K)
    _, why, t = check_prune(torch, S, ents, K, None, (0, 0, 3 * K), weight, L=L)
    assert why[three] == 3 and why[two] == 0 and t["bubbles"] == 1 and t["removed_keys"] == 3
    signed = lambda v: (v + (1 << 63)) % (1 << 64) - (1 << 63)
    assert signed(weight[two] * 3) < signed(weight[three] * 2)                # what a 64-bit product would have seen
    weight[two], weight[three] = 1 << 61, 1 << 62                            # the other way round: the arm of 2 nodes goes
    _, why, _ = check_prune(torch, S, ents, K, None, (0, 0, 3 * K), weight, L=L)
    assert why[two] == 3 and why[three] == 0
    weight[two], weight[three] = 2 << 60, 3 << 60                            # equal means: the larger ordinal goes
    _, why, _ = check_prune(torch, S, ents, K, None, (0, 0, 3 * K), weight, L=L)
    assert why[max(two, three)] == 3 and why[min(two, three)] == 0
    S.close()


def test_a_product_of_2_64(torch_dev):
    """w = 2^62 on both arms, of 3 and of 4 nodes: 4 * 2^62 = 2^64 against 3 * 2^62.  The arm of 4 nodes has the lower mean and
    goes; with products taken in 64 bits, signed or not, the first is 0 and the arm of 3 nodes would go instead."""
    torch = torch_dev
    K = 13
    ents = UO.table(run_bubble(K, 3), K)
    L = GO.Links(ents, K)
    nodes = [len(u[1]) - K + 1 for u in L.utgs]
    three, four = nodes.index(3), nodes.index(4)
    weight = [1 << 61] * L.n
    weight[three] = weight[four] = 1 << 62
    S = load(torch, ents, K)
    _, why, t = check_prune(torch, S, ents, K, None, (0, 0, 3 * K), weight, L=L)
    assert why[four] == 3 and why[three] == 0 and t["removed_keys"] == 4
    assert (weight[three] * 4) % (1 << 64) < (weight[four] * 3) % (1 << 64)   # what a 64-bit product would have seen
    narrow = PR.rule_of(L, (0, 0, 3 * K), weight)
    narrow.mul = lambda a, b: (a * b) % (1 << 64)
    assert narrow.all()[three] == 3 and narrow.all()[four] == 0
    S.close()


def test_a_weight_reverses_the_counts(torch_dev):
    torch = torch_dev
    name, seqs, K, limits, expect = PC.hand_cases()[5]
    assert name == "bubble, unequal counts"
    ents = UO.table(seqs, K)
    L = GO.Links(ents, K)
    S = load(torch, ents, K)
    by_count = check_prune(torch, S, ents, K, None, limits, L=L)[1]
    top = max(u[3] for u in L.utgs)
    by_weight = check_prune(torch, S, ents, K, None, limits, [top + 1 - u[3] for u in L.utgs], L=L)[1]
    assert sum(by_count) == sum(by_weight) == 3 and by_count != by_weight
    negative = check_prune(torch, S, ents, K, None, limits, [-5] * L.n, L=L)[1]            # all count as 0: the ordinal decides
    assert sum(negative) == 3
    S.close()


# ---- 6. a range that cuts a unitig ----

def test_a_range_cuts_a_unitig(torch_dev):
    """A path with one k-mer seen three times, and a tip on it: the range 1-2 cuts the path in two, the k-mer out of range is
    not in the result, and one half is now short enough to be a tip candidate."""
    torch = torch_dev
    K = 21
    rng = random.Random(8)
    while True:
        s = simple(rng, 400, K)
        tip = s[300 - K + 1:300] + PC.other(s[300]) + rnd(rng, 5)
        if clean([s, tip], K, 400 - K + 2 + 6):
            break
    ents = UO.table([s, tip] + [s[30:30 + K]] * 2, K)
    S = load(torch, ents, K)
    out, why, t = check_prune(torch, S, ents, K, None, (0, 2 * K, 0))
    assert (t["unitigs"], t["tips"], t["kept_keys"]) == (3, 1, len(ents) - 6)
    out, why, t = check_prune(torch, S, ents, K, (1, 2), (0, 2 * K, 0))
    cut = UO.canon(UO.key_of(s[30:30 + K]), K)
    assert t["unitigs"] == 4 and t["tips"] == 1 and cut not in {x for x, _ in out}
    assert t["kept_keys"] + t["removed_keys"] == len(ents) - 1 and t["kept_keys"] == len(out) == len(ents) - 7
    out, why, t = check_prune(torch, S, ents, K, (3, None), (K, 0, 0))                   # that k-mer alone: an island
    assert (out, why, t["kept_keys"], t["removed_keys"]) == ([], [1], 0, 1)
    S.close()


# ---- 7. every selection of outputs; the operands are only read; the result lives on its own ----

def test_output_selection_and_operands_are_only_read(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    from classpro_amd.api import SortedKmers
    Lb = lib()
    K = 32
    rng = random.Random(32)
    seqs = mixed_graph(rng, K)
    tip = seqs[0][250 - K + 1:250] + PC.other(seqs[0][250]) + rnd(rng, 3)
    ents = UO.table(seqs + [seqs[1], tip, rnd(rng, K + 2), rnd(rng, 3000)], K)
    S = load(torch, ents, K)
    rec0, idx0 = [x.clone() for x in S.ktab()]
    limits = (K + 2, 2 * K, 2 * K - 1)
    lim = (C.c_int64 * 3)(*limits)
    for rng_ in (None, (1, 1)):
        want_out, want_why, want_t = PR.prune(ents, K, rng_, limits)
        U = S.unitigs(rng_, where=True, links=True)
        wt = U.kc.clone() + 1
        views = lambda: (U.seq, U.off, U.kc, U.flag, U.utg, U.at, U.loff, U.link, U.base, wt)
        before = [x.clone() for x in views()]
        args = (S.s, U.u, U.utg.data_ptr(), U.g)
        why = torch.full((len(U),), 9, dtype=torch.uint8, device="cuda:0")
        tal = np.full(7, -7, np.int64)
        assert Lb.cp_kmer_sorted_unitig_prune(*args, None, lim, why.data_ptr(), None, None, None) == 0       # the marks alone
        assert why.tolist() == want_why
        assert Lb.cp_kmer_sorted_unitig_prune(*args, None, lim, None, tal.ctypes.data, None, None) == 0      # the tally alone
        assert dict(zip(PR.TALLY, tal.tolist())) == want_t
        h = C.c_void_p()
        assert Lb.cp_kmer_sorted_unitig_prune(*args, None, lim, None, None, None, C.byref(h)) == 0 and h.value       # the table alone
        out = SortedKmers.__new__(SortedKmers)
        out.L, out.device, out.K = S.L, S.device, K
        out._adopt(h)
        check(torch, out, want_out, K)
        out.close()
        none, why2, t2 = S.prune(U, *limits, weight=wt, table=False)                   # through the Python surface, no table
        assert none is None and t2 == PR.prune(ents, K, rng_, limits, [u[3] + 1 for u in GO.Links(ents, K, rng_).utgs])[2]
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, views()))
        U.close()
    rec1, idx1 = S.ktab()
    assert torch.equal(rec0, rec1) and torch.equal(idx0, idx1)
    U = S.unitigs(where=True, links=True)
    out, why, t = S.prune(U, *limits)
    U.close()
    S.close()                                              # the result lives on its own
    check(torch, out, PR.prune(ents, K, None, limits)[0], K)
    out.close()


# ---- 8. the result answers find, ktab and a second unitigs call ----

def test_the_result_is_an_ordinary_table(torch_dev):
    torch = torch_dev
    K = 21
    g, seqs = PC.read_set(3, K, False)
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    out, why, t = S.prune(U, 0, 2 * K, 2 * K - 1)
    want = PR.prune(ents, K, None, (0, 2 * K, 2 * K - 1))[0]
    assert 0 < t["removed_keys"] and len(want) == t["kept_keys"]
    check(torch, out, want, K)                             # ktab: records and index
    place = {x: i for i, (x, _) in enumerate(want)}
    qs = [x for x, _ in ents] + [UO.canon(7, K)]
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")
    assert out.find(i64([q >> 63 for q in qs]), i64([q & M63 for q in qs])).tolist() == [place.get(q, -1) for q in qs]
    V = out.unitigs(links=True)
    L = GO.Links(want, K)
    assert V.strings() == [u[1] for u in L.utgs] and V.links() == L.arcs and V.kc.tolist() == [u[3] for u in L.utgs]
    assert out.compare(S) == (0, len(ents) - len(want), len(want)) and out.hist()[4].sum() == len(want)
    for x in (V, U, out, S):
        x.close()


# ---- 9. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    Lb = lib()
    K = 21
    rng = random.Random(9)
    ents = UO.table(mixed_graph(rng, K), K)
    S = load(torch, ents, K)
    other = load(torch, UO.table([rnd(rng, 300)], K + 1), K + 1)
    small = load(torch, UO.table([rnd(rng, 300)], K), K)
    half = C.c_void_p()
    assert Lb.cp_kmer_sorted_load_begin(K, KO.index(ents, K).ctypes.data, C.byref(half)) == 0
    U, V, W = S.unitigs(where=True, links=True), other.unitigs(where=True, links=True), small.unitigs(where=True, links=True)
    tal = np.full(7, -7, np.int64)
    l3 = lambda *v: (C.c_int64 * 3)(*v)

    def call(s, u=U.u, d_utg=U.utg.data_ptr(), g=U.g, lim=l3(K, K, K), why=None, t=tal.ctypes.data, out=None):
        return Lb.cp_kmer_sorted_unitig_prune(s, u, d_utg, g, None, lim, why, t, None, out)

    bad = [call(None), call(S.s, u=None), call(S.s, g=None), call(S.s, lim=None), call(half), call(S.s, u=V.u), call(S.s, d_utg=None),
           call(S.s, lim=l3(-1, 0, 0)), call(S.s, lim=l3(0, -1, 0)), call(S.s, lim=l3(0, 0, -7)), call(S.s, t=None), call(S.s, g=W.g)]
    assert bad == [EINVAL] * len(bad)
    for kw in (dict(s=None), dict(s=half), dict(s=S.s, u=V.u), dict(s=S.s, lim=l3(0, -1, 0)), dict(s=S.s, d_utg=None)):
        h = C.c_void_p(1)
        assert call(out=C.byref(h), **kw) == EINVAL and h.value is None
        assert b"cp_kmer_sorted_unitig_prune" in Lb.cp_last_error()
    assert bool((tal == -7).all())
    Lb.cp_kmer_sorted_destroy(half)
    assert call(S.s) == 0 and dict(zip(PR.TALLY, tal.tolist())) == PR.prune(ents, K, None, (K, K, K))[2]
    # a where array and weights that are not this call's: any marks, no access outside the arrays
    wild = torch.randint(-5, 1 << 40, (len(ents),), dtype=torch.int64, device="cuda:0")
    h = C.c_void_p()
    assert call(S.s, d_utg=wild.data_ptr(), out=C.byref(h)) == 0 and h.value
    assert 0 <= Lb.cp_kmer_sorted_size(h) <= len(ents) and tal[0] == len(U)
    Lb.cp_kmer_sorted_destroy(h)
    # no unitigs in range: no arrays are needed, the result is empty
    Z = S.unitigs((1000, None), where=True, links=True)
    assert call(S.s, u=Z.u, d_utg=None, g=Z.g, out=C.byref(h)) == 0 and h.value
    assert Lb.cp_kmer_sorted_size(h) == 0 and tal.tolist() == [0] * 7
    Lb.cp_kmer_sorted_destroy(h)
    with pytest.raises(ValueError):
        S.prune(S.unitigs(), tips=K)                       # no where arrays, no links
    with pytest.raises(ValueError):
        S.prune(W, tips=K)                                 # of another snapshot
    with pytest.raises(ValueError):
        S.prune(U, tips=-1)
    with pytest.raises(ValueError):
        S.prune(U, tips=K, weight=torch.zeros(3, dtype=torch.int64))
    for x in (Z, U, V, W, S, other, small):
        x.close()


# ---- 10. the read sets of the host test through clean, round by round ----

@pytest.mark.parametrize("spaced", [True, False])
@pytest.mark.parametrize("K", [15, 21])
def test_clean_round_by_round(torch_dev, K, spaced):
    torch = torch_dev
    g, seqs = PC.read_set(1, K, spaced)
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    limits = (0, 2 * K, 2 * K - 1)
    want, tallies = PR.clean(ents, K, None, limits)
    out, got = S.clean(None, *limits)
    assert got == tallies
    check(torch, out, want, K)
    if spaced:
        assert [x for x, _ in want] == [x for x, _ in UO.table([g], K)] and len(got) == 2
    out.close()
    want1, t1 = PR.clean(ents, K, (2, None), limits, rounds=1)         # a range in round 1, and the rounds run out
    out, got = S.clean((2, None), *limits, rounds=1)
    assert got == t1 and len(got) == 1
    check(torch, out, want1, K)
    out.close()
    S.close()


# ---- 11. a random set of about 50 000 keys ----

def test_fifty_thousand_keys(torch_dev):
    torch = torch_dev
    K = 21
    rng = random.Random(50)
    g = rnd(rng, 20000)
    seqs = [g] * 3 + PC.reads(rng, g, K, False)
    ents = UO.table(seqs, K)
    assert 45000 < len(ents) < 60000
    S = load(torch, ents, K)
    _, why, t = check_prune(torch, S, ents, K, None, (K + 5, 2 * K, 2 * K - 1))
    assert t["tips"] > 20 and t["bubbles"] > 50 and t["unitigs"] > 3000
    check_prune(torch, S, ents, K, (2, None), (K + 5, 2 * K, 2 * K - 1))
    S.close()

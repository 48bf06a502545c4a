"""Phasing heterozygous sites from reads on a real MI355X (`-m gpu`): cp_kmer_sorted_het_sites, cp_kmer_counts_add_keys,
cp_kmer_sorted_read_links, cp_phase_forest, cp_kmer_sorted_phase_split and the driver SortedKmers.phase, each against
tests/phase_oracle.py.  Everything is integers: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import hetpairs_oracle as HO
import ktab_oracle as KO
import phase_oracle as PO
from test_gpu_ktab import flat, table_of
from test_gpu_setop import check as check_snapshot
from test_gpu_tabprof import i64, load

pytestmark = pytest.mark.gpu
EINVAL, EOVERFLOW = -1, -5
CELLS = 16384                                              # KC_CELLS: positions per block of the profile kernels


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def check_sites(torch, S, ents, K):
    mate, mark, ns = PO.sites(ents, K)
    got_mark, got_ns, tally, got_mate = S.het_sites(mates=True)
    assert got_mark.dtype == torch.int32 and got_mate.dtype == torch.int64
    assert got_mate.tolist() == mate and got_mark.tolist() == mark and got_ns == ns
    assert tally == {"mated": 2 * ns, "unmated": len(ents) - 2 * ns}
    m2, n2, t2 = S.het_sites()                             # without d_mate: the same marks
    assert m2.tolist() == mark and n2 == ns and t2 == tally
    return ns


# ---- het_sites ----

@pytest.mark.parametrize("K", [20, 21, 31, 63])
def test_het_sites(torch_dev, K):
    torch = torch_dev
    ents = HO.planted(random.Random(300 + K), K, 3000)     # more than a tile: families of degree 2 are unmated
    S = load(torch, ents, K, piece=999)
    ns = check_sites(torch, S, ents, K)
    assert 0 < 2 * ns < len(ents) and max(HO.degrees(ents, K)) >= 2
    uniq = HO.members(ents, K, None, True)                 # the result of het_pairs(unique): every entry is mated
    P = S.het_pairs(1, 1, True, table=True)[2]
    check_snapshot(torch, P, uniq, K)
    assert check_sites(torch, P, uniq, K) * 2 == len(uniq) > 0
    P.close()
    S.close()


def test_het_sites_chain_and_empty(torch_dev):
    torch = torch_dev
    seq = b"AACAAAAACAA"                                   # K = 4: AACA ~ AAAA ~ ACAA, a chain and no clique
    T = table_of(torch, [seq], 4)
    S = T.sorted(1)
    ents = KO.table([seq], 4)
    mate, mark, ns = PO.sites(ents, 4)
    at = {x: i for i, (x, _) in enumerate(ents)}
    assert all(mate[at[PO.encode(s)]] == -1 for s in (b"AACA", b"AAAA", b"ACAA"))
    check_sites(torch, S, ents, 4)
    E = S.combine(S, "sub")                                # an empty snapshot
    assert len(E) == 0
    mk, n0, t0 = E.het_sites()
    assert mk.numel() == 0 and n0 == 0 and t0 == {"mated": 0, "unmated": 0}
    for x in (E, S, T):
        x.close()


# ---- add_keys ----

def test_add_keys(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import ClassProError
    from classpro_amd.api import KmerCounts
    rng = np.random.default_rng(3)
    distinct = rng.integers(0, 1 << 62, 3000, dtype=np.int64)
    keys = np.concatenate([distinct[rng.integers(0, 3000, 200000)], np.full(70000, distinct[7])])
    rng.shuffle(keys)
    T = KmerCounts(32, initial_slots=64)                   # 64 slots: failed inserts, growth and replay
    T.add_keys(torch.from_numpy(keys[:150000]).cuda())
    T.add_keys(torch.from_numpy(keys[150000:]).cuda(), hi=torch.zeros(len(keys) - 150000, dtype=torch.int64))
    T.add_keys(torch.zeros(0, dtype=torch.int64))          # n = 0
    s = T.sorted(1)
    want, cnt = np.unique(keys, return_counts=True)
    assert s.lo.cpu().numpy().tolist() == want.tolist() and s.counts.cpu().numpy().tolist() == cnt.tolist()
    assert not s.hi.any() and T.stats()["growths"] > 0 and T.stats()["n_kmers"] == len(keys)
    s.close()
    T.close()
    T = KmerCounts(32)                                     # the first call sizes an unsized table; hi = 1 is bit 63
    T.add_keys(torch.tensor([5, 5, 9], dtype=torch.int64), hi=torch.tensor([1, 1, 0], dtype=torch.int64))
    s = T.sorted(1)
    assert (s.hi.tolist(), s.lo.tolist(), s.counts.tolist()) == ([0, 1], [9, 5], [1, 2])
    s.close()
    with pytest.raises(ClassProError) as e:                # a key of more than 2K bits, found on the device; the others are added
        T.add_keys(torch.tensor([1, 2], dtype=torch.int64), hi=torch.tensor([2, 0], dtype=torch.int64))
    assert e.value.code == EINVAL and "1 of the 2 keys" in str(e.value)
    with pytest.raises(ClassProError) as e:
        T.add_keys(torch.tensor([-1], dtype=torch.int64))  # lo > 2^63 - 1
    assert e.value.code == EINVAL
    s = T.sorted(1)
    assert s.lo.tolist() == [2, 9, 5]
    s.close()
    T.close()
    T = KmerCounts(5)                                      # 2K = 10 bits
    with pytest.raises(ClassProError):
        T.add_keys(torch.tensor([1023, 1024], dtype=torch.int64))
    T.close()
    F = KmerCounts(32, filter_bits=1 << 16)                # a filtered table is refused
    with pytest.raises(ClassProError) as e:
        F.add_keys(torch.tensor([1], dtype=torch.int64))
    assert e.value.code == EINVAL and "cp_kmer_counts_add_keys" in str(e.value)
    F.close()


# ---- read_links ----

K = 21


@pytest.fixture(scope="module")
def links_case(torch_dev):
    """A contig of 40,000 bases and a table P whose k-mers END at chosen positions of it: at a chunk edge (63, 64), at the
    edges of blocks of 8192 and 16384 positions, then nothing for two blocks."""
    rng = random.Random(17)
    contig = bytes(rng.choice(b"ACGT") for _ in range(40000))
    ends = [63, 64, 200, 8191, 8192, CELLS - 1, CELLS, 39000, 39500, 39999]
    assert ends[7] // 8192 - ends[6] // 8192 >= 2          # a whole block of the marker kernel without a marker
    keys, sh = {}, 2 * (K - 1 - K // 2)
    for n, j in enumerate(ends):
        x = HO.canon(PO.encode(contig[j - K + 1:j + 1]), K)
        y = HO.canon(x ^ (1 + n % 3) << sh, K)
        keys[x], keys[y] = 3 + n, 40 + n
    ents = sorted(keys.items())
    assert len(ents) == 2 * len(ends)
    kmer = lambda j: contig[j - K + 1:j + 1]
    mate_of = lambda j: PO.decode(HO.canon(PO.encode(kmer(j)), K) ^ (1 + ends.index(j) % 3) << sh, K)
    reads = [contig, contig[:K - 1], b"", kmer(200) + b"N" + kmer(8191),             # an N between two markers: the link stays
             b"", b"ACGT", kmer(64) + b"A" + mate_of(64) + PO.revcomp_seq(kmer(64)),   # the same site three times: two selfs
             PO.revcomp_seq(contig[8000:8400]), b"", kmer(39999)]
    return torch_dev, ents, reads


def run_links(torch, S, mark, reads, **kw):
    links, tally = S.read_links(flat(torch, reads), mark, **kw)
    return links.tolist(), tally.tolist()


@pytest.mark.parametrize("canonical", [True, False])
def test_read_links(links_case, canonical, monkeypatch):
    torch, ents, reads = links_case
    S = load(torch, ents, K)
    mate, mark, ns = PO.sites(ents, K)
    assert ns == len(ents) // 2
    mk = S.het_sites()[0]
    want, wt = PO.read_links(ents, mark, reads, K, canonical)
    if canonical:
        assert wt == [10 + 2 + 3 + 2 + 1, 9 + 1 + 1, 2] and len(set(want)) >= 9
    else:
        assert 0 < wt[0] < 18                              # forward keys: some of the contig's k-mers are not their canonical form
    assert run_links(torch, S, mk, reads, canonical=canonical) == (want, wt)
    monkeypatch.setenv("CLASSPRO_PHASE_GUESS", "1")        # the staging array too small: the pass is repeated at the exact size
    assert run_links(torch, S, mk, reads, canonical=canonical) == (want, wt)
    monkeypatch.delenv("CLASSPRO_PHASE_GUESS")
    order = list(range(len(reads)))                        # the reads permuted: the same multiset of keys
    random.Random(5).shuffle(order)
    got, gt = run_links(torch, S, mk, [reads[i] for i in order], canonical=canonical)
    assert sorted(got) == sorted(want) and gt == wt and got != want
    S.close()


def test_read_links_capacity(links_case):
    torch, ents, reads = links_case
    from classpro_amd._lib import ClassProError
    S = load(torch, ents, K)
    mk = S.het_sites()[0]
    want, wt = PO.read_links(ents, PO.sites(ents, K)[1], reads, K)
    seq, off = flat(torch, reads)
    total = C.c_int64(-1)
    tally = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    rc = S.L.cp_kmer_sorted_read_links(S.s, mk.data_ptr(), 1, seq.data_ptr(), off.data_ptr(), len(reads), int(off[-1]), None, 0,
                                       C.byref(total), tally.data_ptr(), None)              # the counting call
    assert rc == EOVERFLOW and total.value == len(want) and tally.tolist() == [0, 0, 0]
    with pytest.raises(ClassProError) as e:                # one too small: the exact total, an untouched tally
        S.read_links((seq, off), mk, capacity=len(want) - 1, tally=tally)
    assert e.value.code == EOVERFLOW and "%d links" % len(want) in str(e.value) and tally.tolist() == [0, 0, 0]
    links, t = S.read_links((seq, off), mk, capacity=len(want), tally=tally)
    assert links.tolist() == want and t is tally and tally.tolist() == wt
    S.read_links((seq, off), mk, tally=tally)              # added to
    assert tally.tolist() == [2 * x for x in wt]
    empty, t0 = S.read_links(flat(torch, [b"", b"ACG"]), mk)
    assert empty.numel() == 0 and t0.tolist() == [0, 0, 0]
    S.close()


# ---- phase_forest ----

def edges_of(torch, counts):
    """The edge snapshot of {link key: occurrences}, built with add_keys and sorted."""
    from classpro_amd.api import KmerCounts
    T = KmerCounts(32)
    keys = np.repeat(np.array(list(counts.keys()), dtype=np.int64), np.array(list(counts.values()), dtype=np.int64))
    T.add_keys(torch.from_numpy(keys).cuda())
    s = T.sorted(1)
    T.close()
    return s


def check_forest(torch, counts, nsites, min_support=2):
    from classpro_amd.api import phase_forest
    E = edges_of(torch, counts)
    block, side, t = phase_forest(E, nsites, min_support)
    E.close()
    wb, ws, wt = PO.forest(counts, nsites, min_support)
    assert block.dtype == torch.int64 and side.dtype == torch.uint8
    assert block.tolist() == wb and side.tolist() == ws and t == wt
    return wb, ws, wt


def test_forest_path_and_star(torch_dev):
    torch = torch_dev
    rng = random.Random(9)
    path = {PO.link_key(s, 0, s + 1, rng.randint(0, 1)): 2 for s in range(4999)}
    wb, ws, t = check_forest(torch, path, 5000)
    assert (t["blocks"], t["largest"], t["forest"], t["conflicts"]) == (1, 5000, 4999, 0) and set(wb) == {0} and 0 < sum(ws) < 5000
    path = {k: 1 + rng.randint(1, 5) for k in path}        # margins of every size: long chains of hooks in one round
    check_forest(torch, path, 5000)
    star = {PO.link_key(0, 0, s, s & 1): 3 for s in range(1, 1000)}
    wb, ws, t = check_forest(torch, star, 1000)
    assert t["largest"] == 1000 and t["rounds"] == 1 and ws == [s & 1 for s in range(1000)]


def test_forest_triangles_and_classes(torch_dev):
    torch = torch_dev
    key = PO.link_key
    wb, ws, t = check_forest(torch, {key(0, 0, 1, 0): 3, key(1, 0, 2, 0): 2, key(0, 0, 2, 1): 1}, 4, 1)
    assert (ws, t["conflicts"], t["single"]) == ([0, 0, 0, 0], 1, 1)          # margins 3, 2, 1: the margin-1 edge conflicts
    wb, ws, t = check_forest(torch, {key(0, 0, 1, 1): 2, key(0, 0, 2, 0): 2, key(1, 0, 2, 0): 2}, 3)
    assert (ws, t["conflicts"]) == ([0, 1, 0], 1)          # equal margins: the tie goes by (s, t)
    wb, ws, t = check_forest(torch, {key(0, 0, 1, 0): 65535, key(0, 0, 2, 0): 70000, key(1, 0, 2, 1): 70000}, 3)
    assert (ws, t["conflicts"]) == ([0, 0, 0], 1)          # 70000 is clamped to 65535: (0, 1) comes first
    counts = {key(0, 0, 1, 0): 1, key(2, 0, 3, 0): 2, key(2, 0, 3, 1): 2, key(4, 0, 5, 1): 2, 3 << 32 | 2 << 1: 9, 1 << 32 | 9 << 1: 9,
              key(6, 0, 7, 0): 4, key(6, 0, 7, 1): 1}      # weak, tied, only a trans key, two bad keys, both keys of a pair
    wb, ws, t = check_forest(torch, counts, 8)
    assert (t["edges"], t["weak"], t["tied"], t["kept"], t["bad"], t["blocks"]) == (4, 1, 1, 2, 2, 2)
    assert wb == [0, 1, 2, 3, 4, 4, 6, 6] and ws == [0, 0, 0, 0, 0, 1, 0, 0]
    wb, ws, t = check_forest(torch, {}, 5)                  # no edges
    assert wb == [0, 1, 2, 3, 4] and t["single"] == 5 and t["rounds"] == 0
    wb, ws, t = check_forest(torch, {key(0, 0, 1, 0): 2}, 0)   # nsites = 0: the key is bad
    assert wb == [] and t["bad"] == 1 and t["edges"] == 0


def test_forest_random_graph(torch_dev):
    torch = torch_dev
    rng = random.Random(21)
    counts = {}
    while len(counts) < 6000:
        s, u = rng.randrange(2000), rng.randrange(2000)
        if s != u:
            x = rng.randint(0, 1)
            counts[PO.link_key(s, 0, u, x)] = rng.randint(1, 5)
            if rng.random() < 0.3:                         # both keys of the pair
                counts[PO.link_key(s, 0, u, 1 - x)] = rng.randint(1, 5)
    wb, ws, t = check_forest(torch, counts, 2000)
    assert t["conflicts"] > 100 and t["tied"] > 0 and t["weak"] > 100 and t["rounds"] > 1 and t["largest"] > 1000
    check_forest(torch, counts, 2000, 1)
    check_forest(torch, counts, 1500, 3)                   # keys that name sites past the end are bad


def test_forest_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import ClassProError
    from classpro_amd.api import phase_forest
    E = edges_of(torch, {PO.link_key(0, 0, 1, 0): 2})
    T = table_of(torch, [b"ACGTACGTACGTAAC"], 5)
    S = T.sorted(1)
    for args in ((S, 2, 2), (E, 2, 0), (E, -1, 2), (E, 1 << 31, 2)):
        with pytest.raises(ClassProError) as e:
            phase_forest(*args)
        assert e.value.code == EINVAL and "cp_phase_forest" in str(e.value)
    for x in (E, S, T):
        x.close()


# ---- phase_split and the driver ----

@pytest.fixture(scope="module")
def genome_case():
    rng = random.Random(K)
    h1, h2, snps = PO.genome(rng, K)
    return h1, h2, snps, PO.tiled_reads((h1, h2))


def check_phase(torch, reads, count_range, batches):
    T = table_of(torch, reads, K)
    S = T.sorted(1)
    got = S.phase([flat(torch, b) for b in batches], count_range=count_range, min_support=2)
    want = PO.phase(PO.table(reads, K), K, batches, count_range, 2)
    assert got["nsites"] == want["nsites"] and got["sites"] == want["sites"] and got["links"] == want["links"]
    assert got["forest"] == want["forest"]
    assert got["mark"].tolist() == want["mark"] and got["block"].tolist() == want["block"] and got["side"].tolist() == want["side"]
    for name in ("P", "A", "B"):
        check_snapshot(torch, got[name], want[name], K)
        if want[name]:
            hi, lo, _ = KO.hi_lo_cnt(want[name])
            assert got[name].find(i64(torch, hi), i64(torch, lo)).tolist() == list(range(len(want[name])))
    a, b, p = ({x for x, _ in want[n]} for n in ("A", "B", "P"))
    assert not a & b and a | b <= p
    for x in (got["P"], got["A"], got["B"], S, T):
        x.close()
    return want


def test_phase_first_principles(torch_dev, genome_case):
    h1, h2, snps, reads = genome_case
    r = check_phase(torch_dev, reads, None, [reads[:30], reads[30:31], reads[31:]])
    f = r["forest"]
    assert (f["blocks"], f["conflicts"], f["tied"], f["single"]) == (1, 0, 0, 0) and r["nsites"] == len(snps)
    k1, k2 = ({x for x, _ in PO.table([h], K)} for h in (h1, h2))
    p = {x for x, _ in r["P"]}
    assert {frozenset(x for x, _ in r["A"]), frozenset(x for x, _ in r["B"])} == {frozenset((k1 - k2) & p), frozenset((k2 - k1) & p)}


def test_phase_reads_with_errors(torch_dev, genome_case):
    h1, h2, snps, reads = genome_case
    rng = random.Random(77)
    noisy = []
    for s in reads:                                        # 0.5 % substitutions
        s = bytearray(s)
        for i in range(len(s)):
            if rng.random() < 0.005:
                s[i] = rng.choice([c for c in b"ACGT" if c != s[i]])
        noisy.append(bytes(s))
    r = check_phase(torch_dev, noisy, (3, None), [noisy[:50], noisy[50:]])
    assert r["nsites"] > 0.9 * len(snps) and r["forest"]["blocks"] >= 1 and r["forest"]["largest"] > len(snps) // 2


def test_split_arguments(torch_dev):
    torch = torch_dev
    ents = HO.planted(random.Random(4), K, 300)
    S = load(torch, ents, K)
    mate, mark, ns = PO.sites(ents, K)
    mk = S.het_sites()[0]
    block = list(range(ns))
    side = [s & 1 for s in range(ns)]
    for s in range(0, ns - 1, 3):                          # every third site takes its neighbour into a block; the rest stay single
        block[s + 1] = s
    A, B = S.phase_split(mk, i64(torch, block), torch.tensor(side, dtype=torch.uint8, device="cuda:0"))
    wa, wb = PO.split(ents, mark, block, side)
    check_snapshot(torch, A, wa, K)
    check_snapshot(torch, B, wb, K)
    assert wa and wb and len(wa) + len(wb) < 2 * ns
    with pytest.raises(ValueError):
        S.phase_split(mk, i64(torch, block), torch.zeros(ns + 1, dtype=torch.uint8, device="cuda:0"))
    for x in (A, B, S):
        x.close()

"""cp_kmer_sorted_read_paths (SortedKmers.read_paths) on a real MI355X (`-m gpu`), against the walking oracle of
tests/path_oracle.py and against the properties Spelling and Mirror taken from the outputs alone: the hand cases of
tests/test_gpu_unitig_graph.py with their sources, every substring of K and K+1 bases, reads with an N, empty and short
reads; closed chains run round three times; one long segment over four blocks at every lane and block edge; reads of K
bases in one lane's chunk; a read whose every position is a head across a block edge; random read sets at K up to 63 with
and without a count range; 200,000 keys and 2 Mbases against positions known by construction; coverage and support, their
sums, batching and accumulation; the identities with `profiles` and `read_runs`; capacity and overflow; that everything
passed in is only read; foreign where arrays; the argument errors; a thousand `cp_count_nonzero` calls in a row, with a
`read_paths` call after every tenth, that all give the one answer.  Everything is integers and bytes: the tolerance is
zero."""
import ctypes as C
import random

import pytest

import path_oracle as PO
import unitig_oracle as UO
from test_gpu_ktab import flat
from test_gpu_tabprof import load
from test_gpu_unitig_graph import hand_cases
from test_gpu_unitigs import circle, with_counts
from test_paths_host import bubble, haplotypes, random_reads
from test_unitig_host import clean, rcs, rnd, simple

pytestmark = pytest.mark.gpu
EINVAL, EOVERFLOW = -1, -5
BLOCK = 16384
FIELDS = PO.FIELDS


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def enc(reads):
    return [r.encode() for r in reads]


def got(torch, S, U, reads, **kw):
    """(seg_off, [(first, n, x, q, read, flags)], tally) as lists."""
    off, s, t = S.read_paths(U, flat(torch, enc(reads)), **kw)
    assert off.dtype == torch.int64 and s["first"].dtype == s["x"].dtype == torch.int64
    assert all(s[k].dtype == torch.int32 for k in ("n", "q", "read", "flags"))
    return off.cpu().tolist(), list(zip(*[s[k].cpu().tolist() for k in FIELDS])), t


def check(torch, S, U, P, reads, mirror=True):
    """The records, the offsets, the tally, the coverage and the support of one batch against the oracle, and the two
    properties from the outputs alone.  Returns the oracle's batch."""
    want = P.batch(reads)
    off, segs, t = got(torch, S, U, reads, coverage=True, support=True)
    assert off == want[0] and segs == want[1], (P.K, P.range)
    assert {k: t[k] for k in PO.TALLY} == want[2]
    assert t["coverage"].cpu().tolist() == want[3] and t["support"].cpu().tolist() == want[4]
    assert sum(want[3]) == t["present"] and sum(want[4]) == t["joined"]
    if mirror:
        strings = U.strings()
        off2, segs2, _ = got(torch, S, U, [PO.rcs(r) for r in reads])
        for r, read in enumerate(reads):
            PO.properties(P.K, strings, read, segs[off[r]:off[r + 1]], segs2[off2[r]:off2[r + 1]])
    return want


def sources(name, K):
    """The strings the tables of hand_cases() were made from."""
    if name == "single":
        return ["ACCGT"]
    if name == "homopolymer":
        return ["A" * 60]
    if name in ("hairpin", "palindrome"):
        return ["AT" * 30]
    if name == "k plus one":
        return ["ACGGTC"]
    if name == "bubble":
        return list(bubble()[:2])
    if name == "closed":
        rng = random.Random(5)
        while True:
            s = rnd(rng, 40)
            c = circle(s, K)
            if clean([c[:40 + K - 2]], K, 40):
                return [c, s * 3 + s[:K - 1]]
    s = simple(random.Random(5), 30, 5)
    return [s + rcs(s)]


# ---- 1. the hand cases ----

@pytest.mark.parametrize("which", range(8))
def test_hand_cases(torch_dev, which):
    torch = torch_dev
    name, ents, K = hand_cases()[which]
    src = sources(name, K)
    assert [x for x, _ in UO.table(src, K)] == [x for x, _ in ents]
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    P = PO.Paths(ents, K)
    reads = src + [rcs(s) for s in src]
    for s in src:
        reads += [s[i:i + K] for i in range(len(s) - K + 1)] + [s[i:i + K + 1] for i in range(len(s) - K)]
        reads += [s[:len(s) // 2] + "N" + s[len(s) // 2 + 1:], "N" + s, s + "N", s[:K - 1], "", s[:1]]
    want = check(torch, S, U, P, reads)
    if name == "bubble":
        assert [(f, n, fl) for f, n, _, _, _, fl in want[1][:3]] == [(0, 6, 0), (6, 7, 1), (13, 6, 1)]
    if name == "closed":
        three = [s for s in want[1] if s[4] == 1]
        assert sum(s[1] for s in three) == 120 and [s[5] for s in three] == [0] + [1] * (len(three) - 1)
    check(torch, S, U, P, reads + reads, mirror=False)                                # the same reads twice in one batch
    off, segs, t = got(torch, S, U, [])                                                # an empty batch
    assert (off, segs) == ([0], []) and all(t[k] == 0 for k in PO.TALLY)
    assert got(torch, S, U, ["", "ACG"[:K - 1], ""])[:2] == ([0, 0, 0, 0], [])
    U.close()
    S.close()


def test_empty_table(torch_dev):
    torch = torch_dev
    K = 9
    E = load(torch, [], K)
    U = E.unitigs(where=True, links=True)
    reads = [rnd(random.Random(1), 50), "ACGTNACGTACGTACGT", "", "ACG"]
    off, segs, t = got(torch, E, U, reads, coverage=True, support=True)
    assert (off, segs) == ([0] * 5, []) and (t["positions"], t["present"], t["absent"], t["other"]) == (51, 0, 46, 5)
    assert t["coverage"].numel() == 0 and t["support"].numel() == 0
    U.close()
    E.close()


@pytest.mark.parametrize("n", [2, 3, 64])
def test_closed_chains_three_times_round(torch_dev, n):
    torch = torch_dev
    K = 21
    rng = random.Random(n)
    while True:
        s = rnd(rng, n)
        c = circle(s, K)
        if clean([c[:n + K - 2]], K, n):
            break
    ents = UO.table([c], K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    P = PO.Paths(ents, K)
    assert len(P.utgs) == 1 and P.utgs[0][2]
    reps = s * ((3 * n + K - 1) // n + 2)
    reads = [reps[a:a + 3 * n + K - 1] for a in range(n)]
    want = check(torch, S, U, P, reads + [rcs(r) for r in reads])
    assert all(sum(x[1] for x in want[1][want[0][r]:want[0][r + 1]]) == 3 * n for r in range(2 * n))
    assert want[2]["joined"] >= 2 * 2 * n and sorted(want[4]) == sorted([want[2]["joined"] // 2] * 2)
    U.close()
    S.close()


# ---- 2. lanes and blocks ----

@pytest.fixture(scope="module")
def long_path(torch_dev):
    """One 50,000-base sequence whose k-mers form one path: the table, and the read."""
    torch = torch_dev
    K = 21
    rng = random.Random(50000)
    while True:
        s = rnd(rng, 50000)
        w = {s[i:i + K - 1] for i in range(len(s) - K + 2)}
        if len(w) == len(s) - K + 2 and not any(rcs(x) in w for x in w):
            break
    ents = UO.table([s], K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    assert len(U) == 1 and U.strings()[0] in (s, rcs(s))
    return S, U, s, K


@pytest.mark.parametrize("at", [63, 64, 65, 16383, 16384, 16385])
def test_one_segment_over_four_blocks(torch_dev, long_path, at):
    """The read's first k-mer position falls on batch position `at`: filler reads without a k-mer position before it."""
    torch = torch_dev
    S, U, s, K = long_path
    fwd = U.strings()[0] == s
    nk = len(s) - K + 1
    fill = at - (K - 1)
    filler = ["ACGTACGTACGTACGTACGT"[:K - 1]] * (fill // (K - 1)) + ["A" * (fill % (K - 1))]
    assert sum(len(f) for f in filler) + K - 1 == at
    reads = filler + [s, "", rcs(s)]
    off, segs, t = got(torch, S, U, reads, coverage=True)
    r = len(filler)
    assert off == [0] * (r + 1) + [1, 1, 2]
    assert segs == [(0, nk, 0 if fwd else 1, 0, r, 0), (0, nk, 1 if fwd else 0, 0, r + 2, 0)]
    assert (t["positions"], t["present"], t["segments"], t["joined"], t["walks"]) == (2 * nk, 2 * nk, 2, 0, 2)
    assert t["coverage"].tolist() == [2 * nk]


@pytest.mark.parametrize("K", [5, 21])
def test_reads_of_exactly_k_bases_in_a_row(torch_dev, K):
    """100 reads of K bases: at K = 5 they share a few lanes' chunks of 64 positions.  Any sequence serves: a read of K
    bases has one position, and that is one segment whatever the graph."""
    torch = torch_dev
    rng = random.Random(K)
    s = rnd(rng, 100 + K - 1)
    ents = UO.table([s], K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    P = PO.Paths(ents, K)
    reads = [s[i:i + K] for i in range(100)]
    want = check(torch, S, U, P, reads + [s] + [rcs(r) for r in reads[:30]] + ["", s[:K - 1], s[3:]])
    assert want[0][:101] == list(range(101)) and all(x[1] == 1 and x[5] == 0 for x in want[1][:100])
    U.close()
    S.close()


def test_every_position_a_head_across_a_block_edge(torch_dev):
    """The complete set of K = 6: every node is its own unitig, so every position of a read is a head, all but the first
    joined; the read straddles the edge of the first block."""
    torch = torch_dev
    K = 6
    ents = with_counts({UO.canon(x, K) for x in range(1 << (2 * K))}, K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    P = PO.Paths(ents, K)
    assert len(P.utgs) == len(ents)
    rng = random.Random(6)
    read = rnd(rng, 700)
    filler = rnd(rng, BLOCK - 300)
    want = check(torch, S, U, P, [filler, read, rcs(read)], mirror=False)
    mine = want[1][want[0][1]:want[0][2]]
    assert len(mine) == 695 and [x[5] for x in mine] == [0] + [1] * 694 and want[2]["joined"] == want[2]["segments"] - 3
    U.close()
    S.close()


# ---- 3. random ----

@pytest.mark.parametrize("K", [5, 12, 21, 32, 33, 63])
def test_random_reads(torch_dev, K):
    torch = torch_dev
    rng = random.Random(K)
    seqs = haplotypes(rng, K, n=1500, snps=12)
    seqs += [seqs[0][100:400], seqs[1][700:1200]]                                      # counts above 1 for the range
    ents = UO.table(seqs, K)
    S = load(torch, ents, K, piece=999)
    reads = random_reads(rng, seqs, 2000, 400)
    for count_range in (None, (2, None)):
        U = S.unitigs(count_range, where=True, links=True)
        P = PO.Paths(ents, K, count_range)
        want = check(torch, S, U, P, reads)
        assert want[2]["joined"] > 50 and want[2]["absent"] > 0 and want[2]["other"] > 0 and want[2]["walks"] > 1000
        if count_range is None:
            whole = want[2]["present"]
        else:
            assert 0 < want[2]["present"] < whole
        U.close()
    S.close()


def test_two_megabases_over_200000_keys(torch_dev):
    """Twenty random sequences of 10,000 bases at K = 21: each is one unitig, so a read cut from one of them is one segment
    whose x and q follow from where it was cut; one read in four carries a substitution and is two segments."""
    torch = torch_dev
    K = 21
    rng = random.Random(2000000)
    seqs = [rnd(rng, 10000) for _ in range(20)]
    S = load(torch, UO.table(seqs, K), K)
    assert len(S) == 20 * (10000 - K + 1)
    U = S.unitigs(where=True, links=True)
    strings = U.strings()
    assert len(U) == 20 and U.nlinks == 0
    place = {}
    for i, s in enumerate(seqs):
        u = strings.index(s) if s in strings else strings.index(rcs(s))
        place[i] = (u, strings[u] == s)
    reads, want, cov = [], [], [0] * 20
    total = 0
    while total < 2000000:
        i, L = rng.randrange(20), rng.randrange(K + 60, 3000)
        a = rng.randrange(10000 - L)
        strand = rng.random() < 0.5
        read = seqs[i][a:a + L]
        u, fwd = place[i]
        nk, nodes = L - K + 1, 10000 - K + 1
        cut = rng.randrange(K + 5, L - K - 5) if rng.random() < 0.25 else None
        if cut is not None:
            read = read[:cut] + {"A": "C", "C": "G", "G": "T", "T": "A"}[read[cut]] + read[cut + 1:]
        parts = [(0, nk)] if cut is None else [(0, cut - K + 1), (cut + 1, nk - cut - 1)]
        mine = []
        for f, n in parts:                                 # on the sequence the part begins at k-mer a + f
            x, q = 2 * u + (0 if fwd else 1), a + f        # the orientation of u that spells the sequence
            if strand:
                x, q, f = x ^ 1, nodes - q - n, nk - f - n
            mine.append((f, n, x, q, len(reads), 0))
            cov[u] += n
        want += sorted(mine)
        reads.append(rcs(read) if strand else read)
        total += L
    off, segs, t = got(torch, S, U, reads, coverage=True)
    assert segs == want and off[-1] == len(want) and t["joined"] == 0 and t["coverage"].tolist() == cov
    assert t["present"] == sum(cov) and t["absent"] == K * (len(want) - len(reads)) and t["other"] == 0
    U.close()
    S.close()


# ---- 4. coverage and support ----

def test_sums_batching_and_accumulation(torch_dev):
    torch = torch_dev
    K = 12
    rng = random.Random(4)
    seqs = haplotypes(rng, K, n=600, snps=8)
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    P = PO.Paths(ents, K)
    reads = random_reads(rng, seqs, 60, 300)
    want = check(torch, S, U, P, reads, mirror=False)
    assert want[2]["joined"] > 10
    cov1, sup1 = want[3], want[4]
    for cut in range(len(reads) + 1):                      # a batch split in two calls at every read boundary
        cov = torch.zeros(len(U), dtype=torch.int64, device="cuda:0")
        sup = torch.zeros(U.nlinks, dtype=torch.int64, device="cuda:0")
        for part in (reads[:cut], reads[cut:]):
            _, _, t = got(torch, S, U, part, coverage=cov, support=sup)
            assert t["coverage"] is cov and t["support"] is sup
        assert cov.tolist() == cov1 and sup.tolist() == sup1, cut
    cov = torch.full((len(U),), 7, dtype=torch.int64, device="cuda:0")                 # added to, not overwritten
    sup = torch.full((U.nlinks,), -3, dtype=torch.int64, device="cuda:0")
    got(torch, S, U, reads, coverage=cov, support=sup)
    got(torch, S, U, reads, coverage=cov)
    assert cov.tolist() == [7 + 2 * c for c in cov1] and sup.tolist() == [c - 3 for c in sup1]
    V = S.unitigs(where=True)                              # no links: coverage yes, support no
    assert got(torch, S, V, reads, coverage=True)[2]["coverage"].tolist() == cov1
    with pytest.raises(ValueError):
        S.read_paths(V, flat(torch, enc(reads)), support=True)
    with pytest.raises(ValueError):
        S.read_paths(S.unitigs(links=True), flat(torch, enc(reads)))                   # no where arrays
    with pytest.raises(ValueError):
        S.read_paths(U, flat(torch, enc(reads)), coverage=torch.zeros(len(U) + 1, dtype=torch.int64, device="cuda:0"))
    V.close()
    U.close()
    S.close()


# ---- 5. identities with what exists ----

@pytest.mark.parametrize("count_range", [None, (2, None)])
def test_identities_with_profiles_and_read_runs(torch_dev, count_range):
    torch = torch_dev
    K = 21
    rng = random.Random(5)
    seqs = haplotypes(rng, K, n=1000, snps=8)
    seqs += [seqs[0][200:600]]
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    U = S.unitigs(count_range, where=True)
    reads = random_reads(rng, seqs, 300, 400)
    batch = flat(torch, enc(reads))
    off, segs, t = got(torch, S, U, reads)
    tally = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    prof = S.profiles(batch, tally=tally).view(torch.int16).to(torch.int64)
    lo = 1 if count_range is None else count_range[0]
    present = int((prof >= lo).sum().item())
    assert t["present"] == present and t["other"] == int(tally[2].item())
    assert t["absent"] == int(tally[0].item()) + int(tally[1].item()) - present and t["positions"] == int(tally.sum().item())
    roff, runs = S.read_runs(None, batch, emit=S.RUN_NONE | S.RUN_OTHER, a_range=count_range)
    cols = [runs[k].cpu().tolist() for k in ("first", "last", "read")]
    outside = {(r, i) for f, l, r in zip(*cols) for i in range(f, l + 1)}
    inside = {(r, i) for f, n, _, _, r, _ in segs for i in range(f, f + n)}
    every = {(r, i) for r, read in enumerate(reads) for i in range(len(read) - K + 1)}
    assert not (inside & outside) and (inside | outside) == every and len(inside) == t["present"]
    U.close()
    S.close()


# ---- 6. capacity ----

def raw(torch, L, S, U, reads, capacity, segs, g=True, cov=None, sup=None, utg=None, at=None):
    """One call of the C function: (rc, total, seg_off, tally)."""
    from classpro_amd.api import _stream_of
    seq, seq_off = flat(torch, enc(reads))
    n = len(reads)
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    total, tally = C.c_int64(-1), (C.c_int64 * 7)()
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    rc = L.cp_kmer_sorted_read_paths(S.s, U.u, ptr(U.utg if utg is None else utg), ptr(U.at if at is None else at),
                                     U.g if g else None, seq.data_ptr(), seq_off.data_ptr(), n, int(seq_off[-1].item()),
                                     ptr(segs), capacity, off.data_ptr(), ptr(cov), ptr(sup), tally, C.byref(total),
                                     _stream_of(torch.device("cuda:0")))
    torch.cuda.synchronize()
    return rc, total.value, off.cpu().tolist(), list(tally)


def test_capacity_and_overflow(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K = 12
    rng = random.Random(6)
    seqs = haplotypes(rng, K, n=600, snps=8)
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    P = PO.Paths(ents, K)
    reads = random_reads(rng, seqs, 80, 300)
    woff, wsegs, wt, wcov, wsup = P.batch(reads)
    n = len(wsegs)
    assert n > 100 and wt["joined"] > 10
    want_tally = [wt[k] for k in PO.TALLY]
    cov = torch.zeros(len(U), dtype=torch.int64, device="cuda:0")
    sup = torch.zeros(U.nlinks, dtype=torch.int64, device="cuda:0")
    rc, total, off, tally = raw(torch, L, S, U, reads, 0, None, cov=cov, sup=sup)      # the counting call
    assert (rc, total, off, tally) == (EOVERFLOW, n, woff, want_tally) and b"do not fit" in L.cp_last_error()
    assert not cov.any() and not sup.any()                                             # a call that overflows adds nothing
    buf = torch.full((n + 5, 4), -9, dtype=torch.int64, device="cuda:0")
    rc, total, off, tally = raw(torch, L, S, U, reads, n - 1, buf, cov=cov, sup=sup)   # one too few
    assert (rc, total, off, tally) == (EOVERFLOW, n, woff, want_tally) and not cov.any() and not sup.any()
    assert (buf[n - 1:] == -9).all()                                                   # nothing written beyond
    tail = buf.view(torch.int32)[:n - 1, 4:]
    rows = list(zip(buf[:n - 1, 0].tolist(), tail[:, 0].tolist(), buf[:n - 1, 1].tolist(), tail[:, 1].tolist(),
                    tail[:, 2].tolist(), tail[:, 3].tolist()))
    assert rows == wsegs[:n - 1]                                                       # the records below the capacity, whole
    buf.fill_(-9)
    rc, total, off, tally = raw(torch, L, S, U, reads, n, buf, cov=cov, sup=sup)       # exact
    assert (rc, total, off, tally) == (0, n, woff, want_tally) and (buf[n:] == -9).all()
    assert cov.tolist() == wcov and sup.tolist() == wsup
    U.close()
    S.close()


# ---- 7. only read; foreign arrays; argument errors ----

def test_inputs_are_only_read_and_foreign_arrays_stay_inside(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K = 12
    rng = random.Random(7)
    seqs = haplotypes(rng, K, n=600, snps=8)
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True, components=True)
    reads = random_reads(rng, seqs, 80, 300)
    views = [S.hi, S.lo, S.counts, U.seq, U.off, U.kc, U.flag, U.utg, U.at, U.loff, U.link, U.base, U.comp]
    before = [v.clone() for v in views]
    got(torch, S, U, reads, coverage=True, support=True)
    # where arrays of another table, and values that point anywhere: nothing raised, nothing outside the outputs touched
    other = haplotypes(random.Random(70), K, n=900, snps=3)
    T = load(torch, UO.table(other, K), K)
    V = T.unitigs(where=True, links=True)
    n = len(S)
    assert len(T) * 2 >= n
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    foreign = [(torch.cat([V.utg, V.utg])[:n].contiguous(), torch.cat([V.at, V.at])[:n].contiguous()),
               (torch.randint(-5, 1 << 40, (n,), generator=gen, device="cuda:0"), torch.randint(-5, 1 << 40, (n,), generator=gen, device="cuda:0")),
               (torch.full((n,), (1 << 62), dtype=torch.int64, device="cuda:0"), torch.full((n,), -1, dtype=torch.int64, device="cuda:0"))]
    guard = 64
    for utg, at in foreign:
        cov = torch.zeros(len(U) + 2 * guard, dtype=torch.int64, device="cuda:0")
        sup = torch.zeros(U.nlinks + 2 * guard, dtype=torch.int64, device="cuda:0")
        buf = torch.full((4096 + 2 * guard, 4), -9, dtype=torch.int64, device="cuda:0")
        rc, total, off, tally = raw(torch, L, S, U, reads, 4096, buf[guard:], cov=cov[guard:], sup=sup[guard:], utg=utg, at=at)
        assert rc in (0, EOVERFLOW) and total >= 0 and off[0] == 0 and off[-1] == total and off == sorted(off)
        assert not cov[:guard].any() and not cov[guard + len(U):].any() and not sup[:guard].any() and not sup[guard + U.nlinks:].any()
        assert (buf[:guard] == -9).all() and (buf[guard + 4096:] == -9).all()
    for v, b in zip(views, before):
        assert torch.equal(v, b)
    for x in (V, T, U, S):
        x.close()


def test_argument_errors(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    from classpro_amd.api import _stream_of
    L = lib()
    K = 12
    seqs = haplotypes(random.Random(8), K, n=300, snps=3)
    S = load(torch, UO.table(seqs, K), K)
    S9 = load(torch, UO.table(seqs, 9), 9)
    U = S.unitigs(where=True, links=True)
    U9 = S9.unitigs(where=True, links=True)
    seq, seq_off = flat(torch, enc(seqs))
    n, total_bases = len(seqs), int(seq_off[-1].item())
    off = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    buf = torch.zeros((64, 4), dtype=torch.int64, device="cuda:0")
    sup = torch.zeros(max(U.nlinks, 1), dtype=torch.int64, device="cuda:0")
    total = C.c_int64()
    st = _stream_of(torch.device("cuda:0"))
    good = dict(s=S.s, u=U.u, utg=U.utg.data_ptr(), at=U.at.data_ptr(), g=U.g, seq=seq.data_ptr(), seq_off=seq_off.data_ptr(), n=n,
                total_bases=total_bases, segs=buf.data_ptr(), capacity=64, off=off.data_ptr(), cov=None, sup=None, tally=None,
                total=C.byref(total))
    order = ("s", "u", "utg", "at", "g", "seq", "seq_off", "n", "total_bases", "segs", "capacity", "off", "cov", "sup", "tally", "total")
    call = lambda **kw: L.cp_kmer_sorted_read_paths(*[dict(good, **kw)[k] for k in order], st)
    assert call() in (0, EOVERFLOW)
    bad = [dict(s=None), dict(u=None), dict(total=None), dict(u=U9.u), dict(utg=None), dict(at=None), dict(g=None, sup=sup.data_ptr()),
           dict(n=-1), dict(total_bases=-1), dict(capacity=-1), dict(segs=None), dict(off=None), dict(seq_off=None), dict(seq=None)]
    for kw in bad:
        off.fill_(-7)
        assert call(**kw) == EINVAL and b"cp_kmer_sorted_read_paths" in L.cp_last_error(), kw
        torch.cuda.synchronize()
        assert (off == -7).all(), kw                       # before any launch
    assert call(g=None) in (0, EOVERFLOW) and call(segs=None, capacity=0) in (0, EOVERFLOW)
    c = C.c_int64(-1)
    v = torch.tensor([0, 3, 0, -1, 0, 9], dtype=torch.int64, device="cuda:0")
    assert L.cp_count_nonzero(v.data_ptr(), 6, C.byref(c), st) == 0 and c.value == 3
    big = torch.zeros(100000, dtype=torch.int64, device="cuda:0")
    big[::7] = 5
    assert L.cp_count_nonzero(big.data_ptr(), big.numel(), C.byref(c), st) == 0 and c.value == len(range(0, 100000, 7))
    for x in (U, U9, S, S9):
        x.close()


# ---- 8. the counters, over and over ----

def test_a_thousand_counts_in_a_row_are_one_answer(torch_dev):
    """A guard against a counter that is zeroed out of order: 1,000 consecutive cp_count_nonzero calls on
    one vector whose non-zeros are known, a small read_paths call after every tenth so that the stream-ordered pool keeps
    handing its memory back and forth between the two.  Every count, and every tally, coverage and support of read_paths,
    is the oracle's.  A wrong-count check, bounded and not retried: it stops at the first mismatch and names the call.  It
    cannot show that such a race is absent, only that it did not happen in these calls."""
    torch = torch_dev
    from classpro_amd._lib import lib
    from classpro_amd.api import _stream_of
    L = lib()
    K = 12
    rng = random.Random(8)
    seqs = haplotypes(rng, K, n=600, snps=8)
    ents = UO.table(seqs, K)
    S = load(torch, ents, K)
    U = S.unitigs(where=True, links=True)
    reads = random_reads(rng, seqs, 60, 300)
    woff, wsegs, wt, wcov, wsup = PO.Paths(ents, K).batch(reads)
    assert wt["present"] > 1000 and wt["absent"] > 0 and wt["other"] > 0 and wt["joined"] > 10
    batch = flat(torch, enc(reads))
    v = torch.zeros(100001, dtype=torch.int64, device="cuda:0")
    v[::7] = -3
    v[5::1001] = 1 << 40
    want = int((v != 0).sum().item())
    assert want == len(set(range(0, 100001, 7)) | set(range(5, 100001, 1001)))
    st = _stream_of(torch.device("cuda:0"))
    c = C.c_int64()
    for i in range(1000):
        c.value = -1
        assert L.cp_count_nonzero(v.data_ptr(), v.numel(), C.byref(c), st) == 0
        assert c.value == want, "cp_count_nonzero call %d gave %d, not %d" % (i, c.value, want)
        if i % 10 == 9:
            off, segs, t = S.read_paths(U, batch, coverage=True, support=True)
            assert {k: t[k] for k in PO.TALLY} == wt, "read_paths call %d" % (i // 10)
            assert t["coverage"].tolist() == wcov and t["support"].tolist() == wsup, "read_paths call %d" % (i // 10)
            assert off.tolist() == woff and len(segs["first"]) == len(wsegs), "read_paths call %d" % (i // 10)
    U.close()
    S.close()

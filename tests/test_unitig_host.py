"""tabunitig and the unitigs without a GPU: tests/unitig_oracle.py against cases worked out by hand and against its own
invariants (every in key once, both strands alike, no unitig that could be extended, the k-mers of the spelled unitigs are
the in keys), cp_unitig_n50, every error tabunitig reports before it touches the device (exact message, exit status 1,
empty stdout, no file created), and the symbols' declarations and the returns that need no device."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import ktab_oracle as KO
import unitig_oracle as UO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabunitig")
USAGE = "Usage: tabunitig [-v] <table>[.ktab][:<lo>-<hi>] [<out_root>]\n"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
rcs = lambda s: "".join(COMP[c] for c in reversed(s))
key = UO.key_of


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def sub_kmers(seqs, k):
    return [min(s[p:p + k], rcs(s[p:p + k])) for s in seqs for p in range(len(s) - k + 1)]


def clean(seqs, K, distinct):
    """The K-1-mers of the sequences fall into exactly `distinct` classes and none is its own reverse complement: two
    k-mers share a K-1-mer only where the sequences say so, so the graph branches nowhere else."""
    w = sub_kmers(seqs, K - 1)
    return len(set(w)) == distinct and all(x != rcs(x) for x in w)


def simple(rng, n, K):
    """A random sequence whose k-mers form one path."""
    while True:
        s = rnd(rng, n)
        if clean([s], K, n - K + 2):
            return s


def summary(ents, K, count_range=None):
    return [(f, t, c, kc) for f, t, c, kc, _ in UO.unitigs(ents, K, count_range)]


# ---- the oracle against the cases worked out by hand ----

def test_hand_single_kmer():
    ents = [(key("ACCGT"), 7)]
    assert UO.adjacency(ents, 5) == [0]
    assert summary(ents, 5) == [(0, "ACCGT", False, 7)]
    assert UO.where(ents, 5) == ([0], [0])
    assert UO.tally(ents, 5) == dict(keys=1, unitigs=1, bases=5, circular=0, longest=5, isolated=1, tips=0, branching=0, arcs=0)
    assert UO.fasta(UO.unitigs(ents, 5)) == b">0 LN:i:5 KC:i:7\nACCGT\n"
    assert UO.line(ents, 5) == "tabunitig: 1 k-mers, 1 unitigs, 5 bases, 0 circular, longest 5, N50 5\n"


def test_hand_homopolymer():
    ents = UO.table(["AAAAAAAA"], 5)
    assert ents == [(0, 4)]
    assert UO.adjacency(ents, 5) == [0x81]                 # AAAAA -> AAAAA by A, TTTTT -> TTTTT by T: the node itself
    assert summary(ents, 5) == [(0, "AAAAA", False, 4)]
    t = UO.tally(ents, 5)
    assert (t["isolated"], t["tips"], t["branching"], t["arcs"]) == (0, 0, 0, 2)


def test_hand_k_plus_one_bases():
    """ACGGTC at K = 5: ACGGT is the reverse complement of the key ACCGT (entry 0), CGGTC is a key (entry 1).  The path is
    state 1 -> state 2; its mirror starts at flip(2) = 3, so it is spelled from state 1: the smaller end node, reversed."""
    ents = UO.table(["ACGGTC"], 5)
    assert [UO.text_of(x, 5) for x, _ in ents] == ["ACCGT", "CGGTC"]
    assert UO.adjacency(ents, 5) == [0x20, 0x80]           # ACGGT -> CGGTC by C; GACCG -> ACCGT by T
    g = UO.Graph(ents, 5)
    assert g.out(1) == {1: 2} and g.out(3) == {3: 0} and g.out(0) == {} and g.out(2) == {}
    assert g.link(1) == 2 and g.link(3) == 0 and g.back(2) == 1
    assert summary(ents, 5) == [(1, "ACGGTC", False, 2)]
    assert UO.where(ents, 5) == ([0, 0], [1, 2])
    t = UO.tally(ents, 5)
    assert (t["tips"], t["arcs"], t["bases"]) == (2, 2, 6)


def test_hand_snp_bubble():
    K = 7
    rng = random.Random(3)
    while True:
        left, right = rnd(rng, 12), rnd(rng, 12)
        h1, h2 = left + "A" + right, left + "C" + right
        ents = UO.table([h1, h2], K)
        if len(ents) == 26 and clean([h1, h2], K, 20 + K - 1):       # 19 k-mers each, 12 of them shared
            break
    utgs = summary(ents, K)
    assert len(utgs) == 4
    assert sorted(len(t) for _, t, _, _ in utgs) == [12, 12, 2 * K - 1, 2 * K - 1]
    for _, t, circ, kc in utgs:
        assert not circ and any(t in h or rcs(t) in h for h in (h1, h2))
        assert kc == (len(t) - K + 1) * (2 if len(t) == 12 else 1)
    arms = {t for _, t, _, _ in utgs if len(t) == 2 * K - 1}
    assert {min(a, rcs(a)) for a in arms} == {min(x, rcs(x)) for x in (h1[12 - K + 1:12 + K], h2[12 - K + 1:12 + K])}
    t = UO.tally(ents, K)
    assert (t["branching"], t["tips"], t["isolated"]) == (2, 2, 0)


def test_hand_closed_sequence():
    K = 7
    rng = random.Random(5)
    while True:
        s = rnd(rng, 40)
        if clean([s + s[:K - 2]], K, 40):
            break
    ents = UO.table([s + s[:K - 1]], K)
    assert len(ents) == 40
    (first, text, circ, kc), = summary(ents, K)
    assert circ and first == 0 and kc == 40 and len(text) == 40 + K - 1
    both = s + s + s[:K - 1]
    assert text in both or rcs(text) in both
    assert UO.text_of(ents[0][0], K) == text[:K]
    t = UO.tally(ents, K)
    assert (t["circular"], t["tips"], t["branching"], t["arcs"]) == (1, 0, 0, 80)
    assert UO.fasta(UO.unitigs(ents, K)) == (">0 LN:i:%d KC:i:40 CL:Z:circular\n%s\n" % (len(text), text)).encode()


@pytest.mark.parametrize("K", [5, 6])
def test_hand_joined_to_its_reverse_complement(K):
    """s + rc(s).  Odd K = 2m+1: the k-mers across the joint are pairwise each other's reverse complement, the walk ends in
    a hairpin after m of them: one unitig.  Even K = 2m: the middle one is a palindrome and stands alone."""
    m = K // 2
    rng = random.Random(K)
    while True:                                            # every K-1-mer twice, mirrored, but the middle one of odd K
        s = rnd(rng, 30)
        j = s + rcs(s)
        w = sub_kmers([j], K - 1)                          # ... which is the one that is its own reverse complement
        if len(set(w)) == (len(j) - K + 2 + K % 2) // 2 and sum(x == rcs(x) for x in w) == K % 2:
            break
    ents = UO.table([j], K)
    n = 30 - K + 1
    utgs = summary(ents, K)
    if K % 2:
        assert len(ents) == n + m
        (first, text, circ, kc), = utgs
        assert not circ and len(text) == n + m + K - 1 and kc == 2 * (n + m)
        assert text in s + rcs(s) or rcs(text) in s + rcs(s)
    else:
        assert len(ents) == n + m
        pal = (s + rcs(s))[30 - m:30 + m]
        assert pal == rcs(pal)
        assert sorted(len(t) for _, t, _, _ in utgs) == [K, n + m - 1 + K - 1]
        assert pal in [t for _, t, _, _ in utgs]
        i = [x for x, _ in ents].index(key(pal))
        b = UO.adjacency(ents, K)[i]
        assert b and (b & 15) == (b >> 4)


def test_hand_palindrome_at_even_k():
    ents = sorted([(key("ACGT"), 3), (key("CGTA"), 5)])
    assert UO.adjacency(ents, 4) == [0x11, 0x80]           # ACGT -> CGTA by A from both states; TACG -> ACGT by T
    assert summary(ents, 4) == [(0, "ACGT", False, 3), (2, "CGTA", False, 5)]


# ---- the oracle's own invariants ----

def check_invariants(ents, K, count_range=None):
    g = UO.Graph(ents, K, count_range)
    utgs = g.unitigs()
    nodes = [s >> 1 for u in utgs for s in u[4]]
    assert sorted(nodes) == sorted(g.ord.values())          # every in key, once
    kmers = []
    for first, text, circ, kc, path in utgs:
        assert len(text) == len(path) + K - 1 and first == path[0]
        kmers += [UO.canon(UO.key_of(text[p:p + K]), K) for p in range(len(path))]
        for a, b in zip(path, path[1:]):
            assert g.link(a) == b and g.link(b ^ 1) == a ^ 1
        if circ:
            assert g.link(path[-1]) == path[0] and first == 2 * min(s >> 1 for s in path)
        else:
            assert g.link(path[-1]) is None and g.back(path[0]) is None       # it cannot be extended
            assert path[0] <= path[-1] ^ 1
    assert sorted(kmers) == sorted(g.ord)
    assert [u[0] for u in utgs] == sorted(u[0] for u in utgs)
    return utgs


@pytest.mark.parametrize("K", [3, 4, 5, 6])
def test_invariants_on_every_canonical_kmer(K):
    ents = [(x, 1 + x % 5) for x in sorted({UO.canon(x, K) for x in range(1 << (2 * K))})]
    utgs = check_invariants(ents, K)
    assert len(utgs) == len(ents)                           # every node branches
    check_invariants(ents, K, (2, 3))


@pytest.mark.parametrize("alphabet", ["AC", "ACGT"])
def test_invariants_on_random_soups(alphabet):
    rng = random.Random(len(alphabet))
    shapes = set()
    for it in range(150):
        K = rng.randint(2, 6)
        seqs = [rnd(rng, rng.randint(K, 40), alphabet) for _ in range(rng.randint(1, 4))]
        if it % 3 == 0:                                    # a closed sequence, alone or beside one other
            s = rnd(rng, rng.randint(K, 12), alphabet)
            seqs = seqs[:it % 2] + [s + s[:K - 1]]
        ents = UO.table(seqs, K)
        utgs = check_invariants(ents, K)
        assert summary(UO.table([rcs(s) for s in seqs], K), K) == [u[:4] for u in utgs]        # both strands alike
        check_invariants(ents, K, (1, 1))
        shapes |= {(u[2], len(u[4]) > 1) for u in utgs}
    assert shapes == {(False, False), (False, True), (True, True)}


def test_n50_of_the_oracle():
    assert UO.n50([]) == 0 and UO.n50([7]) == 7 and UO.n50([2, 2, 2, 2]) == 2
    assert UO.n50([10] + [1] * 10) == 10 and UO.n50([10] + [1] * 11) == 1 and UO.n50([10, 9, 1]) == 10 and UO.n50([8, 2, 5, 5]) == 5


# ---- the host functions of the library ----

def test_n50_through_ctypes(built):
    from classpro_amd import _lib
    from classpro_amd.api import unitig_n50
    L = _lib.lib()
    rng = random.Random(50)
    for n in (0, 1, 2, 3, 10, 1000):
        v = [rng.randint(1, 1 << rng.randint(1, 40)) for _ in range(n)]
        assert unitig_n50(v) == UO.n50(v)
        assert unitig_n50(np.array(v, np.int64)) == UO.n50(v)
    assert unitig_n50([0, 0]) == 0 and unitig_n50([(1 << 62), (1 << 62), 5]) == 1 << 62
    assert L.cp_unitig_n50(None, 3) == -1 and b"cp_unitig_n50" in L.cp_last_error()
    assert L.cp_unitig_n50(None, -1) == -1
    bad = np.array([4, -1], np.int64)
    assert L.cp_unitig_n50(bad.ctypes.data, 2) == -1
    assert L.cp_unitig_n50(None, 0) == 0


def test_symbols_are_declared_listed_and_exported(built):
    import ctypes as C
    from classpro_amd import _lib
    L = _lib.lib()
    for name, nargs in (("cp_kmer_sorted_unitigs", 8), ("cp_unitigs_count", 1), ("cp_unitigs_bases", 1),
                        ("cp_unitigs_arrays", 5), ("cp_unitigs_destroy", 1), ("cp_unitig_n50", 2)):
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "Unitigs of sorted k-mers" in hdr and "CP_UTG_WIDTH = 11" in hdr
    for k, name in enumerate(("KEYS", "UNITIGS", "BASES", "CIRCULAR", "LONGEST", "ISOLATED", "TIPS", "BRANCHING", "ARCS")):
        assert "CP_UTG_%s = %d" % (name, k) in hdr
    # a NULL snapshot is refused before the device is touched, and a given `out` is cleared
    t = np.full(11, -7, np.int64)
    h = C.c_void_p(12345)
    assert L.cp_kmer_sorted_unitigs(None, None, t.ctypes.data, None, None, None, None, C.byref(h)) == -1
    assert h.value is None and (t == -7).all()
    assert b"cp_kmer_sorted_unitigs" in L.cp_last_error()
    assert L.cp_kmer_sorted_unitigs(None, None, None, None, None, None, None, None) == -1
    assert L.cp_unitigs_count(None) == 0 and L.cp_unitigs_bases(None) == 0
    assert L.cp_unitigs_arrays(None, None, None, None, None) == -1 and b"cp_unitigs_arrays" in L.cp_last_error()
    L.cp_unitigs_destroy(None)


# ---- tabunitig's errors ----

K0 = 12


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("unitig_host"))
    ents = KO.table(mixed_reads(K0, 5), K0)
    fastk.write_fastk_ktab(d, "tab", K0, 1, [x for x, _ in ents], [c for _, c in ents], 3)
    return d


def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    a, out = os.path.join(d, "tab"), os.path.join(d, "out")
    before = listing(d)
    cases = [((), USAGE), ((a, out, out), USAGE), (("-v",), USAGE),
             (("-q", a), "tabunitig: -q is an illegal option\n"),
             (("-vc", a, out), "tabunitig: -c is an illegal option\n"),
             (("-x3", a, out), "tabunitig: -x is an illegal option\n"),
             ((a + ":0-3", out), "tabunitig: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a + ":5-2", out), "tabunitig: Count range of %s needs 1 <= lo <= hi (5-2)\n" % a),
             ((a + ":5-2",), "tabunitig: Count range of %s needs 1 <= lo <= hi (5-2)\n" % a),
             ((a, os.path.join(d, "no_such_dir", "out")),
              "tabunitig: Cannot open %s/no_such_dir/out.unitigs.fa for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".unitigs.fa")
    before = listing(d)
    r = run(a, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabunitig: Cannot open %s.unitigs.fa for 'w'\n" % out)
    assert listing(d) == before


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)
    before = listing(d)
    r = run("-v", os.path.join(d, "tab"), os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabunitig: " + msg), how
    assert listing(d) == before

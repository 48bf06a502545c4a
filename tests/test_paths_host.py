"""Reads through the unitig graph, the part that needs no GPU: the oracle of tests/path_oracle.py on cases written out by hand
(the SNP bubble, a read with one substitution, a closed chain run round), the three properties Joins, Spelling and Mirror
on the complete k-mer sets of K = 5 and 6 and on random two-haplotype graphs, `path_walks` against the oracle, the kernels'
words, summaries and walk on the host (tests/kp_sum_check.cpp under AddressSanitizer and UBSan), the exports, the argument
errors of cp_kmer_sorted_read_paths, cp_count_nonzero and `read_paths` that come before the device, and every error tabpath
reports before it touches the GPU (exact stderr, exit 1, nothing on stdout, no file created).  Everything is integers and
bytes: the tolerance is zero."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import path_oracle as PO
import unitig_oracle as UO
from conftest import ROOT, build_if_changed
from test_readhits_host import good                        # noqa: F401  (the fixture: two tables at K = 12, one at K = 8, a source)
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil
from test_unitig_host import clean, rcs, rnd, simple

TOOL = os.path.join(ROOT, "classpro_amd", "tabpath")
USAGE = ("Usage: tabpath [-v] [-g] [-b<int(67108864)>] [-o<out_root>] <table>[.ktab][:<lo>-<hi>] "
         "<source>[.db|.dam|.f[ast][aq][.gz]]\n")


def bubble():
    """The SNP bubble of test_gpu_unitig_graph.hand_cases(): (h1, h2, K)."""
    rng = random.Random(3)
    K = 7
    while True:
        left, right = rnd(rng, 12), rnd(rng, 12)
        h1, h2 = left + "A" + right, left + "C" + right
        if len(UO.table([h1, h2], K)) == 26 and clean([h1, h2], K, 20 + K - 1):
            return h1, h2, K


def haplotypes(rng, K, n=300, snps=4):
    """Two haplotypes that differ at a few places, a hairpin, a homopolymer run and a sequence joined to its reverse
    complement: a graph with bubbles, tips, self arcs and arcs onto the other strand."""
    h1 = rnd(rng, n)
    h2 = list(h1)
    for p in rng.sample(range(K, n - K), snps):
        h2[p] = rng.choice([c for c in "ACGT" if c != h1[p]])
    s = rnd(rng, 3 * K)
    return [h1, "".join(h2), "AT" * K, "A" * (2 * K), s + rcs(s)]


def random_reads(rng, seqs, n, longest):
    """Substrings of the sequences and of their reverse complements, some with an N or a substitution, some random."""
    reads = []
    for _ in range(n):
        s = rng.choice(seqs)
        s = rcs(s) if rng.random() < 0.5 else s
        a = rng.randrange(len(s))
        r = list(s[a:a + rng.randrange(1, longest + 1)])
        what = rng.random()
        if what < 0.15:
            r[rng.randrange(len(r))] = "N"
        elif what < 0.35:
            r[rng.randrange(len(r))] = rng.choice("ACGT")
        elif what < 0.4:
            r = list(rnd(rng, len(r)))
        reads.append("".join(r))
    return reads


# ---- the oracle on cases written out by hand ----

def test_oracle_on_the_snp_bubble():
    h1, h2, K = bubble()
    P = PO.Paths(UO.table([h1, h2], K), K)
    assert len(P.utgs) == 4 and sorted(P.nodes) == [6, 6, 7, 7]
    segs = P.segments(h1)
    assert [(f, n, fl) for f, n, _, _, _, fl in segs] == [(0, 6, 0), (6, 7, 1), (13, 6, 1)]      # left flank, one arm, right flank
    assert [P.nodes[x >> 1] for _, _, x, _, _, _ in segs] == [6, 7, 6] and all(s[3] == 0 for s in segs)
    other = P.segments(h2)
    assert segs[0][2] == other[0][2] and segs[2][2] == other[2][2] and segs[1][2] >> 1 != other[1][2] >> 1
    back = P.segments(rcs(h1))
    assert [(f, n, x, q, fl) for f, n, x, q, _, fl in back] == [(0, 6, segs[2][2] ^ 1, 0, 0), (6, 7, segs[1][2] ^ 1, 0, 1),
                                                                  (13, 6, segs[0][2] ^ 1, 0, 1)]
    PO.check_properties(P, h1)
    off, all_segs, t, cov, sup = P.batch([h1, rcs(h1), h2[3:20], "ACG", ""])
    assert off == [0, 3, 6, 9, 9, 9] and t["positions"] == 19 + 19 + 11 and t["present"] == t["positions"]
    assert (t["segments"], t["joined"], t["walks"]) == (9, 6, 3)
    assert sum(cov) == t["present"] and sum(sup) == t["joined"] and max(sup) == 1
    assert P.walks(segs) == [(0, 25, [s[2] for s in segs], 25, 0)]
    name = P.gaf([h1], ["r"]).decode().split("\t")
    assert name[:5] == ["r", "25", "0", "25", "+"] and name[6:] == ["25", "0", "25", "25", "25", "255\n"]


def test_oracle_on_a_substitution_and_a_closed_chain():
    K = 9
    s = simple(random.Random(11), 80, K)
    P = PO.Paths(UO.table([s], K), K)
    assert len(P.utgs) == 1 and P.segments(s)[0][:2] == (0, 72) and len(P.segments(s)) == 1
    p = 40
    for c in "ACGT":                                       # a substitution whose K new k-mers are not in the table
        read = s[:p] + c + s[p + 1:]
        if c != s[p] and all(st == PO.ABSENT for st in P.steps(read)[p - K + 1:p + 1]):
            break
    segs = P.segments(read)
    assert [(f, n, fl) for f, n, _, _, _, fl in segs] == [(0, p - K + 1, 0), (p + 1, 72 - p - 1, 0)]       # a gap of K positions
    assert len(P.walks(segs)) == 2 and P.batch([read])[2]["absent"] == K
    PO.check_properties(P, read)
    with_n = s[:p] + "N" + s[p + 1:]
    assert P.batch([with_n])[2]["other"] == K and [x[:2] for x in P.segments(with_n)] == [x[:2] for x in segs]
    # a closed chain of n nodes run round three times: three segments, the later two joined by the self arc
    n = 12
    while True:
        c = rnd(random.Random(n), n)
        ring = c + c[:K - 1]
        if clean([ring], K, n):
            break
        n += 1
    P = PO.Paths(UO.table([ring], K), K)
    assert len(P.utgs) == 1 and P.utgs[0][2] and P.L.arcs[0][::2] == (0, 0)
    for read in (c * 3 + c[:K - 1], rcs(c * 3 + c[:K - 1])):
        segs = P.segments(read)
        assert sum(x[1] for x in segs) == 3 * n and [x[5] for x in segs] == [0] + [1] * (len(segs) - 1)
        assert all(x[3] == 0 and x[1] == n for x in segs[1:-1]) and len(P.walks(segs)) == 1
        PO.check_properties(P, read)
    assert sorted(P.batch([c * 3 + c[:K - 1]])[4]) == [0, len(P.segments(c * 3 + c[:K - 1])) - 1]      # one of the two self arcs


# ---- the three properties ----

@pytest.mark.parametrize("K", [5, 6])
def test_properties_on_every_canonical_kmer(K):
    """Every head is joined but the first: the complete set has every arc.  K = 6 holds palindromes."""
    ents = [(x, 1 + x % 7) for x in sorted({UO.canon(x, K) for x in range(1 << (2 * K))})]
    rng = random.Random(K)
    for count_range in (None, (2, 5)):
        P = PO.Paths(ents, K, count_range)
        reads = [rnd(rng, rng.randrange(K, 120)) for _ in range(40)] + ["ACGT" * 10, "A" * 30, "AT" * 20, "ACGTACGTNACGTACGTAC"]
        for read in reads:
            PO.check_properties(P, read)                   # segments() itself asserts Joins
        _, segs, t, cov, sup = P.batch(reads)
        assert sum(cov) == t["present"] and sum(sup) == t["joined"]
        if count_range is None:
            assert t["absent"] == 0 and t["walks"] == len(reads) + 1       # the N cuts one read in two


@pytest.mark.parametrize("K", [5, 8, 12])
def test_properties_on_random_graphs(K):
    rng = random.Random(K)
    for count_range in (None, (2, None)):
        seqs = haplotypes(rng, K)
        P = PO.Paths(UO.table(seqs, K), K, count_range)
        reads = random_reads(rng, seqs, 150, 120)
        for read in reads:
            PO.check_properties(P, read)
        _, segs, t, cov, sup = P.batch(reads)
        assert sum(cov) == t["present"] and sum(sup) == t["joined"] > 0 and t["absent"] > 0 and t["other"] > 0


# ---- path_walks ----

def test_path_walks_against_the_oracle():
    from classpro_amd.api import path_walks
    K = 8
    rng = random.Random(2)
    seqs = haplotypes(rng, K)
    P = PO.Paths(UO.table(seqs, K), K)
    reads = random_reads(rng, seqs, 60, 150) + ["", "ACG"]
    off, segs, _, _, _ = P.batch(reads)
    cols = {k: [s[i] for s in segs] for i, k in enumerate(PO.FIELDS)}
    want = []
    for r, read in enumerate(reads):
        for f, e, xs, plen, q in P.walks(P.segments(read, r)):
            want.append((r, f, e, "".join("%s%d" % ("<" if x & 1 else ">", x >> 1) for x in xs), plen, q))
    assert path_walks(off, cols, P.nodes, K) == want and len(want) > len(reads) // 2
    assert any(len(w[3].replace("<", ">").split(">")) > 3 for w in want)
    assert path_walks([0, 0], {k: [] for k in PO.FIELDS}, [], K) == []
    cols["read"][0] += 1
    with pytest.raises(ValueError):
        path_walks(off, cols, P.nodes, K)


# ---- the words, the summaries and the walk of the kernels, on the host ----

def test_summary_algebra_on_the_host():
    """classpro_amd/csrc/kp_sum.h compiles for the host: tests/kp_sum_check.cpp runs the three passes of kmer_paths.hip over
    random reads with small lanes and blocks, under AddressSanitizer and UBSan, against a plain loop."""
    src = os.path.join(ROOT, "tests", "kp_sum_check.cpp")
    exe = os.path.join(ROOT, "tests", "_kp_sum_check")
    inc = os.path.join(ROOT, "classpro_amd", "csrc")
    build_if_changed(exe, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           "-o", exe, src], [src, os.path.join(inc, "kp_sum.h")])
    r = subprocess.run([exe, "20000"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (0, "ok 20000\n"), r.stdout + r.stderr


# ---- the exports and the errors before the device ----

def test_library_exports_and_argument_errors(built):
    from classpro_amd import _lib
    from classpro_amd.api import SortedKmers, Unitigs
    L = _lib.lib()
    assert {"cp_kmer_sorted_read_paths", "cp_count_nonzero"} <= set(_lib.SYMBOLS)
    assert len(L.cp_kmer_sorted_read_paths.argtypes) == 17 and len(L.cp_count_nonzero.argtypes) == 4
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "typedef struct cp_path_seg { int64_t first, x; int32_t n, q, read, flags; } cp_path_seg;" in hdr
    assert ("enum { CP_PATH_POSITIONS = 0, CP_PATH_PRESENT = 1, CP_PATH_ABSENT = 2, CP_PATH_OTHER = 3, CP_PATH_SEGMENTS = 4,\n"
            "       CP_PATH_JOINED = 5, CP_PATH_WALKS = 6, CP_PATH_WIDTH = 7 };") in hdr
    assert "Reads through the unitig graph" in hdr and SortedKmers.PATH_TALLY == PO.TALLY
    t = C.c_int64(7)
    tally = (C.c_int64 * 7)()
    assert L.cp_kmer_sorted_read_paths(None, None, None, None, None, None, None, 0, 0, None, 0, None, None, None, tally, C.byref(t), None) == -1
    assert b"cp_kmer_sorted_read_paths" in L.cp_last_error()
    assert L.cp_count_nonzero(None, 0, None, None) == -1 and b"cp_count_nonzero" in L.cp_last_error()
    assert L.cp_count_nonzero(None, -1, C.byref(t), None) == -1 and L.cp_count_nonzero(None, 5, C.byref(t), None) == -1
    assert L.cp_count_nonzero(None, 0, C.byref(t), None) == 0 and t.value == 0
    S = SortedKmers.__new__(SortedKmers)
    S.s = None
    with pytest.raises(ValueError):
        S.read_paths(None, None)
    S.s, S.K, S.n, S.device = 1, 9, 0, "cuda:0"            # the checks of U come before anything is called
    try:
        with pytest.raises(ValueError):
            S.read_paths(None, None)
        U = Unitigs(L, "cuda:0", 9, None, {"unitigs": 0, "bases": 0}, None, None, None)
        with pytest.raises(ValueError):
            S.read_paths(U, None)
    finally:
        S.s = None


# ---- tabpath before the GPU ----

def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    a, b, src = os.path.join(d, "tab"), os.path.join(d, "o:ther.ktab"), os.path.join(d, "reads")
    before = listing(d)
    missing = "tabpath: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d
    cases = [((), USAGE), ((a,), USAGE), ((a, b, src), USAGE), (("-v", "-g", "-b5", "-oout"), USAGE), (("-g", a), USAGE),
             (("-x", a, src), "tabpath: -x is an illegal option\n"),
             (("-vq", a, src), "tabpath: -q is an illegal option\n"),
             (("-gm", "-oout", a, src), "tabpath: -m is an illegal option\n"),
             (("-v", "-T4", a, src), "tabpath: -T is an illegal option\n"),
             (("-bx", a, src), "tabpath: -b 'x' argument is not an integer\n"),
             (("-b", a, src), "tabpath: -b '' argument is not an integer\n"),
             (("-b1e6", a, src), "tabpath: -b '1e6' argument is not an integer\n"),
             (("-b0", a, src), "tabpath: Bases per device batch must be positive (0)\n"),
             (("-b-1", "-g", a, src), "tabpath: Bases per device batch must be positive (-1)\n"),
             (("-g", a, src), "tabpath: -g needs -o\n"),
             (("-vg", "-o", a + ":0-3", src), "tabpath: -g needs -o\n"),
             ((a + ":0-3", src), "tabpath: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((b + ":5-2", src), "tabpath: Count range of %s needs 1 <= lo <= hi (5-2)\n" % b),
             ((a + ":3", src), "tabpath: Cannot open %s:3.ktab [errno=2]\n" % a),              # no range: part of the path
             ((a, os.path.join(d, "nothing")), missing),
             (("-g", "-o" + os.path.join(d, "out"), b + ":2-", os.path.join(d, "nothing")), missing),
             (("-o" + os.path.join(d, "no_such_dir", "out"), a, src), "tabpath: Cannot open %s/no_such_dir/out.gaf for 'w'\n" % d),
             (("-g", "-o" + os.path.join(d, "no_such_dir", "out"), a, src),
              "tabpath: Cannot open %s/no_such_dir/out.gaf for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(os.path.join(d, "out.gfa"))                   # a directory has the second file's name: the first is not left behind
    before = listing(d)
    r = run("-g", "-o" + os.path.join(d, "out"), a, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabpath: Cannot open %s/out.gfa for 'w'\n" % d)
    assert listing(d) == before
    os.mkdir(os.path.join(d, "dir.gaf"))
    before = listing(d)
    r = run("-o" + os.path.join(d, "dir"), a, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabpath: Cannot open %s/dir.gaf for 'w'\n" % d)
    assert listing(d) == before
    unreadable = os.path.join(d, "locked.fasta")
    open(unreadable, "w").write(">r\nACGT\n")
    os.chmod(unreadable, 0)
    if not os.access(unreadable, os.R_OK):                 # root reads everything: nothing to see then
        before = listing(d)
        r = run("-g", "-o" + os.path.join(d, "out2"), a, unreadable)
        assert (r.returncode, r.stdout) == (1, "") and r.stderr.startswith("tabpath: Cannot open %s" % unreadable)
        assert listing(d) == before


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    r = run("-g", "-o" + os.path.join(d, "out"), os.path.join(d, "tab"), os.path.join(d, "reads.fasta"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabpath: " + msg), how
    assert listing(d) == before

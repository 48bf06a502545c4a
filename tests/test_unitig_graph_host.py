"""tabgraph and the links between unitigs without a GPU: tests/unitig_graph_oracle.py against cases worked out by hand, with
the expected arcs written out, and against its own invariants (mirror symmetry off palindromes, the LINKS identity, the
K-1 overlap of the spelled strings along every arc, the k-mer of every arc is in the table), the symbols' declarations and
the returns that need no device, and every error tabgraph reports before it touches the device (exact message, exit
status 1, empty stdout, no file created)."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import ktab_oracle as KO
import unitig_graph_oracle as GO
import unitig_oracle as UO
from conftest import ROOT, build_if_changed
from test_gpu_ktab import mixed_reads
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil
from test_unitig_host import clean, key, rcs, rnd

TOOL = os.path.join(ROOT, "classpro_amd", "tabgraph")
USAGE = "Usage: tabgraph [-v] <table>[.ktab][:<lo>-<hi>] <out_root>\n"
A, C_, G, T = 0, 1, 2, 3


# ---- the oracle against the cases worked out by hand ----

def test_hand_single_kmer():
    ents = [(key("ACCGT"), 7)]
    L = GO.Links(ents, 5)
    assert L.arcs == [] and L.comp == [0] and L.loff() == [0, 0, 0]
    assert L.tally() == dict(links=0, dead_ends=2, tip_unitigs=0, isolated_unitigs=1, self=0, components=1, largest_bases=5)
    assert L.gfa() == b"H\tVN:Z:1.0\nS\t0\tACCGT\tLN:i:5\tKC:i:7\tco:i:0\n"
    assert L.line() == ("tabgraph: 1 k-mers, 1 unitigs, 5 bases, 0 circular, longest 5, N50 5\n"
                        "tabgraph: 0 links, 2 dead ends, 0 tip unitigs, 1 components, largest 5 bases\n")


def test_hand_homopolymer():
    """AAAA -> AAAA by A as spelled, TTTT -> TTTT by T reversed: a self arc on either strand."""
    ents = UO.table(["A" * 60], 21)
    assert ents == [(0, 40)]
    L = GO.Links(ents, 21)
    assert L.arcs == [(0, A, 0), (1, T, 1)] and L.loff() == [0, 1, 2]
    t = L.tally()
    assert (t["links"], t["self"], t["dead_ends"], t["components"], t["largest_bases"]) == (2, 2, 0, 1, 21)
    assert L.gfa() == ("H\tVN:Z:1.0\nS\t0\t%s\tLN:i:21\tKC:i:40\tco:i:0\nL\t0\t+\t0\t+\t20M\nL\t0\t-\t0\t-\t20M\n" % ("A" * 21)).encode()


def test_hand_dinucleotide_hairpin_and_palindrome():
    """AT x 30.  K = 21: one node, ATA..A, whose successor by T is its own reverse complement: a hairpin, 2u -> 2u+1 and,
    from the other strand by A, 2u+1 -> 2u.  K = 20: AT x 10 and TA x 10 are palindromes, one-node unitigs spelled in their
    even state; both orientations of each carry the same arc, and every arc lands on '+'."""
    ents = UO.table(["AT" * 30], 21)
    assert len(ents) == 1
    L = GO.Links(ents, 21)
    assert L.arcs == [(0, T, 1), (1, A, 0)]
    assert (L.tally()["self"], L.tally()["components"]) == (2, 1)
    ents = UO.table(["AT" * 30], 20)
    assert [UO.text_of(x, 20) for x, _ in ents] == ["AT" * 10, "TA" * 10]
    L = GO.Links(ents, 20)
    assert [u[0] for u in L.utgs] == [0, 2]
    assert L.arcs == [(0, A, 2), (1, A, 2), (2, T, 0), (3, T, 0)] and L.comp == [0, 0]
    t = L.tally()
    assert (t["links"], t["self"], t["dead_ends"], t["components"], t["largest_bases"]) == (4, 0, 0, 1, 40)


def test_hand_k_plus_one_bases():
    """ACGGTC at K = 5 is one unitig of two nodes: nothing follows either end."""
    ents = UO.table(["ACGGTC"], 5)
    L = GO.Links(ents, 5)
    assert L.n == 1 and L.arcs == []
    assert L.tally() == dict(links=0, dead_ends=2, tip_unitigs=0, isolated_unitigs=1, self=0, components=1, largest_bases=6)


def test_hand_snp_bubble():
    """Two flanks and two arms.  In some orientation the left flank reaches both arms and both arms reach the right
    flank: 4 arcs, and their 4 mirror images."""
    K = 7
    rng = random.Random(3)
    while True:
        left, right = rnd(rng, 12), rnd(rng, 12)
        h1, h2 = left + "A" + right, left + "C" + right
        ents = UO.table([h1, h2], K)
        if len(ents) == 26 and clean([h1, h2], K, 20 + K - 1):
            break
    L = GO.Links(ents, K)
    assert L.n == 4 and len(L.arcs) == 8 and L.comp == [0, 0, 0, 0]
    flank = [u for u in range(4) if len(L.utgs[u][1]) == 12]
    arm = [u for u in range(4) if len(L.utgs[u][1]) == 2 * K - 1]
    assert len(flank) == 2 and len(arm) == 2
    deg = [L.loff()[x + 1] - L.loff()[x] for x in range(8)]
    for u in flank:                                        # one end of a flank forks, the other is dead
        assert sorted((deg[2 * u], deg[2 * u + 1])) == [0, 2]
    for u in arm:
        assert (deg[2 * u], deg[2 * u + 1]) == (1, 1)
    for x, c, y in L.arcs:
        assert ((x >> 1) in flank) != ((y >> 1) in flank) and (y ^ 1, x ^ 1) in {(a, b) for a, _, b in L.arcs}
    t = L.tally()
    assert (t["links"], t["dead_ends"], t["tip_unitigs"], t["isolated_unitigs"], t["self"], t["components"]) == (8, 2, 2, 0, 0, 1)
    assert t["largest_bases"] == 2 * 12 + 2 * (2 * K - 1)


def test_hand_closed_sequence():
    K = 7
    rng = random.Random(5)
    while True:
        s = rnd(rng, 40)
        if clean([s + s[:K - 2]], K, 40):
            break
    ents = UO.table([s + s[:K - 1]], K)
    L = GO.Links(ents, K)
    text = L.utgs[0][1]
    assert L.n == 1 and L.utgs[0][2]
    assert L.arcs == [(0, "ACGT".index(text[K - 1]), 0), (1, "ACGT".index(rcs(text)[K - 1]), 1)]       # exactly the two self arcs
    assert text[-(K - 1):] == text[:K - 1]
    t = L.tally()
    assert (t["links"], t["self"], t["dead_ends"], t["components"]) == (2, 2, 0, 1)


def test_hand_joined_to_its_reverse_complement():
    """s + rc(s) at K = 5: one unitig that ends in a hairpin; that end reaches its own other strand."""
    K = 5
    rng = random.Random(K)
    while True:
        s = rnd(rng, 30)
        j = s + rcs(s)
        ents = UO.table([j], K)
        L = GO.Links(ents, K)
        if L.n == 1 and not L.utgs[0][2] and len(L.arcs) == 1:                  # ... whose other end is no hairpin too
            break
    text = L.utgs[0][1]
    (x, c, y), = L.arcs
    assert y == x ^ 1                                      # 2u -> 2u+1 or 2u+1 -> 2u, whichever end the hairpin is
    string = rcs(text) if x & 1 else text
    assert rcs(string)[:K] == string[-(K - 1):] + "ACGT"[c]
    t = L.tally()
    assert (t["links"], t["self"], t["dead_ends"], t["tip_unitigs"]) == (1, 1, 1, 1)


# ---- the oracle's own invariants ----

def check_invariants(ents, K, count_range=None):
    L = GO.Links(ents, K, count_range)
    g, arcs = L.g, L.arcs
    assert arcs == sorted(arcs) and len({(x, c) for x, c, _ in arcs}) == len(arcs)
    string = lambda x: rcs(L.utgs[x >> 1][1]) if x & 1 else L.utgs[x >> 1][1]
    pal = [len(u[4]) == 1 and g.palindromic(u[4][0]) for u in L.utgs]
    have = {(x, y) for x, _, y in arcs}
    for x, c, y in arcs:
        a, b = string(x), string(y)
        assert a[-(K - 1):] == b[:K - 1] and b[K - 1] == "ACGT"[c]                  # the overlap of K-1 bases
        assert UO.canon(UO.key_of(a[-(K - 1):] + "ACGT"[c]), K) in g.ord            # the k-mer of the arc is in
        if pal[y >> 1]:
            assert not y & 1                                                        # into a palindrome: on '+'
        if not pal[x >> 1] and not pal[y >> 1]:
            assert (y ^ 1, x ^ 1) in have                                           # the mirror arc
    for u in range(L.n):
        if pal[u]:
            assert [(c, y) for x, c, y in arcs if x == 2 * u] == [(c, y) for x, c, y in arcs if x == 2 * u + 1]
        if L.utgs[u][2]:
            assert [(x, y) for x, _, y in arcs if x >> 1 == u or y >> 1 == u] == [(2 * u, 2 * u), (2 * u + 1, 2 * u + 1)]
    ut = UO.tally(ents, K, count_range, L.utgs)
    assert len(arcs) == ut["arcs"] - 2 * (ut["keys"] - ut["unitigs"])               # the LINKS identity
    for x, _, y in arcs:
        assert L.comp[x >> 1] == L.comp[y >> 1]
    assert all(L.comp[c] == c and c <= u for u, c in enumerate(L.comp))
    return L


@pytest.mark.parametrize("K", [4, 5, 6])
def test_invariants_on_every_canonical_kmer(K):
    ents = [(x, 1 + x % 5) for x in sorted({UO.canon(x, K) for x in range(1 << (2 * K))})]
    L = check_invariants(ents, K)
    assert len(L.arcs) == 8 * len(ents) and L.tally()["components"] == 1           # every end has four arcs
    check_invariants(ents, K, (2, 3))


@pytest.mark.parametrize("alphabet", ["AC", "ACGT"])
def test_invariants_on_random_soups(alphabet):
    rng = random.Random(len(alphabet))
    seen = set()
    for it in range(150):
        K = rng.randint(2, 6)
        seqs = [rnd(rng, rng.randint(K, 40), alphabet) for _ in range(rng.randint(1, 4))]
        if it % 3 == 0:                                    # a closed sequence, alone or beside one other
            s = rnd(rng, rng.randint(K, 12), alphabet)
            seqs = seqs[:it % 2] + [s + s[:K - 1]]
        ents = UO.table(seqs, K)
        L = check_invariants(ents, K)
        M = GO.Links(UO.table([rcs(s) for s in seqs], K), K)
        assert M.arcs == L.arcs and M.comp == L.comp        # both strands alike
        check_invariants(ents, K, (1, 1))
        t = L.tally()
        seen |= {k for k in GO.TALLY if t[k] > 0} | ({"many"} if t["components"] > 1 else set())
    assert seen == set(GO.TALLY) | {"many"}


# ---- the host side of the library ----

def test_symbols_are_declared_listed_and_exported(built):
    import ctypes as C
    from classpro_amd import _lib
    L = _lib.lib()
    for name, nargs in (("cp_kmer_sorted_unitig_links", 9), ("cp_unitig_graph_links", 1), ("cp_unitig_graph_arrays", 5),
                        ("cp_unitig_graph_destroy", 1)):
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == nargs
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "Links between unitigs" in hdr and "CP_UGL_WIDTH = 8" in hdr and "CP_UTG_WIDTH = 11" in hdr
    for k, name in enumerate(("LINKS", "DEAD_ENDS", "TIP_UNITIGS", "ISOLATED_UNITIGS", "SELF", "COMPONENTS", "LARGEST_BASES", "ROUNDS")):
        assert "CP_UGL_%s = %d" % (name, k) in hdr
    from classpro_amd.api import Unitigs
    assert Unitigs.LINK_TALLY[:7] == GO.TALLY and len(Unitigs.LINK_TALLY) == 8
    # a NULL snapshot is refused before the device is touched, and a given `out` is cleared
    t = np.full(8, -7, np.int64)
    h = C.c_void_p(12345)
    assert L.cp_kmer_sorted_unitig_links(None, None, None, None, None, t.ctypes.data, 1, None, C.byref(h)) == -1
    assert h.value is None and (t == -7).all()
    assert b"cp_kmer_sorted_unitig_links" in L.cp_last_error()
    assert L.cp_unitig_graph_links(None) == 0
    assert L.cp_unitig_graph_arrays(None, None, None, None, None) == -1 and b"cp_unitig_graph_arrays" in L.cp_last_error()
    L.cp_unitig_graph_destroy(None)


# ---- the windows of the FASTA and GFA writers on the host ----

def test_windows_on_the_host():
    """classpro_amd/csrc/host/unitig_window.h compiles for the host: tests/window_check.cpp runs its Window and its two
    writers with a fetch from host arrays at windows of 1 to 4 elements -- a unitig that ends at a refill, starts at one,
    spans two and three windows; 5 unitigs and 7 links at unitig windows of 1 and 2 and link windows of 1, 2 and 3, with and
    without the RC tags; no unitig at all -- under AddressSanitizer and UBSan, byte for byte against a writer that holds
    everything."""
    src = os.path.join(ROOT, "tests", "window_check.cpp")
    exe = os.path.join(ROOT, "tests", "_window_check")
    inc = os.path.join(ROOT, "classpro_amd", "csrc")
    build_if_changed(exe, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           "-o", exe, src], [src, os.path.join(inc, "host", "unitig_window.h")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (0, "ok\n", "")


# ---- tabgraph's errors ----

K0 = 12


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("unitig_graph_host"))
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
    cases = [((), USAGE), ((a,), USAGE), ((a, out, out), USAGE), (("-v",), USAGE), (("-v", a), USAGE),
             (("-q", a, out), "tabgraph: -q is an illegal option\n"),
             (("-vc", a, out), "tabgraph: -c is an illegal option\n"),
             (("-x3", a, out), "tabgraph: -x is an illegal option\n"),
             ((a + ":0-3", out), "tabgraph: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a + ":5-2", out), "tabgraph: Count range of %s needs 1 <= lo <= hi (5-2)\n" % a),
             ((a, os.path.join(d, "no_such_dir", "out")), "tabgraph: Cannot open %s/no_such_dir/out.gfa for 'w'\n" % d),
             ((a, os.path.join(a + ".ktab", "out")), "tabgraph: Cannot open %s.ktab/out.gfa for 'w'\n" % a)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".gfa")                                 # a directory in its place
    before = listing(d)
    r = run(a, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabgraph: Cannot open %s.gfa for 'w'\n" % out)
    assert listing(d) == before
    if os.geteuid() != 0:                                  # a file that may not be written (root may write any)
        ro = os.path.join(d, "ro")
        open(ro + ".gfa", "w").write("kept\n")
        os.chmod(ro + ".gfa", 0o444)
        before = listing(d)
        r = run(a, ro)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabgraph: Cannot open %s.gfa for 'w'\n" % ro)
        assert listing(d) == before and open(ro + ".gfa").read() == "kept\n"


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)
    before = listing(d)
    r = run("-v", os.path.join(d, "tab"), os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabgraph: " + msg), how
    assert listing(d) == before

"""Phasing heterozygous sites from reads without a GPU: tests/phase_oracle.py on cases whose answer follows from how they are
built, classpro_amd/csrc/ph_rule.h on the host under AddressSanitizer and UBSan against the oracle, the argument errors of
the five library calls that come before the device, and every error `tabphase` reports before the GPU is touched.  The
tolerance is zero."""
import os
import random
import shutil
import subprocess

import pytest

import hetpairs_oracle as HO
import phase_oracle as PO
from conftest import ROOT, build_if_changed
from test_tabprof_host import NO_GPU, SPOILED, good, listing, spoil          # noqa: F401  (good: a table at K = 12 and a source)

TOOL = os.path.join(ROOT, "classpro_amd", "tabphase")
USAGE = ("Usage: tabphase [-v] [-m<int(2)>] [-b<int(67108864)>] [-T<int(4)>]\n"
         "                <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]] [<out_root>]\n")
MIN_SUPPORT = 2


# ---- the oracle on cases whose answer is known ----

def test_hand_sites_and_links():
    K = 5                                                  # AACAA ~ AAGAA and ACCCA ~ ACTCA at the centre base; CCGCC has no partner
    P = sorted((PO.encode(s), c) for s, c in ((b"AACAA", 3), (b"AAGAA", 4), (b"CCGCC", 2), (b"ACCCA", 5), (b"ACTCA", 6)))
    mate, mark, ns = PO.sites(P, K)
    by = {PO.decode(x, K): (m, k) for (x, _), m, k in zip(P, mate, mark)}
    assert ns == 2 and by[b"CCGCC"] == (-1, -1)
    assert by[b"AACAA"][1] == 0 and by[b"AAGAA"][1] == 1 and by[b"ACCCA"][1] == 2 and by[b"ACTCA"][1] == 3
    # one read: site 0 allele 0, an N, site 1 allele 1, site 1 again on the other strand, then a read of its own
    reads = [b"AACAA" + b"N" + b"ACTCA" + b"G" + b"TGAGT", b"AAGAA", b"ACG", b""]
    links, tally = PO.read_links(P, mark, reads, K)
    assert links == [PO.link_key(0, 0, 1, 1)] == [0 << 32 | 1 << 1 | 1] and tally == [4, 1, 1]


def test_hand_forests():
    key = PO.link_key
    # a frustrated triangle with margins 3, 2, 1: the margin-1 edge is the conflict
    counts = {key(0, 0, 1, 0): 3, key(1, 0, 2, 0): 2, key(0, 0, 2, 1): 1}
    block, side, t = PO.forest(counts, 4, 1)
    assert block == [0, 0, 0, 3] and side == [0, 0, 0, 0]
    assert (t["kept"], t["forest"], t["conflicts"], t["blocks"], t["single"], t["largest"]) == (3, 2, 1, 1, 1, 3)
    # equal margins: the tie goes by (s, t), so (1, 2) is the conflict
    counts = {key(0, 0, 1, 1): 2, key(0, 0, 2, 0): 2, key(1, 0, 2, 0): 2}
    block, side, t = PO.forest(counts, 3, 2)
    assert side == [0, 1, 0] and t["conflicts"] == 1 and t["rounds"] == 1
    # the clamp: 70000 and 65535 are one class, so the smaller (s, t) comes first
    counts = {key(0, 0, 1, 0): 65535, key(0, 0, 2, 0): 70000, key(1, 0, 2, 1): 70000}
    block, side, t = PO.forest(counts, 3, 2)
    assert side == [0, 0, 0] and t["conflicts"] == 1
    # weak, tied, a pair with only its trans key, bad keys
    counts = {key(0, 0, 1, 0): 1, key(2, 0, 3, 0): 2, key(2, 0, 3, 1): 2, key(4, 0, 5, 1): 2, 3 << 32 | 2 << 1: 9, 1 << 32 | 9 << 1: 9}
    block, side, t = PO.forest(counts, 6, 2)
    assert (t["edges"], t["weak"], t["tied"], t["kept"], t["bad"]) == (3, 1, 1, 1, 2)
    assert block == [0, 1, 2, 3, 4, 4] and side == [0, 0, 0, 0, 0, 1] and t["single"] == 4


def conditions(h1, h2, snps, reads_per_hap, K, rlen=3000, step=500):
    """The conditions under which the claim of the first-principles case holds, checked on the CPU."""
    seen = set()
    for h in (h1, h2):                                     # no (K-1)-mer of the two haplotypes repeats, on either strand
        for j in range(len(h) - K + 2):
            w = h[j:j + K - 1]
            c = min(w, PO.revcomp_seq(w))
            if h is h2 and h1[j:j + K - 1] == w:
                continue                                   # the same place of the other haplotype
            assert c not in seen
            seen.add(c)
    starts = range(0, len(h1) - rlen + 1, step)
    for a, b in zip(snps, snps[1:]):                       # every adjacent SNP pair is spanned, k-mers and all
        n = sum(s <= a - K + 1 and b + K - 1 < s + rlen for s in starts)
        assert n >= MIN_SUPPORT
    assert len(snps) > 100


@pytest.mark.parametrize("K", [21, 20])
def test_first_principles(K):
    """Two haplotypes with SNPs more than K apart, error-free tiled reads: one block, no conflict, nothing tied, and A is
    exactly the marker k-mers of one haplotype, B those of the other.  At K = 20 every SNP gives two sites."""
    rng = random.Random(K)
    h1, h2, snps = PO.genome(rng, K)
    reads = PO.tiled_reads((h1, h2))
    conditions(h1, h2, snps, len(reads) // 2, K)
    T = PO.table(reads, K)
    r = PO.phase(T, K, [reads[:40], reads[40:]], None, MIN_SUPPORT)
    f = r["forest"]
    assert r["nsites"] == len(snps) * (2 if K % 2 == 0 else 1) and r["sites"]["unmated"] == 0
    assert (f["blocks"], f["conflicts"], f["tied"], f["single"], f["bad"]) == (1, 0, 0, 0, 0) and f["largest"] == r["nsites"]
    k1 = {x for x, _ in PO.table([h1], K)}
    k2 = {x for x, _ in PO.table([h2], K)}
    A, B = {x for x, _ in r["A"]}, {x for x, _ in r["B"]}
    assert {frozenset(A), frozenset(B)} == {frozenset(k1 - k2) & frozenset(x for x, _ in r["P"]),
                                            frozenset(k2 - k1) & frozenset(x for x, _ in r["P"])}
    assert A | B == {x for x, _ in r["P"]} and not A & B
    line1, line2 = PO.lines(r, len(reads))
    assert line1.startswith("tabphase: %d k-mers, %d sites, %d sequences, " % (len(r["P"]), r["nsites"], len(reads)))
    assert " 0 conflicts, 1 blocks, largest %d sites, 0 unlinked sites\n" % r["nsites"] in line2
    assert PO.sites_tsv(r, K).count(b"\n") == r["nsites"]


# ---- ph_rule.h on the host ----

def test_rule_on_the_host():
    """classpro_amd/csrc/ph_rule.h compiles for the host: tests/ph_rule_check.cpp runs the key, order and parity functions
    and ph_forest_host over random graphs under AddressSanitizer and UBSan; the forests are the oracle's."""
    src = os.path.join(ROOT, "tests", "ph_rule_check.cpp")
    exe = os.path.join(ROOT, "tests", "_ph_rule_check")
    inc = os.path.join(ROOT, "classpro_amd", "csrc")
    build_if_changed(exe, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           "-o", exe, src], [src, os.path.join(inc, "ph_rule.h")])
    n = 400
    r = subprocess.run([exe, str(n), "11"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "rule %d" % n
    at, graphs, kept = 0, 0, 0
    while lines[at].startswith("G "):
        ns, ms, ne = map(int, lines[at].split()[1:])
        counts = {}
        for k in range(ne):
            s, t, cis, trans = map(int, lines[at + 1 + k].split()[1:])
            if cis:
                counts[PO.link_key(s, 0, t, 0)] = cis
            if trans:
                counts[PO.link_key(s, 0, t, 1)] = trans
        at += 1 + ne
        block, side, t = PO.forest(counts, ns, ms)
        assert lines[at].split()[1:] == [str(b) for b in block], graphs
        assert lines[at + 1].split()[1:] == [str(s) for s in side], graphs
        assert [int(x) for x in lines[at + 2].split()[1:]] == [t[c] for c in PO.TALLY[:9]], graphs
        at += 3
        graphs, kept = graphs + 1, kept + t["kept"]
    assert graphs == n and kept > 10 * n and at == len(lines) - 1


# ---- the exports and the errors that come before the device ----

def test_library_exports(built):
    import ctypes as C
    from classpro_amd import _lib, api
    L = _lib.lib()
    names = ["cp_kmer_counts_add_keys", "cp_kmer_sorted_het_sites", "cp_kmer_sorted_read_links", "cp_phase_forest",
             "cp_kmer_sorted_phase_split"]
    assert set(names) <= set(_lib.SYMBOLS)
    assert [len(getattr(L, n).argtypes) for n in names] == [5, 6, 12, 7, 8]
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert ("enum { CP_PH_EDGES = 0, CP_PH_KEPT = 1, CP_PH_TIED = 2, CP_PH_WEAK = 3, CP_PH_FOREST = 4, CP_PH_CONFLICTS = 5, "
            "CP_PH_BLOCKS = 6,") in hdr
    assert hdr.index("Heterozygous pairs of sorted k-mers (tabhet)") < hdr.index("Phasing heterozygous sites from reads (tabphase)") \
        < hdr.index("Unitigs of sorted k-mers (tabunitig)")
    assert api.PHASE_TALLY == PO.TALLY and api.SortedKmers.LINK_TALLY == ("markers", "links", "self")
    n = C.c_int64(-7)
    for call, who in ((lambda: L.cp_kmer_counts_add_keys(None, None, None, 0, None), b"cp_kmer_counts_add_keys"),
                      (lambda: L.cp_kmer_sorted_het_sites(None, None, None, C.byref(n), None, None), b"cp_kmer_sorted_het_sites"),
                      (lambda: L.cp_kmer_sorted_read_links(None, None, 1, None, None, 0, 0, None, 0, C.byref(n), None, None),
                       b"cp_kmer_sorted_read_links"),
                      (lambda: L.cp_phase_forest(None, 0, 2, None, None, None, None), b"cp_phase_forest"),
                      (lambda: L.cp_kmer_sorted_phase_split(None, None, None, None, 0, 0, None, None),
                       b"cp_kmer_sorted_phase_split")):
        assert call() == -1 and who in L.cp_last_error(), who
    assert n.value == -7
    S = api.SortedKmers.__new__(api.SortedKmers)
    S.s = None
    for call in (lambda: S.het_sites(), lambda: S.read_links(None, None), lambda: S.phase_split(None, None, None),
                 lambda: api.phase_forest(S, 0)):
        with pytest.raises(ValueError):
            call()


# ---- tabphase before the GPU ----

def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    a, src, out = os.path.join(d, "tab"), os.path.join(d, "reads.fasta"), os.path.join(d, "out")
    before = listing(d)
    cases = [((), USAGE), ((a,), USAGE), (("-v", "-m2", a), USAGE), ((a, src, out, out), USAGE),
             (("-x", a, src), "tabphase: -x is an illegal option\n"),
             (("-vq", a, src), "tabphase: -q is an illegal option\n"),
             (("-mx", a, src), "tabphase: -m 'x' argument is not an integer\n"),
             (("-b", a, src), "tabphase: -b '' argument is not an integer\n"),
             (("-T1e3", a, src), "tabphase: -T '1e3' argument is not an integer\n"),
             (("-m0", a, src, out), "tabphase: Support of an edge must be positive (0)\n"),
             (("-b0", a, src), "tabphase: Bases per device batch must be positive (0)\n"),
             (("-T0", a, src), "tabphase: Number of threads must be positive (0)\n"),
             ((a + ":0-3", src), "tabphase: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a + ":5-2", src, out), "tabphase: Count range of %s needs 1 <= lo <= hi (5-2)\n" % a),
             ((os.path.join(d, "nothing"), src, out), "tabphase: Cannot open %s/nothing.ktab [errno=2]\n" % d),
             ((a, os.path.join(d, "nothing"), out),
              "tabphase: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d),
             ((a, src, os.path.join(d, "no_such_dir", "out")), "tabphase: Cannot open %s/no_such_dir/out.A.ktab for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".sites.tsv")                           # a directory has the last file's name: the four before it are not left behind
    before = listing(d)
    r = run(a, src, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabphase: Cannot open %s.sites.tsv for 'w'\n" % out)
    assert listing(d) == before
    os.symlink(a + ".ktab", out + ".A.ktab")               # the result would replace the operand
    r = run(a, src, out)
    assert (r.returncode, r.stdout) == (1, "") and r.stderr == "tabphase: %s.A.ktab is the operand: the result needs a name of its own\n" % out


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    msg = spoil(d, how)                                    # spoils `tab`; "K = 4" is among them
    before = listing(d)
    r = run("-m3", os.path.join(d, "tab") + ":2-", os.path.join(d, "reads"), os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabphase: " + msg), how
    assert listing(d) == before

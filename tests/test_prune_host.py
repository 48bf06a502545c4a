"""Pruning the unitig graph, the part that needs no GPU: the oracle of tests/prune_oracle.py on graphs built by hand whose
marks follow from how they are built, the first-principles case (reads with spaced errors over a genome come back as the
genome's k-mers, in two rounds), the rule of classpro_amd/csrc/kn_rule.h on the host under AddressSanitizer and UBSan
against the oracle (tests/kn_rule_check.cpp), the export and the argument errors of cp_kmer_sorted_unitig_prune that come
before the device, and every error tabclean reports before it touches the GPU (exact stderr, exit 1, nothing on stdout, no
file created).  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import prune_cases as PC
import prune_oracle as PR
import unitig_graph_oracle as GO
import unitig_oracle as UO
from conftest import ROOT, build_if_changed
from test_readhits_host import good                        # noqa: F401  (the fixture: two tables at K = 12, one at K = 8, a source)
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabclean")
USAGE = ("Usage: tabclean [-v] [-i<int(0)>] [-t<int(2K)>] [-b<int(0)>] [-r<int(10)>] [-T<int(4)>]\n"
         "                <table>[.ktab][:<lo>-<hi>] [<out_root>]\n")


# ---- the oracle on the cases built by hand ----

@pytest.mark.parametrize("which", range(len(PC.hand_cases())))
def test_hand_cases(which):
    name, seqs, K, limits, expect = PC.hand_cases()[which]
    ents = UO.table(seqs, K)
    L = GO.Links(ents, K)
    want = PC.expected_why(L.utgs, expect)
    out, why, t = PR.prune(ents, K, None, limits, L=L)
    assert why == want, name
    gone = {UO.canon(UO.key_of(s[p:p + K]), K) for s in expect for p in range(len(s) - K + 1)}
    assert [x for x, _ in out] == [x for x, _ in ents if x not in gone], name
    assert t["unitigs"] == L.n and t["removed_keys"] == len(gone) and t["kept_keys"] == len(ents) - len(gone)
    assert (t["islands"], t["tips"], t["bubbles"]) == tuple(sum(w == k for w in expect.values()) for k in (1, 2, 3))
    assert t["removed_bases"] == sum(len(s) for s in expect)


def test_hand_cases_written_out():
    """The marks of four of the cases as literal lists, in the order of the unitigs."""
    got = {}
    for name, seqs, K, limits, _ in PC.hand_cases():
        got[name] = PR.prune(UO.table(seqs, K), K, None, limits)[1]
    assert got["tip on a path"] == [2, 0, 0] and got["a lone dead end stays"] == [0, 0, 0]
    assert got["bubble, unequal counts"] == [0, 0, 0, 3] and got["three arms, unequal"] == [0, 3, 0, 3, 0]


@pytest.mark.parametrize("which", range(4))
def test_nothing_goes_at_self_arcs_and_palindromes(which):
    name, ents, K = PC.quiet_cases()[which]
    out, why, t = PR.prune(ents, K, None, (1000, 1000, 1000))
    assert out == ents and not any(why) and t["removed_keys"] == 0, name


def test_each_limit_at_zero():
    seqs, K, expect = PC.limit_case()
    ents = UO.table(seqs, K)
    L = GO.Links(ents, K)
    assert not any(PR.prune(ents, K, None, (0, 0, 0), L=L)[1])
    union = {}
    for r in range(3):
        limits = [0, 0, 0]
        limits[r] = 2 * K
        assert PR.prune(ents, K, None, tuple(limits), L=L)[1] == PC.expected_why(L.utgs, expect[r])
        union.update(expect[r])
    assert PR.prune(ents, K, None, (2 * K, 2 * K, 2 * K), L=L)[1] == PC.expected_why(L.utgs, union)


# ---- first principles ----

@pytest.mark.parametrize("K", [15, 21])
@pytest.mark.parametrize("seed", PC.SEEDS)
def test_spaced_errors_give_the_genome_back(K, seed):
    """Error sites a multiple of 2K apart give tips and simple bubbles only: one round removes every error k-mer and no
    other, the second removes nothing."""
    g, seqs = PC.read_set(seed, K, True)
    ents = UO.table(seqs, K)
    truth = UO.table([g], K)
    assert len(ents) > len(truth) + 100
    out, tallies = PR.clean(ents, K, None, (0, 2 * K, 2 * K - 1))
    assert [x for x, _ in out] == [x for x, _ in truth]
    assert len(tallies) == 2 and tallies[1]["removed_keys"] == 0 and tallies[0]["removed_keys"] == len(ents) - len(truth)
    assert tallies[0]["tips"] > 0 and tallies[0]["bubbles"] > 0


@pytest.mark.parametrize("K", [15, 21])
@pytest.mark.parametrize("seed", PC.SEEDS)
def test_unspaced_errors_lose_no_genome_kmer(K, seed):
    """Uniform error sites leave interleaved bubbles behind; no k-mer of the genome goes."""
    g, seqs = PC.read_set(seed, K, False)
    out, tallies = PR.clean(UO.table(seqs, K), K, None, (0, 2 * K, 2 * K - 1))
    assert {x for x, _ in UO.table([g], K)} <= {x for x, _ in out} and tallies[0]["removed_keys"] > 0


def test_command_text():
    seqs, K, _ = PC.limit_case()
    ents = UO.table(seqs, K)
    text, out = PR.text(ents, K, None, (0, 2 * K, 0))
    lines = text.splitlines()
    assert lines[0] == UO.line(ents, K).replace("tabunitig", "tabclean").strip()
    assert lines[1] == "tabclean: round 1: 7 unitigs, 0 islands, 1 tips, 0 bubbles, 3 k-mers removed"
    assert lines[2] == "tabclean: round 2: 5 unitigs, 0 islands, 0 tips, 0 bubbles, 0 k-mers removed"
    assert lines[4] == "tabclean: %d k-mers in, %d out, 2 rounds" % (len(ents), len(ents) - 3) and len(lines) == 5
    text, out1 = PR.text(ents, K, (2, None), (2 * K, 2 * K, 2 * K), rounds=1)
    assert text.splitlines()[-1] == "tabclean: %d k-mers in, %d out, 1 rounds" % (sum(c >= 2 for _, c in ents), len(out1))


# ---- kn_rule.h on the host ----

def test_rule_on_the_host():
    """classpro_amd/csrc/kn_rule.h compiles for the host: tests/kn_rule_check.cpp runs it over random small graphs, half of
    them with a planted bubble and fork, a third with weights near 2^62, and over arrays of random words, under
    AddressSanitizer and UBSan; the marks it prints are those of the oracle."""
    src = os.path.join(ROOT, "tests", "kn_rule_check.cpp")
    exe = os.path.join(ROOT, "tests", "_kn_rule_check")
    inc = os.path.join(ROOT, "classpro_amd", "csrc")
    build_if_changed(exe, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           "-o", exe, src], [src, os.path.join(inc, "kn_rule.h")])
    r = subprocess.run([exe, "3000", "7"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "wild 3000" and len(lines) == 7 * 3000 + 1
    seen, wraps = [0, 0, 0, 0], 0
    for g in range(3000):
        head = lines[7 * g].split()
        assert head[0] == "G"
        K, count, links, isl, tip, bub = map(int, head[1:])
        rows = {}
        for ln in lines[7 * g + 1:7 * g + 7]:
            f = ln.split()
            rows[f[0]] = [int(x) for x in f[1:]]
        assert len(rows["loff"]) == 2 * count + 1 and len(rows["link"]) == links and len(rows["why"]) == count
        bases = [b - a for a, b in zip(rows["off"], rows["off"][1:])]
        R = PR.Rule(rows["loff"], rows["link"], bases, [f & 1 for f in rows["flag"]], rows["weight"], K, (isl, tip, bub))
        want = R.all()
        assert rows["why"] == want, (g, rows)
        for w in want:
            seen[w] += 1
        if max(rows["weight"]) > 1 << 61:                  # would 64-bit products have given another answer?
            narrow = PR.Rule(rows["loff"], rows["link"], bases, [f & 1 for f in rows["flag"]], rows["weight"], K, (isl, tip, bub))
            narrow.mul = lambda a, b: (a * b) % (1 << 64)
            wraps += narrow.all() != want
    assert min(seen) > 100, seen
    assert wraps > 0                                       # some graphs do tell 64-bit products from exact ones


# ---- the export and the errors before the device ----

def test_library_export_and_argument_errors(built):
    from classpro_amd import _lib
    from classpro_amd.api import SortedKmers, Unitigs
    L = _lib.lib()
    assert "cp_kmer_sorted_unitig_prune" in _lib.SYMBOLS and len(L.cp_kmer_sorted_unitig_prune.argtypes) == 10
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert ("enum { CP_PRUNE_UNITIGS, CP_PRUNE_ISLANDS, CP_PRUNE_TIPS, CP_PRUNE_BUBBLES, CP_PRUNE_REMOVED_KEYS,\n"
            "       CP_PRUNE_REMOVED_BASES, CP_PRUNE_KEPT_KEYS, CP_PRUNE_WIDTH };") in hdr
    assert hdr.index("Reads through the unitig graph") < hdr.index("Pruning the unitig graph") < hdr.index("Global-threshold labels")
    assert SortedKmers.PRUNE_TALLY == PR.TALLY
    tally, limits = (C.c_int64 * 7)(*[-7] * 7), (C.c_int64 * 3)(0, 0, 0)
    for args in ((None, None, None, None, None, limits, None, tally, None), (None, None, None, None, None, None, None, None, None)):
        h = C.c_void_p(1)
        assert L.cp_kmer_sorted_unitig_prune(*args, C.byref(h)) == -1 and h.value is None
        assert b"cp_kmer_sorted_unitig_prune" in L.cp_last_error()
    assert list(tally) == [-7] * 7
    S = SortedKmers.__new__(SortedKmers)
    S.s = None
    with pytest.raises(ValueError):
        S.prune(None)
    with pytest.raises(ValueError):
        S.clean()
    S.s, S.K, S.n, S.device = 1, 9, 0, "cuda:0"            # the checks of U come before anything is called
    try:
        with pytest.raises(ValueError):
            S.prune(None)
        U = Unitigs(L, "cuda:0", 9, None, {"unitigs": 0, "bases": 0}, None, None, None)
        with pytest.raises(ValueError):
            S.prune(U, tips=18)
        with pytest.raises(ValueError):
            S.clean(rounds=0)
    finally:
        S.s = None


# ---- tabclean before the GPU ----

def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    a, b = os.path.join(d, "tab"), os.path.join(d, "o:ther.ktab")
    out = os.path.join(d, "out")
    before = listing(d)
    cases = [((), USAGE), (("-v",), USAGE), ((a, out, b), USAGE), (("-t5", "-b3"), USAGE),
             (("-x", a), "tabclean: -x is an illegal option\n"),
             (("-vq", a, out), "tabclean: -q is an illegal option\n"),
             (("-g", a, out), "tabclean: -g is an illegal option\n"),
             (("-tx", a), "tabclean: -t 'x' argument is not an integer\n"),
             (("-i", a), "tabclean: -i '' argument is not an integer\n"),
             (("-b1e3", a, out), "tabclean: -b '1e3' argument is not an integer\n"),
             (("-i-1", a, out), "tabclean: Island limit must be non-negative (-1)\n"),
             (("-t-5", a, out), "tabclean: Tip limit must be non-negative (-5)\n"),
             (("-b-2", a, out), "tabclean: Bubble limit must be non-negative (-2)\n"),
             (("-r0", a, out), "tabclean: Number of rounds must be positive (0)\n"),
             (("-r-3", a), "tabclean: Number of rounds must be positive (-3)\n"),
             (("-T0", a, out), "tabclean: Number of threads must be positive (0)\n"),
             ((a + ":0-3", out), "tabclean: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             (("-t0", b + ":5-2"), "tabclean: Count range of %s needs 1 <= lo <= hi (5-2)\n" % b),
             ((a + ":3", out), "tabclean: Cannot open %s:3.ktab [errno=2]\n" % a),                # no range: part of the path
             ((os.path.join(d, "nothing"), out), "tabclean: Cannot open %s/nothing.ktab [errno=2]\n" % d),
             ((a, a), "tabclean: %s.ktab is the operand: the result needs a name of its own\n" % a),
             (("-b23", a + ".ktab:2-", a), "tabclean: %s.ktab is the operand: the result needs a name of its own\n" % a),
             ((a, os.path.join(d, "no_such_dir", "out")), "tabclean: Cannot open %s/no_such_dir/out.ktab for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(os.path.join(d, "out.hist"))                  # a directory has the second file's name: the first is not left behind
    before = listing(d)
    r = run("-b23", a, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabclean: Cannot open %s/out.hist for 'w'\n" % d)
    assert listing(d) == before


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    r = run("-t30", "-b23", os.path.join(d, "tab") + ":2-", os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabclean: " + msg), how
    assert listing(d) == before

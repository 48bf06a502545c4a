"""tabhet and the heterozygous pairs without a GPU: tests/hetpairs_oracle.py against the three cases worked out by hand and
against a restatement on the strings themselves (both orientations written out, one substitution at position m), every
error tabhet reports before it touches the device (exact message, exit status 1, empty stdout, no file created), and the
symbol's declaration and the returns that need no device."""
import itertools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import hetpairs_oracle as HO
import ktab_oracle as KO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabhet")
USAGE = ("Usage: tabhet [-v] [-a] [-t] [-x<int(1000)>] [-y<int(1000)>] [-T<int(4)>]\n"
         "              <table>[.ktab][:<lo>-<hi>] [<out_root>]\n")
key = lambda s: KO.key_of(s.encode())


# ---- the oracle against the cases worked out by hand ----

def test_hand_case_palindromic_flanks():
    assert HO.candidates(key("ACAGT"), 5) == {key("ACCGT")}
    assert HO.canon(key("ACGGT"), 5) == key("ACCGT") and HO.canon(key("ACTGT"), 5) == key("ACAGT")


def test_hand_case_family_of_three():
    ents = [(key(s), c) for s, c in (("AAAAA", 4), ("AACAA", 9), ("AAGAA", 2))]
    assert HO.degrees(ents, 5) == [2, 2, 2]
    assert len(HO.pairs(ents, 5, unique=False)) == 3 and HO.pairs(ents, 5, unique=True) == []
    t = HO.tally(ents, 5, unique=False)
    assert t == {"keys": 3, "paired": 3, "multi": 3, "pairs": 3, "unique": 0, "out": 3}
    assert HO.tally(ents, 5)["out"] == 0 and HO.members(ents, 5) == []
    m = HO.matrix(ents, 5, 5, 5, unique=False)
    assert m.sum() == 3 and m[4, 5] == 1 and m[2, 4] == 1 and m[2, 5] == 1       # (4,9) (2,4) (2,9), folded at 5
    assert HO.het_text(m) == b"#a\tb\tpairs\n2\t4\t1\n2\t5\t1\n4\t5\t1\n"
    # a range that removes AAGAA leaves one unique pair
    assert HO.degrees(ents, 5, (3, None)) == [1, 1, 0] and HO.pairs(ents, 5, (3, None)) == [(key("AAAAA"), key("AACAA"))]


def test_hand_case_even_k_chain():
    ents = sorted((key(s), 1) for s in ("AACA", "AAAA", "ACAA"))
    by = dict(zip([x for x, _ in ents], HO.degrees(ents, 4)))
    assert (by[key("AACA")], by[key("AAAA")], by[key("ACAA")]) == (1, 2, 1)
    assert key("ACAA") not in HO.candidates(key("AACA"), 4)
    t = HO.tally(ents, 4, unique=False)
    assert (t["pairs"], t["unique"], t["multi"], t["out"]) == (2, 0, 1, 3)


# ---- the oracle against the strings ----

COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
rc = lambda s: "".join(COMP[c] for c in reversed(s))


def string_siblings(xs, K):
    """{x: the y in xs, y != x, of which some orientation differs from some orientation of x at position m and nowhere
    else}, on the strings of the canonical k-mers xs."""
    m = K // 2
    have = set(xs)
    out = {}
    for x in xs:
        found = set()
        for o in (x, rc(x)):
            for c in "ACGT":
                if c != o[m]:
                    v = o[:m] + c + o[m + 1:]
                    y = min(v, rc(v))
                    if y != x and y in have:
                        found.add(y)
        out[x] = found
    return out


def check_against_strings(keys, K):
    text = {x: KO.text_of(x, K).upper() for x in keys}
    ents = [(x, 1) for x in sorted(keys)]
    want = string_siblings(sorted(text.values()), K)
    got = HO.siblings(ents, K)
    assert {text[x]: {text[y] for y in ys} for x, ys in got.items()} == want
    for x, ys in got.items():
        for y in ys:
            assert x in got[y]                             # symmetric


@pytest.mark.parametrize("K", [3, 4, 5, 6, 7, 8])
def test_oracle_against_strings_on_every_canonical_kmer(K):
    keys = {HO.canon(x, K) for x in range(1 << (2 * K))}
    check_against_strings(keys, K)


@pytest.mark.parametrize("K", [21, 40])
def test_oracle_against_strings_on_sparse_tables(K):
    ents = HO.planted(random.Random(K), K, 2000)
    check_against_strings({x for x, _ in ents}, K)
    t = HO.tally(ents, K)
    assert t["pairs"] > 800 and t["unique"] > 500 and t["multi"] > 0
    assert set(HO.degrees(ents, K)) >= {0, 1, 2}


# ---- tabhet's errors ----

K0 = 12


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("hetpairs_host"))
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
    cases = [((), USAGE), ((a, out, out), USAGE), (("-v", "-a", "-x3"), USAGE),
             (("-q", a), "tabhet: -q is an illegal option\n"),
             (("-vc", a, out), "tabhet: -c is an illegal option\n"),
             (("-xq", a, out), "tabhet: -x 'q' argument is not an integer\n"),
             (("-x", a, out), "tabhet: -x '' argument is not an integer\n"),
             (("-y3.5", a, out), "tabhet: -y '3.5' argument is not an integer\n"),
             (("-Tx", a, out), "tabhet: -T 'x' argument is not an integer\n"),
             (("-T0", a, out), "tabhet: Number of threads must be positive (0)\n"),
             (("-x0", a, out), "tabhet: Histogram bounds must lie in [1, 32767] (0, 1000)\n"),
             (("-y32768", a, out), "tabhet: Histogram bounds must lie in [1, 32767] (1000, 32768)\n"),
             (("-x2047", "-y2048", a, out), "tabhet: Histogram of 4196352 cells exceeds 4194304\n"),
             ((a + ":0-3", out), "tabhet: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a + ":5-2", out), "tabhet: Count range of %s needs 1 <= lo <= hi (5-2)\n" % a),
             (("-t", a), "tabhet: -t needs <out_root>\n"),
             (("-at", a + ":2-"), "tabhet: -t needs <out_root>\n"),
             (("-t", a, a), "tabhet: %s.ktab is the operand: the result needs a name of its own\n" % a),
             ((a, os.path.join(d, "no_such_dir", "out")), "tabhet: Cannot open %s/no_such_dir/out.het for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".hist")                                # the last output cannot be created: the first two are removed again
    before = listing(d)
    r = run("-t", a, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabhet: Cannot open %s.hist for 'w'\n" % out)
    assert listing(d) == before
    os.mkdir(out + ".het")
    before = listing(d)
    r = run(a, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabhet: Cannot open %s.het for 'w'\n" % out)
    assert listing(d) == before


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)
    before = listing(d)
    r = run("-t", os.path.join(d, "tab"), os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabhet: " + msg), how
    assert listing(d) == before


# ---- the symbol ----

def test_symbol_is_declared_listed_and_exported(built):
    import ctypes as C
    from classpro_amd import _lib
    L = _lib.lib()
    assert "cp_kmer_sorted_het_pairs" in _lib.SYMBOLS and len(L.cp_kmer_sorted_het_pairs.argtypes) == 10
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert ("enum { CP_HET_KEYS = 0, CP_HET_PAIRED = 1, CP_HET_MULTI = 2, CP_HET_PAIRS = 3, CP_HET_UNIQUE = 4, "
            "CP_HET_OUT = 5, CP_HET_WIDTH = 6 };") in hdr
    assert "Heterozygous pairs of sorted k-mers" in hdr
    # a NULL snapshot is refused before the device is touched, and a given `out` is cleared
    m, t = np.full(4, -7, np.int64), np.full(6, -7, np.int64)
    h = C.c_void_p(12345)
    assert L.cp_kmer_sorted_het_pairs(None, None, 1, 1, 1, m.ctypes.data, t.ctypes.data, None, None, C.byref(h)) == -1
    assert h.value is None and (m == -7).all() and (t == -7).all()
    assert b"cp_kmer_sorted_het_pairs" in L.cp_last_error()
    assert L.cp_kmer_sorted_het_pairs(None, None, 1, 1, 1, None, None, None, None, None) == -1

"""tabop and the set algebra without a GPU: the identities of tests/setop_oracle.py on random entry lists, every error
tabop reports before it touches the device (exact message, exit status 1, empty stdout, no file created), how an
operand's count range is split off, and the two new exports of the library."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import ktab_oracle as KO
import setop_oracle as SO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabop")
USAGE = ("Usage: tabop [-v] [-T<int(4)>] [-c<left|sum|min|max>]\n"
         "             <A>[.ktab][:<lo>-<hi>] <and|or|sub|xor> <B>[.ktab][:<lo>-<hi>] [<out_root>]\n")
OPS, RULES = ("and", "or", "sub", "xor"), ("left", "sum", "min", "max")
RANGES = (None, (2, None), (None, 3), (2, 5), (7, 7))


def random_entries(rng, n, space=400, top=9):
    return [(k, rng.randint(1, top)) for k in sorted(rng.sample(range(space), n))]


@pytest.mark.parametrize("seed", range(6))
def test_oracle_identities(seed):
    rng = random.Random(seed)
    a, b = random_entries(rng, rng.randint(0, 200)), random_entries(rng, rng.randint(0, 200))
    for ra in RANGES:
        for rb in RANGES:
            res = {op: SO.combine(a, b, op, "left", ra, rb) for op in OPS}
            for op in OPS:
                ents, tally = res[op]
                assert ents == sorted(ents) and len({k for k, _ in ents}) == len(ents)
                assert tally == res["and"][1][:3] + (len(ents),)
            oa, ob, both = res["and"][1][:3]
            lo, hi = ra or (None, None)
            in_a = [e for e in a if (lo or 1) <= e[1] <= (hi or SO.BIG)]
            assert oa + both == len(in_a)
            assert (len(res["and"][0]), len(res["or"][0]), len(res["sub"][0]), len(res["xor"][0])) == (both, oa + ob + both, oa,
                                                                                                      oa + ob)
            # and + sub partition what is in A; xor = (a sub b) or (b sub a)
            assert sorted(res["and"][0] + res["sub"][0]) == in_a
            b_sub_a = SO.combine(b, a, "sub", "left", rb, ra)[0]
            assert res["xor"][0] == SO.combine(res["sub"][0], b_sub_a, "or")[0] == sorted(res["sub"][0] + b_sub_a)
            for rule in RULES:
                for op in ("sub", "xor"):                  # one side is in: every rule gives its count
                    assert SO.combine(a, b, op, rule, ra, rb)[0] == res[op][0]
            A, B = dict(in_a), dict(SO.combine(b, b, "and", "left", rb)[0])
            for rule, f in (("sum", lambda x, y: x + y), ("min", min), ("max", max), ("left", lambda x, y: x)):
                assert SO.combine(a, b, "and", rule, ra, rb)[0] == [(k, f(A[k], B[k])) for k in sorted(set(A) & set(B))]
    assert SO.combine(a, a, "and")[0] == a and SO.combine(a, a, "sub")[0] == [] and SO.combine(a, [], "or")[0] == a
    h = SO.hist(a + [(1000, 32767), (1001, 40000)])
    assert h[4].sum() == len(a) + 2 and h[2] == sum(c == 1 for _, c in a) and h[3] == 72767 and h[4][32766] == 2


K0, K1 = 12, 8


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """Two tables at K = 12, one of them under a name that holds a ':', and one at K = 8."""
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("setop_host"))
    for name, k, seed, parts in (("tab", K0, 5, 3), ("o:ther", K0, 7, 1), ("tab8", K1, 5, 2)):
        ents = KO.table(mixed_reads(k, seed), k)
        fastk.write_fastk_ktab(d, name, k, 1, [x for x, _ in ents], [c for _, c in ents], parts)
    return d


def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    a, b, b8, out = os.path.join(d, "tab"), os.path.join(d, "o:ther.ktab"), os.path.join(d, "tab8"), os.path.join(d, "out")
    before = listing(d)
    cases = [((), USAGE), ((a,), USAGE), ((a, "and"), USAGE), ((a, "and", b, out, out), USAGE), (("-v", "-T2", "-csum"), USAGE),
             (("-x", a, "and", b), "tabop: -x is an illegal option\n"),
             (("-vq", a, "and", b, out), "tabop: -q is an illegal option\n"),
             (("-Tx", a, "and", b, out), "tabop: -T 'x' argument is not an integer\n"),
             (("-T0", a, "and", b, out), "tabop: Number of threads must be positive (0)\n"),
             (("-T-2", a, "and", b, out), "tabop: Number of threads must be positive (-2)\n"),
             (("-cavg", a, "and", b, out), "tabop: Count rule must be one of left, sum, min, max (avg)\n"),
             (("-c", a, "and", b, out), "tabop: Count rule must be one of left, sum, min, max ()\n"),
             ((a, "nand", b, out), "tabop: Operator must be one of and, or, sub, xor (nand)\n"),
             ((a, "AND", b), "tabop: Operator must be one of and, or, sub, xor (AND)\n"),
             ((a + ":0-3", "and", b, out), "tabop: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a, "and", b + ":5-2", out), "tabop: Count range of %s needs 1 <= lo <= hi (5-2)\n" % b),
             ((a + ":3-7", "or", b + ":0-", out), "tabop: Count range of %s needs 1 <= lo <= hi (0-)\n" % b),
             ((a, "and", b8, out), "tabop: K of %s.ktab (12) and %s.ktab (8) differ\n" % (a, b8)),
             ((b8 + ".ktab", "sub", b), "tabop: K of %s.ktab (8) and %s (12) differ\n" % (b8, b)),
             ((a, "and", b, a), "tabop: %s.ktab is an operand: the result needs a name of its own\n" % a),
             ((a, "sub", b, os.path.join(d, ".", "o:ther")), "tabop: %s/./o:ther.ktab is an operand: the result needs a name of its own\n" % d),
             ((a, "and", b, os.path.join(d, "no_such_dir", "out")), "tabop: Cannot open %s/no_such_dir/out.ktab for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".hist")                                # the .hist cannot be created: a directory has its name
    before = listing(d)
    r = run(a, "and", b, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabop: Cannot open %s.hist for 'w'\n" % out)
    assert listing(d) == before                            # the stub opened before it is gone again


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how, side):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    ops = [os.path.join(d, "o:ther"), os.path.join(d, "tab")]
    r = run(ops[1 - side], "or", ops[side], os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabop: " + msg), how
    assert listing(d) == before


def test_range_parsing(built, good):
    """What is left of an operand once its range is split off shows in the message that names the two stubs."""
    d = good
    b8 = os.path.join(d, "tab8")
    differ = lambda x: "tabop: K of %s.ktab (12) and %s.ktab (8) differ\n" % (os.path.join(d, x), b8)
    before = listing(d)
    for arg, name in (("tab:3-", "tab"), ("tab:-7", "tab"), ("tab:3-7", "tab"), ("tab.ktab:3-7", "tab"), ("tab:-", "tab"),
                      ("o:ther", "o:ther"), ("o:ther:2-", "o:ther"), ("o:ther.ktab:1-32767", "o:ther"),
                      ("tab:99999999999999999999-", "tab")):
        r = run(os.path.join(d, arg), "and", b8 + ":4-4")
        assert (r.returncode, r.stdout, r.stderr) == (1, "", differ(name)), arg
    for arg in ("tab:3", "tab:3-7x", "tab:a-7", "tab:3--7", "tab:+3-7", "tab: 3-7"):       # no range: part of the path
        r = run(os.path.join(d, arg), "and", b8)
        assert (r.returncode, r.stdout) == (1, "") and r.stderr == "tabop: Cannot open %s.ktab [errno=2]\n" % os.path.join(d, arg)
    assert listing(d) == before


def test_library_exports(built):
    import ctypes as C
    from classpro_amd import _lib
    L = _lib.lib()
    assert {"cp_kmer_sorted_combine", "cp_kmer_sorted_hist"} <= set(_lib.SYMBOLS)
    assert L.cp_kmer_sorted_combine.argtypes[-1] == C.POINTER(C.c_void_p) and len(L.cp_kmer_sorted_combine.argtypes) == 8
    assert len(L.cp_kmer_sorted_hist.argtypes) == 4
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "enum { CP_SET_AND = 0, CP_SET_OR = 1, CP_SET_SUB = 2, CP_SET_XOR = 3 };" in hdr
    assert "enum { CP_CNT_LEFT = 0, CP_CNT_SUM = 1, CP_CNT_MIN = 2, CP_CNT_MAX = 3 };" in hdr
    # arguments are checked before the device is touched
    t = (C.c_int64 * 4)()
    assert L.cp_kmer_sorted_combine(None, None, 0, 0, None, t, None, None) == -1
    assert L.cp_kmer_sorted_hist(None, None, None, None) == -1

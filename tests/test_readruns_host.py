"""Runs of k-mer states, the part that needs no GPU: the oracle of tests/runs_oracle.py on marker strings whose runs are
written out, cp_run_blocks and `run_blocks` against the oracle's rule, the block N50 with a tie, the exports, the argument
errors of cp_kmer_sorted_read_runs that come before the device, and every error tabtrack reports before it touches the GPU
(exact stderr, exit 1, nothing on stdout, no file created).  Everything is integers: the tolerance is zero."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import runs_oracle as UO
from conftest import ROOT, build_if_changed
from test_readhits_host import good                        # noqa: F401  (the fixture: two tables at K = 12, one at K = 8, a source)
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabtrack")
USAGE = ("Usage: tabtrack [-v] [-m<int(1)>] [-b<int(67108864)>] [-o<out_root>]\n"
         "                <A>[.ktab][:<lo>-<hi>] [<B>[.ktab][:<lo>-<hi>]] <source>[.db|.dam|.f[ast][aq][.gz]]\n")
NONE, A, B, BOTH, OTHER = UO.NONE, UO.A, UO.B, UO.BOTH, UO.OTHER
LONG = "AAA.A.B.AAAA2BB.BBoBA"
LONG_RUNS = [(A, 0, 4, 4), (B, 6, 6, 1), (A, 8, 11, 4), (B, 13, 19, 5), (A, 20, 20, 1)]


# ---- the oracle itself ----

def test_oracle_on_written_markers():
    phase = (UO.PHASE_SKIP, UO.PHASE_EMIT)
    assert phase == (0x19, 0x06)
    assert UO.runs("AA.B2BA", *phase) == [(A, 0, 1, 2), (B, 3, 5, 2), (A, 6, 6, 1)]
    assert UO.runs("AA.B2BA", 0, 1 << NONE) == [(NONE, 2, 2, 1)]
    assert UO.runs("A.ooooo.B") == [(A, 0, 0, 1), (NONE, 1, 1, 1), (OTHER, 2, 6, 5), (NONE, 7, 7, 1), (B, 8, 8, 1)]
    assert UO.runs(LONG, *phase) == LONG_RUNS
    assert UO.blocks(LONG_RUNS, 1) == (LONG_RUNS, 0)
    assert UO.blocks(LONG_RUNS, 2) == ([(A, 0, 11, 8), (B, 13, 19, 5)], 2)
    assert UO.blocks(LONG_RUNS, 5) == ([(B, 13, 19, 5)], 4) and UO.blocks(LONG_RUNS, 6) == ([], 5) and UO.blocks([], 1) == ([], 0)
    assert UO.runs("", *phase) == [] and UO.runs("..2o", *phase) == [] and UO.runs("ABAB", 0, 1 << A) == [(A, 0, 0, 1), (A, 2, 2, 1)]
    assert UO.runs("A.A", 1 << NONE, 1 << A) == [(A, 0, 2, 2)]            # a skipped position neither breaks nor extends


def test_n50_rule():
    assert UO.n50([]) == 0 and UO.n50([7]) == 7
    assert UO.n50([10, 5, 5]) == 10                        # 10 of 20 is half already
    assert UO.n50([9, 5, 5, 1]) == 5                       # 9 of 20 is not: both fives are taken together
    assert UO.n50([4, 4, 4, 4, 3]) == 4 and UO.n50([6, 5, 5, 5]) == 5 and UO.n50([1, 1, 1, 100]) == 100


# ---- the summary algebra of the kernels, on the host ----

def test_summary_algebra_on_the_host():
    """classpro_amd/csrc/kr_sum.h compiles for the host: tests/kr_sum_check.cpp runs the three passes of kmer_runs.hip over
    random reads with small lanes and blocks, under AddressSanitizer and UBSan, against a plain loop."""
    src = os.path.join(ROOT, "tests", "kr_sum_check.cpp")
    exe = os.path.join(ROOT, "tests", "_kr_sum_check")
    inc = os.path.join(ROOT, "classpro_amd", "csrc")
    build_if_changed(exe, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           "-o", exe, src], [src, os.path.join(inc, "kr_sum.h")])
    r = subprocess.run([exe, "20000"], capture_output=True, text=True)
    assert (r.returncode, r.stdout) == (0, "ok 20000\n"), r.stdout + r.stderr


# ---- cp_run_blocks ----

def c_blocks(L, rs, min_n, read=3):
    from classpro_amd.api import RUN_DTYPE
    arr = np.array([(f, l, n, read, s) for s, f, l, n in rs], RUN_DTYPE).reshape(-1)
    out = np.zeros(len(arr) + 1, RUN_DTYPE)
    dropped = C.c_int64(-1)
    nb = L.cp_run_blocks(arr.ctypes.data if len(arr) else out.ctypes.data, len(arr), min_n, out.ctypes.data, C.byref(dropped))
    assert nb >= 0 and all(int(x) == read for x in out["read"][:nb])
    return [(int(b["state"]), int(b["first"]), int(b["last"]), int(b["n"])) for b in out[:nb]], dropped.value


def test_run_blocks_against_the_rule(built):
    from classpro_amd._lib import ClassProError, lib
    from classpro_amd.api import RUN_DTYPE, run_blocks
    L = lib()
    assert RUN_DTYPE.itemsize == 32
    rng = random.Random(4)
    cases = [(LONG_RUNS, m) for m in (1, 2, 3, 5, 6)] + [([], 1), ([(B, 5, 5, 1)], 1), ([(B, 5, 5, 1)], 2)]
    for _ in range(200):
        rs, at = [], 0
        for _ in range(rng.randrange(0, 40)):
            n = rng.choice([1, 1, 2, 3, 10, 1 << 40])
            last = at + n - 1 + rng.randrange(3)
            state = rng.choice([A, B]) if not rs or rng.random() < 0.2 else A + B - rs[-1][0]
            rs.append((state, at, last, n))
            at = last + 1 + rng.randrange(5)
        cases.append((rs, rng.choice([1, 2, 3, 4, 11])))
    for rs, m in cases:
        want = UO.blocks(rs, m)
        assert c_blocks(L, rs, m) == want, (rs, m)
        bl, dropped = run_blocks([(f, l, n, 0, s) for s, f, l, n in rs], m)
        assert ([(s, f, l, n) for f, l, n, _, s in bl], dropped) == want
    cols = {k: np.array([r[i] for r in LONG_RUNS]) for k, i in (("state", 0), ("first", 1), ("last", 2), ("n", 3))}
    cols["read"] = np.zeros(5, np.int32)
    assert run_blocks(cols, 2) == ([(0, 11, 8, 0, A), (13, 19, 5, 0, B)], 2)           # the dict of read_runs as well
    one = np.zeros(1, RUN_DTYPE)
    d = C.c_int64()
    for args in ((None, 1, 1, one.ctypes.data, C.byref(d)), (one.ctypes.data, 1, 1, None, C.byref(d)),
                 (one.ctypes.data, 1, 1, one.ctypes.data, None), (one.ctypes.data, 1, 0, one.ctypes.data, C.byref(d)),
                 (one.ctypes.data, 1, -2, one.ctypes.data, C.byref(d)), (one.ctypes.data, -1, 1, one.ctypes.data, C.byref(d))):
        assert L.cp_run_blocks(*args) == -1 and b"cp_run_blocks" in L.cp_last_error()
    with pytest.raises(ClassProError):
        run_blocks([], 0)


def test_library_exports(built):
    from classpro_amd import _lib
    from classpro_amd.api import SortedKmers
    L = _lib.lib()
    assert {"cp_kmer_sorted_read_runs", "cp_run_blocks"} <= set(_lib.SYMBOLS)
    assert len(L.cp_kmer_sorted_read_runs.argtypes) == 15 and len(L.cp_run_blocks.argtypes) == 5
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "enum { CP_RUN_NONE = 0, CP_RUN_A = 1, CP_RUN_B = 2, CP_RUN_BOTH = 3, CP_RUN_OTHER = 4 };" in hdr
    assert "typedef struct cp_kmer_run { int64_t first, last, n; int32_t read, state; } cp_kmer_run;" in hdr
    assert (SortedKmers.RUN_NONE, SortedKmers.RUN_A, SortedKmers.RUN_B, SortedKmers.RUN_BOTH, SortedKmers.RUN_OTHER) == (1, 2, 4, 8, 16)
    # arguments are checked before the device is touched
    t = C.c_int64()
    assert L.cp_kmer_sorted_read_runs(None, None, 1, None, 0, 31, None, None, 0, 0, None, 0, None, C.byref(t), None) == -1
    assert b"cp_kmer_sorted_read_runs" in L.cp_last_error()


# ---- tabtrack before the GPU ----

def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    a, b, b8, src = os.path.join(d, "tab"), os.path.join(d, "o:ther.ktab"), os.path.join(d, "tab8"), os.path.join(d, "reads")
    before = listing(d)
    cases = [((), USAGE), ((a,), USAGE), ((a, b, src, src), USAGE), (("-v", "-m2", "-b5", "-oout"), USAGE), (("-m2", a), USAGE),
             (("-x", a, b, src), "tabtrack: -x is an illegal option\n"),
             (("-vq", a, src), "tabtrack: -q is an illegal option\n"),
             (("-u", a, b, src), "tabtrack: -u is an illegal option\n"),
             (("-v", "-T4", a, src), "tabtrack: -T is an illegal option\n"),
             (("-mx", a, b, src), "tabtrack: -m 'x' argument is not an integer\n"),
             (("-m", a, b, src), "tabtrack: -m '' argument is not an integer\n"),
             (("-b1e6", a, src), "tabtrack: -b '1e6' argument is not an integer\n"),
             (("-m0", a, b, src), "tabtrack: Minimum number of markers must be positive (0)\n"),
             (("-m-3", a, b, src), "tabtrack: Minimum number of markers must be positive (-3)\n"),
             (("-b0", a, src), "tabtrack: Bases per device batch must be positive (0)\n"),
             (("-b-1", a, b, src), "tabtrack: Bases per device batch must be positive (-1)\n"),
             (("-m2", a, src), "tabtrack: -m needs two tables\n"),
             (("-m1", a + ":0-3", src), "tabtrack: -m needs two tables\n"),
             ((a + ":0-3", src), "tabtrack: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a + ":0-3", b, src), "tabtrack: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a, b + ":5-2", src), "tabtrack: Count range of %s needs 1 <= lo <= hi (5-2)\n" % b),
             ((a + ":3-7", b + ":0-", src), "tabtrack: Count range of %s needs 1 <= lo <= hi (0-)\n" % b),
             ((a + ":3", src), "tabtrack: Cannot open %s:3.ktab [errno=2]\n" % a),             # no range: part of the path
             ((a, b8, src), "tabtrack: K of %s.ktab (12) and %s.ktab (8) differ\n" % (a, b8)),
             ((b8 + ".ktab:2-", b + ":-9", src), "tabtrack: K of %s.ktab (8) and %s (12) differ\n" % (b8, b)),
             ((a, os.path.join(d, "nothing")), "tabtrack: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d),
             ((a, b, os.path.join(d, "nothing")), "tabtrack: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d),
             (("-o" + os.path.join(d, "no_such_dir", "out"), a, src),
              "tabtrack: Cannot open %s/no_such_dir/out.missing.bed for 'w'\n" % d),
             (("-o" + os.path.join(d, "no_such_dir", "out"), a, b, src),
              "tabtrack: Cannot open %s/no_such_dir/out.blocks.bed for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(os.path.join(d, "out.blocks.bed"))            # a directory has the file's name
    before = listing(d)
    r = run("-o" + os.path.join(d, "out"), a, b, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabtrack: Cannot open %s/out.blocks.bed for 'w'\n" % d)
    assert listing(d) == before


@pytest.mark.parametrize("side", [0, 1, 2])
@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how, side):
    """The spoiled table as the only one, as A of two and as B of two."""
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    ops = [[os.path.join(d, "tab")], [os.path.join(d, "tab"), os.path.join(d, "o:ther")], [os.path.join(d, "o:ther"), os.path.join(d, "tab")]]
    r = run("-o" + os.path.join(d, "out"), *ops[side], os.path.join(d, "reads.fasta"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabtrack: " + msg), how
    assert listing(d) == before

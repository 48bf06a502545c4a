"""tabcmp and the count comparison without a GPU: tests/cmphist_oracle.py against three matrices worked out by hand, every
error tabcmp reports before it touches the device (exact message, exit status 1, empty stdout, no file created), and
cp_kmer_qv against the oracle's restatement."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cmphist_oracle as CO
import ktab_oracle as KO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabcmp")
USAGE = ("Usage: tabcmp [-v] [-q] [-x<int(8)>] [-y<int(1000)>] [-w<keys|a|b>]\n"
         "              <A>[.ktab][:<lo>-<hi>] <B>[.ktab][:<lo>-<hi>] [<out_root>]\n")


# ---- the oracle against matrices worked out by hand ----

def test_oracle_hand_matrix_keys_and_weights():
    a = [(1, 1), (2, 2), (3, 5), (7, 1)]
    b = [(2, 1), (3, 9), (4, 1), (5, 2)]
    # key 1: (1,0); 2: (2,1); 3: (min(5,3), min(9,2)) = (3,2); 7: (1,0); 4: (0,1); 5: (0,2)
    assert CO.matrix(a, b, 3, 2).tolist() == [[0, 1, 1], [2, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert CO.matrix(a, b, 3, 2, "a").tolist() == [[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 5]]
    assert CO.matrix(a, b, 3, 2, "b").tolist() == [[0, 1, 2], [0, 0, 0], [0, 1, 0], [0, 0, 9]]
    assert CO.tally(CO.matrix(a, b, 3, 2)) == (2, 2, 2)
    assert CO.completeness(CO.matrix(a, b, 3, 2)) == 50.0
    assert CO.cmp_text(CO.matrix(a, b, 3, 2, "a"), "a") == b"#a\tb\tsumA\n1\t0\t2\n2\t1\t2\n3\t2\t5\n"


def test_oracle_hand_matrix_ranges():
    a = [(1, 1), (2, 2), (3, 5), (7, 1)]
    b = [(2, 1), (3, 9), (4, 1), (5, 2)]
    # A keeps counts >= 2 (keys 2, 3), B keeps counts <= 2 (keys 2, 4, 5): key 3 is in A only, keys 1 and 7 in neither
    m = CO.matrix(a, b, 8, 8, "keys", (2, None), (None, 2))
    want = np.zeros((9, 9), np.int64)
    want[2, 1], want[5, 0], want[0, 1], want[0, 2] = 1, 1, 1, 1
    assert np.array_equal(m, want) and m[0, 0] == 0
    assert CO.tally(m) == (1, 2, 1)
    mb = CO.matrix(a, b, 8, 8, "b", (2, None), (None, 2))
    assert mb.sum() == 1 + 1 + 2 and mb[5, 0] == 0         # the 9 of key 3 is outside B's range: it adds nothing


def test_oracle_hand_matrix_self_empty_and_wrap():
    a = [(10, 1), (11, 40000), (12, 3)]
    m = CO.matrix(a, a, 2, 32767, "a")
    assert m[1, 1] == 1 and m[2, 32767] == 40000 and m[2, 3] == 3 and m.sum() == 40004
    assert CO.matrix([], [], 1, 1).tolist() == [[0, 0], [0, 0]]
    assert CO.matrix(a, [], 1, 1).tolist() == [[0, 0], [3, 0]] and CO.matrix([], a, 1, 1).tolist() == [[0, 3], [0, 0]]
    assert math.isnan(CO.completeness(CO.matrix(a, [], 1, 1)))
    big = [(1, CO.BIG), (2, CO.BIG), (3, 5)]                # 2 * (2^63 - 1) + 5 = 2^64 + 3: the sum is taken modulo 2^64
    assert CO.matrix(big, [], 1, 1, "a")[1, 0] == 3
    q, e = CO.qv(21, 0, 100)
    assert q == math.inf and e == 0.0
    q, e = CO.qv(1, 1, 1000)                               # K = 1: the error is the share itself, QV 30
    assert abs(e - 1e-3) < 1e-15 and abs(q - 30.0) < 1e-9


# ---- tabcmp's errors ----

K0, K1 = 12, 8


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """Two tables at K = 12, one of them under a name that holds a ':', and one at K = 8."""
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("cmphist_host"))
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
    cases = [((), USAGE), ((a,), USAGE), ((a, b, out, out), USAGE), (("-v", "-q", "-x3", "-wa"), USAGE),
             (("-T", a, b), "tabcmp: -T is an illegal option\n"),
             (("-vc", a, b, out), "tabcmp: -c is an illegal option\n"),
             (("-xq", a, b, out), "tabcmp: -x 'q' argument is not an integer\n"),
             (("-x", a, b, out), "tabcmp: -x '' argument is not an integer\n"),
             (("-y3.5", a, b, out), "tabcmp: -y '3.5' argument is not an integer\n"),
             (("-x0", a, b, out), "tabcmp: Histogram bounds must lie in [1, 32767] (0, 1000)\n"),
             (("-y32768", a, b, out), "tabcmp: Histogram bounds must lie in [1, 32767] (8, 32768)\n"),
             (("-x-2", "-y0", a, b, out), "tabcmp: Histogram bounds must lie in [1, 32767] (-2, 0)\n"),
             (("-x2047", "-y2048", a, b, out), "tabcmp: Histogram of 4196352 cells exceeds 4194304\n"),
             (("-x32767", "-y32767", a, b), "tabcmp: Histogram of 1073741824 cells exceeds 4194304\n"),
             (("-wsum", a, b, out), "tabcmp: Weight must be one of keys, a, b (sum)\n"),
             (("-w", a, b, out), "tabcmp: Weight must be one of keys, a, b ()\n"),
             (("-wA", a, b), "tabcmp: Weight must be one of keys, a, b (A)\n"),
             ((a + ":0-3", b, out), "tabcmp: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a, b + ":5-2", out), "tabcmp: Count range of %s needs 1 <= lo <= hi (5-2)\n" % b),
             (("-q", a + ":3-7", b + ":0-", out), "tabcmp: Count range of %s needs 1 <= lo <= hi (0-)\n" % b),
             ((a, b8, out), "tabcmp: K of %s.ktab (12) and %s.ktab (8) differ\n" % (a, b8)),
             ((b8 + ".ktab", b), "tabcmp: K of %s.ktab (8) and %s (12) differ\n" % (b8, b)),
             ((a, b, os.path.join(d, "no_such_dir", "out")), "tabcmp: Cannot open %s/no_such_dir/out.cmp for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    r = run("-", a)                                        # a bare "-" is an operand, not an option that is dropped
    assert (r.returncode, r.stdout) == (1, "") and r.stderr.startswith("tabcmp: Cannot open ") and "-.ktab" in r.stderr
    assert listing(d) == before
    os.mkdir(out + ".cmp")                                 # the .cmp cannot be created: a directory has its name
    before = listing(d)
    r = run("-q", a, b, out)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabcmp: Cannot open %s.cmp for 'w'\n" % out)
    assert listing(d) == before


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how, side):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    ops = [os.path.join(d, "o:ther"), os.path.join(d, "tab")]
    r = run(ops[1 - side], ops[side], os.path.join(d, "out"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabcmp: " + msg), how
    assert listing(d) == before


# ---- cp_kmer_qv ----

def test_kmer_qv_against_the_oracle(built):
    from classpro_amd.api import kmer_qv
    for K in (1, 5, 21, 31, 40, 63):
        for a_only, a_total in ((1, 2), (1, 10), (7, 1000), (123456, 3_000_000_000), (999, 1000), (5, 5)):
            (q, e), (wq, we) = kmer_qv(K, a_only, a_total), CO.qv(K, a_only, a_total)
            assert abs(e - we) <= 1e-12 * abs(we), (K, a_only, a_total)
            assert abs(q - wq) <= 1e-12 * abs(wq), (K, a_only, a_total)
        assert kmer_qv(K, 0, 17) == (math.inf, 0.0)


def test_kmer_qv_rejects_and_exports(built):
    import ctypes as C
    from classpro_amd import _lib
    from classpro_amd._lib import ClassProError
    from classpro_amd.api import kmer_qv
    L = _lib.lib()
    assert {"cp_kmer_sorted_compare_hist", "cp_kmer_qv"} <= set(_lib.SYMBOLS)
    assert len(L.cp_kmer_sorted_compare_hist.argtypes) == 8 and len(L.cp_kmer_qv.argtypes) == 5
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "enum { CP_CMP_KEYS = 0, CP_CMP_A = 1, CP_CMP_B = 2 };" in hdr
    for K, a_only, a_total in ((0, 1, 2), (-3, 1, 2), (21, 1, 0), (21, 0, 0), (21, 1, -5), (21, -1, 10), (21, 11, 10)):
        with pytest.raises(ClassProError) as ei:
            kmer_qv(K, a_only, a_total)
        assert ei.value.code == -1
    q, e = C.c_double(), C.c_double()
    assert L.cp_kmer_qv(21, 1, 2, None, C.byref(e)) == -1 and L.cp_kmer_qv(21, 1, 2, C.byref(q), None) == -1
    assert L.cp_kmer_qv(21, 1, 2, C.byref(q), C.byref(e)) == 0 and q.value > 0      # the library is usable afterwards
    # the arguments of the comparison are checked before the device is touched
    m = np.zeros(4, np.int64)
    assert L.cp_kmer_sorted_compare_hist(None, None, None, 0, 1, 1, m.ctypes.data, None) == -1

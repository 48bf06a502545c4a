"""Read hits in two k-mer tables, the part that needs no GPU: cp_bin_call against the rule restated in
tests/readhits_oracle.py (ties, min_markers, a weight of 0, products past 64 bits), the oracle's rows on reads whose
markers are written out, the two exports, the argument errors of cp_kmer_sorted_read_hits that come before the device,
and every error tabbin reports before it touches the GPU (exact stderr, exit 1, nothing on stdout, no file created).
Everything is integers: the tolerance is zero."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import ktab_oracle as KO
import readhits_oracle as RO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_tabprof_host import NO_GPU, SPOILED, listing, spoil

TOOL = os.path.join(ROOT, "classpro_amd", "tabbin")
USAGE = ("Usage: tabbin [-v] [-u] [-m<int(1)>] [-b<int(67108864)>] [-o<out_root>]\n"
         "              <A>[.ktab][:<lo>-<hi>] <B>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]\n")
K0, K1 = 12, 8


# ---- the oracle itself ----

def test_oracle_rows_on_written_markers():
    assert RO.row_of("AA.B2BA") == [3, 2, 1, 0, 2]
    assert RO.row_of("") == [0, 0, 0, 0, 0] and RO.row_of("..2o2..") == [0, 0, 2, 1, 0]
    assert RO.row_of("A.o.2.A") == [2, 0, 1, 1, 0] and RO.row_of("ABABAB") == [3, 3, 0, 0, 5]
    assert RO.row_of("B" + "." * 50 + "A") == [1, 1, 0, 0, 1]
    K = 5
    a = [(KO.key_of(b"AAAAA"), 3), (KO.key_of(b"AACGT"), 1), (KO.key_of(b"CCCCC"), 9)]
    b = [(KO.key_of(b"AACGT"), 2), (KO.key_of(b"ACGTA"), 5)]
    seqs = [b"AAAAACGTAC", b"TTTTT", b"ACGT", b"", b"AACGTNAAAAA", b"aaaaa"]
    #  AAAAACGTAC: AAAAA A | AAAAC . | AAACG . | AACGT 2 | ACGTA B | CGTAC = rc GTACG, canonical CGTAC .
    assert [RO.markers(s, K, RO.present(a, None), RO.present(b, None)) for s in seqs] == ["A..2B.", "A", "", "", "2oooooA", "o"]
    assert RO.rows(a, b, seqs, K) == [[1, 1, 1, 0, 1], [1, 0, 0, 0, 0], [0] * 5, [0] * 5, [1, 0, 1, 5, 0], [0, 0, 0, 1, 0]]
    assert RO.rows(a, b, seqs[:1], K, a_range=(2, None)) == [[1, 2, 0, 0, 1]]         # AACGT leaves A: it marks B now
    assert RO.rows(a, b, seqs[:2], K, canonical=False) == [[1, 1, 1, 0, 1], [0] * 5]
    assert RO.only(a, b) == (2, 1) and RO.only(a, b, (2, None), (None, 2)) == (2, 1) and RO.only(a, a) == (0, 0)


# ---- cp_bin_call ----

def bin_call(L, row, only_a, only_b, min_markers, normalise):
    h = (C.c_int64 * 5)(*row)
    return chr(L.cp_bin_call(h, only_a, only_b, min_markers, normalise))


def test_bin_call_against_the_rule(built):
    from classpro_amd._lib import lib
    from classpro_amd.api import bin_calls
    L = lib()
    big = 1 << 40
    cases = [([0, 0, 9, 9, 0], 5, 5, 1, 1, "U"),                                     # no marker at all
             ([1, 0, 0, 0, 0], 5, 5, 1, 1, "A"), ([0, 1, 0, 0, 0], 5, 5, 1, 1, "B"),
             ([3, 3, 0, 0, 5], 5, 5, 1, 1, "U"),                                     # a tie
             ([3, 3, 0, 0, 5], 10, 5, 1, 1, "B"), ([3, 3, 0, 0, 5], 5, 10, 1, 1, "A"),   # the smaller set weighs more
             ([3, 3, 0, 0, 5], 10, 5, 1, 0, "U"),                                    # -u: a tie again
             ([2, 4, 0, 0, 0], 10, 20, 1, 1, "U"), ([2, 4, 0, 0, 0], 10, 21, 1, 1, "A"), ([2, 4, 0, 0, 0], 10, 19, 1, 1, "B"),
             ([2, 1, 0, 0, 0], 5, 5, 3, 1, "A"), ([2, 1, 0, 0, 0], 5, 5, 4, 1, "U"),   # min_markers counts nA + nB
             ([4, 0, 7, 7, 0], 5, 5, 5, 1, "U"),                                     # BOTH and OTHER are no markers
             ([2, 3, 0, 0, 0], 0, 1000, 1, 1, "B"), ([2, 3, 0, 0, 0], 1000, 0, 1, 1, "B"),   # a weight of 0: not normalised
             ([3, 2, 0, 0, 0], 0, 0, 1, 1, "A"), ([2, 3, 0, 0, 0], 1, 1000, 1, 1, "A"),
             ([big, big + 1, 0, 0, 0], 1 << 50, 1 << 50, 1, 1, "B"),                 # products of 2^90: equal modulo 2^64
             ([big, big, 0, 0, 0], (1 << 50) + 1, 1 << 50, 1, 1, "B"),
             ([big, big, 0, 0, 0], 1 << 50, (1 << 50) + 1, 1, 1, "A"),
             ([big, 1, 0, 0, 0], 1, 1 << 50, 1, 1, "A"),                             # nA * wB = 2^90 against 1
             ([1 << 24, 1, 0, 0, 0], 1 << 24, 1, 1, 1, "U"),                         # 2^24 * 1 == 1 * 2^24
             ([1 << 62, 1 << 62, 0, 0, 0], 6, 7, RO.BIG, 1, "A")]                    # the sum 2^63 is not below 2^63-1
    for row, oa, ob, mm, nz, want in cases:
        assert RO.call(row, oa, ob, mm, bool(nz)) == want, (row, oa, ob, mm, nz)
        assert bin_call(L, row, oa, ob, mm, nz) == want, (row, oa, ob, mm, nz)
    rng = random.Random(9)
    for _ in range(3000):
        top = rng.choice([3, 10, 1 << 20, 1 << 62])
        row = [rng.randrange(top), rng.randrange(top), rng.randrange(5), rng.randrange(5), rng.randrange(5)]
        if rng.random() < 0.3:
            row[1] = row[0]
        oa, ob = (rng.choice([0, 1, 2, 3, 1 << 33, RO.BIG, rng.randrange(1, 1 << 62)]) for _ in range(2))
        mm, nz = rng.choice([1, 2, 5, top, 2 * top - 1]), rng.randrange(2)
        assert bin_call(L, row, oa, ob, mm, nz) == RO.call(row, oa, ob, mm, bool(nz)), (row, oa, ob, mm, nz)
    rows = np.array([c[0] for c in cases[:13]], np.int64)                             # the Python form: one set of weights
    assert bin_calls(rows, 10, 5) == "".join(RO.call(r, 10, 5) for r in rows.tolist()).encode()
    assert bin_calls(rows, 10, 5, min_markers=4, normalise=False) == "".join(RO.call(r, 10, 5, 4, False) for r in rows.tolist()).encode()
    assert bin_calls(np.zeros((0, 5), np.int64), 1, 1) == b""
    assert L.cp_bin_call(None, 1, 1, 1, 1) == -1


def test_library_exports(built):
    from classpro_amd import _lib
    L = _lib.lib()
    assert {"cp_kmer_sorted_read_hits", "cp_bin_call"} <= set(_lib.SYMBOLS)
    assert len(L.cp_kmer_sorted_read_hits.argtypes) == 10 and len(L.cp_bin_call.argtypes) == 5
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert ("enum { CP_HIT_A = 0, CP_HIT_B = 1, CP_HIT_BOTH = 2, CP_HIT_OTHER = 3, CP_HIT_SWITCHES = 4, CP_HIT_WIDTH = 5 };"
            in hdr)
    # arguments are checked before the device is touched
    assert L.cp_kmer_sorted_read_hits(None, None, 1, None, None, None, 0, 0, None, None) == -1
    assert L.cp_kmer_sorted_read_hits(None, None, 1, None, None, None, 3, 100, None, None) == -1
    assert b"cp_kmer_sorted_read_hits" in L.cp_last_error()


# ---- tabbin before the GPU ----

@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """Two tables at K = 12 (`tab` is the one spoil() spoils), one at K = 8 and a source."""
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("readhits_host"))
    for name, k, seed, parts in (("tab", K0, 5, 3), ("o:ther", K0, 7, 1), ("tab8", K1, 5, 2)):
        ents = KO.table(mixed_reads(k, seed), k)
        fastk.write_fastk_ktab(d, name, k, 1, [x for x, _ in ents], [c for _, c in ents], parts)
    with open(os.path.join(d, "reads.fasta"), "wb") as f:
        f.write(b">r1\nACGTACGTACGTACGTACGTACGTACGT\n")
    return d


def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    a, b, b8, src = os.path.join(d, "tab"), os.path.join(d, "o:ther.ktab"), os.path.join(d, "tab8"), os.path.join(d, "reads")
    out = os.path.join(d, "out")
    before = listing(d)
    cases = [((), USAGE), ((a,), USAGE), ((a, b), USAGE), ((a, b, src, src), USAGE), (("-v", "-u", "-m2", "-b5", "-oout"), USAGE),
             (("-x", a, b, src), "tabbin: -x is an illegal option\n"),
             (("-vq", a, b, src), "tabbin: -q is an illegal option\n"),
             (("-uv", "-T4", a, b, src), "tabbin: -T is an illegal option\n"),
             (("-mx", a, b, src), "tabbin: -m 'x' argument is not an integer\n"),
             (("-m", a, b, src), "tabbin: -m '' argument is not an integer\n"),
             (("-b1e6", a, b, src), "tabbin: -b '1e6' argument is not an integer\n"),
             (("-m0", a, b, src), "tabbin: Minimum number of markers must be positive (0)\n"),
             (("-m-3", a, b, src), "tabbin: Minimum number of markers must be positive (-3)\n"),
             (("-b0", a, b, src), "tabbin: Bases per device batch must be positive (0)\n"),
             ((a + ":0-3", b, src), "tabbin: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             ((a, b + ":5-2", src), "tabbin: Count range of %s needs 1 <= lo <= hi (5-2)\n" % b),
             ((a + ":3-7", b + ":0-", src), "tabbin: Count range of %s needs 1 <= lo <= hi (0-)\n" % b),
             ((a + ":3", b, src), "tabbin: Cannot open %s:3.ktab [errno=2]\n" % a),          # no range: part of the path
             ((a, b8, src), "tabbin: K of %s.ktab (12) and %s.ktab (8) differ\n" % (a, b8)),
             ((b8 + ".ktab:2-", b + ":-9", src), "tabbin: K of %s.ktab (8) and %s (12) differ\n" % (b8, b)),
             ((a, b, os.path.join(d, "nothing")),
              "tabbin: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d),
             (("-o" + os.path.join(d, "no_such_dir", "out"), a, b, src),
              "tabbin: Cannot open %s/no_such_dir/out.A.fasta for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".U.fasta")                             # the third file cannot be created: a directory has its name
    open(out + ".B.fasta", "w").write("kept\n")            # and the second was there before
    before = listing(d)
    r = run("-o" + out, a, b, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabbin: Cannot open %s.U.fasta for 'w'\n" % out)
    assert listing(d) == before                            # the first, created here, is gone again


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how, side):
    d = str(tmp_path / "case")
    shutil.copytree(good, d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    ops = [os.path.join(d, "o:ther"), os.path.join(d, "tab")]
    r = run("-o" + os.path.join(d, "out"), ops[1 - side], ops[side], os.path.join(d, "reads.fasta"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabbin: " + msg), how
    assert listing(d) == before

"""Looking k-mers up in FASTK k-mer tables, the part that needs no GPU: the lookup oracle of tests/tabprof_oracle.py
against the reference's own Load_Kmer_Table / Find_Kmer / Fetch_Count (compiled into oracle/_ref), fastk.read_fastk_ktab_raw
against read_fastk_ktab, the errors tab2prof reports before it touches the GPU (exact stderr, exit 1, no file created),
and the table reader of the tool (csrc/host/ktab_reader.h) driven by tests/ktab_reader_check.cpp under AddressSanitizer
and UBSan on the same good and bad files.  Everything is bytes and integers: the tolerance is zero."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import kprof_oracle as O
import ktab_oracle as KO
import tabprof_oracle as TO
from conftest import ROOT, build_if_changed
from test_gpu_ktab import mixed_reads
from test_ktab_host import KS

TOOL = os.path.join(ROOT, "classpro_amd", "tab2prof")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
ASAN = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")      # a reader that dies does not free what it holds
USAGE = ("Usage: tab2prof [-v] [-C] [-T<int(4)>] [-b<int(67108864)>] [-N<out_root>]\n"
         "                <table>[.ktab] <source>[.db|.dam|.f[ast][aq][.gz]]\n")


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_oracle_against_the_reference(tmp_path, K, nparts):
    """The cell of every k-mer of mixed_reads is the count at Find_Kmer's index, 0 for -1; with three parts of the few
    entries of K = 5 cut so that one part is empty."""
    import ctypes as C
    from classpro_amd import fastk
    L = KO.ref_lib()
    if L is None:
        pytest.skip("the reference's own readers (oracle/_ref) are not built here")
    L.Fetch_Count.restype = C.c_int
    L.Fetch_Count.argtypes = [C.c_void_p, C.c_int64]
    seqs = mixed_reads(K)
    ents = KO.table(seqs[:5], K)[::2]                      # every other k-mer of some of the reads: hits and misses
    if nparts == 3:
        ents = ents[:2]                                    # three parts of two entries: the first part is empty
    fastk.write_fastk_ktab(str(tmp_path), "tab", K, 1, [k for k, _ in ents], [c for _, c in ents], nparts)
    if nparts == 3:
        assert struct.unpack("<iq", open(str(tmp_path / ".tab.ktab.1"), "rb").read(12)) == (K, 0)
    T = KO.RefTable(L, str(tmp_path / "tab"))
    prof, tally = TO.cells(ents, seqs, K)
    hits = 0
    for s, p in zip(seqs, prof):
        keys = TO.read_keys(s, K)
        fw = TO.read_keys(s, K, canonical=False)
        assert len(keys) == len(p) == max(len(s) - K + 1, 0)
        for i, k in enumerate(keys):
            if k is None:
                assert p[i] == 0
                continue
            at = T.find(KO.text_of(fw[i], K))              # the forward k-mer: Find_Kmer takes the canonical one itself
            assert at == TO.find(ents, [k])[0]
            assert int(p[i]) == (L.Fetch_Count(T.T, at) if at >= 0 else 0)
            hits += at >= 0
    assert hits == tally[0] > 0 and tally[1] > 0 and tally[2] > 0
    T.close()


def test_forward_and_canonical_keys_of_the_oracle():
    K = 5
    ents = [(KO.key_of(b"AAAAA"), 40000), (KO.key_of(b"AACGT"), 7)]     # both canonical: rc(AACGT) = ACGTT is larger
    prof, tally = TO.cells(ents, [b"AACGTTN", b"TTTTT", b"ACG", b""], K)
    assert [p.tolist() for p in prof] == [[7, 7, 0], [32767], [], []] and tally == [3, 0, 1]
    prof, tally = TO.cells(ents, [b"AACGTTN", b"TTTTT"], K, canonical=False)
    assert [p.tolist() for p in prof] == [[7, 0, 0], [0]] and tally == [1, 2, 1]
    assert TO.find(ents, [KO.key_of(b"AACGT"), 5, KO.key_of(b"AAAAA")]) == [1, -1, 0]


@pytest.mark.parametrize("K", KS)
def test_raw_reader_round_trip(tmp_path, K):
    from classpro_amd import fastk
    ents = KO.table(mixed_reads(K), K)
    for nparts in (1, 3, len(ents) + 2) if K < 13 else (3,):   # an index of 128 MiB is written once
        d = str(tmp_path / ("p%d" % nparts))
        fastk.write_fastk_ktab(d, "tab", K, 2, [k for k, _ in ents], [c for _, c in ents], nparts)
        k, m, ib, index, rec = fastk.read_fastk_ktab_raw(d, "tab")
        k2, m2, ib2, keys, counts = fastk.read_fastk_ktab(d, "tab")
        assert (k, m, ib) == (k2, m2, ib2) == (K, 2, KO.ibyte_of(K))
        assert index.dtype == np.int64 and rec.dtype == np.uint8
        assert np.array_equal(index, KO.index(ents, K)) and rec.tobytes() == KO.records(ents, K)
        assert keys == [x for x, _ in ents] and counts.tolist() == [min(c, KO.MAXC) for _, c in ents]
    open(os.path.join(d, ".tab.ktab.2"), "ab").write(b"\0")
    with pytest.raises(ValueError):
        fastk.read_fastk_ktab_raw(d, "tab")


# ---- tab2prof before the GPU, and the reader under the sanitizers ----

K0 = 12


@pytest.fixture(scope="module")
def good(tmp_path_factory):
    """A table of three parts at K = 12 (an index of 512 KiB) and a source, in a directory that the cases copy."""
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("tabprof_host"))
    ents = KO.table(mixed_reads(K0), K0)
    fastk.write_fastk_ktab(d, "tab", K0, 1, [k for k, _ in ents], [c for _, c in ents], 3)
    with open(os.path.join(d, "reads.fasta"), "wb") as f:
        f.write(b">r1\nACGTACGTACGTACGTACGTACGTACGT\n")
    return d, ents


def patch(path, offset, data):
    with open(path, "r+b") as f:
        f.seek(offset)
        f.write(data)


def spoil(d, how):
    """Spoils the table under d; returns the message the reader gives, without the program's name."""
    stub, part2 = os.path.join(d, "tab.ktab"), os.path.join(d, ".tab.ktab.2")
    pbyte = ((K0 + 3) >> 2) - 2 + 2
    nels2 = struct.unpack("<q", open(part2, "rb").read()[4:12])[0]
    size2 = os.path.getsize(part2)
    n = sum(struct.unpack("<q", open(os.path.join(d, ".tab.ktab.%d" % p), "rb").read()[4:12])[0] for p in (1, 2, 3))
    if how == "no stub":
        os.remove(stub)
        return "Cannot open %s [errno=2]\n" % stub
    if how == "stub without a header":
        os.truncate(stub, 10)
        return "%s is truncated\n" % stub
    if how == "stub with a short index":
        os.truncate(stub, os.path.getsize(stub) - 1)
        return "%s is truncated\n" % stub
    if how == "K = 4":
        patch(stub, 0, struct.pack("<i", 4))
        return "K-mer length of %s must lie in [5, 63] (4)\n" % stub
    if how == "K = 64":
        patch(stub, 0, struct.pack("<i", 64))
        return "K-mer length of %s must lie in [5, 63] (64)\n" % stub
    if how == "wrong ibyte":
        patch(stub, 12, struct.pack("<i", 3))
        return "%s has 3 prefix bytes, a table of 12-mers has 2\n" % stub
    if how == "no parts":
        patch(stub, 4, struct.pack("<i", 0))
        return "%s names no parts (0)\n" % stub
    if how == "index decreases":
        patch(stub, 16 + 8 * 100, struct.pack("<q", -1))
        return "The index of %s is negative or decreases at prefix 100\n" % stub
    if how == "part missing":
        os.remove(part2)
        return "Table part %s is missing\n" % part2
    if how == "part without a header":
        os.truncate(part2, 11)
        return "Table part %s is truncated\n" % part2
    if how == "part of another K":
        patch(part2, 0, struct.pack("<i", 13))
        return "Table part %s does not have the k-mer length of the stub (13 vs 12)\n" % part2
    if how == "part one byte short":
        os.truncate(part2, size2 - 1)
        return "Table part %s holds %d bytes, its %d records of %d bytes need %d\n" % (part2, size2 - 1, nels2, pbyte, size2)
    if how == "nels sum differs":
        patch(part2, 4, struct.pack("<q", nels2 + 1))
        open(part2, "ab").write(b"\xff" * pbyte)
        return "The parts of %s hold %d entries, its index ends at %d\n" % (stub, n + 1, n)
    raise AssertionError(how)


SPOILED = ["no stub", "stub without a header", "stub with a short index", "K = 4", "K = 64", "wrong ibyte", "no parts",
           "index decreases", "part missing", "part without a header", "part of another K", "part one byte short",
           "nels sum differs"]


def listing(d):
    return sorted(os.path.join(r, f)[len(d):] for r, _d, fs in os.walk(d) for f in fs + _d)


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    msg = spoil(d, how)
    before = listing(d)
    for flags in ([], ["-C"]):
        r = subprocess.run([TOOL] + flags + [os.path.join(d, "tab"), os.path.join(d, "reads")], capture_output=True, text=True,
                           env=NO_GPU)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "tab2prof: " + msg), how
        assert listing(d) == before


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    tab, src = os.path.join(d, "tab.ktab"), os.path.join(d, "reads.fasta")
    before = listing(d)
    go = lambda *a: subprocess.run([TOOL] + list(a), capture_output=True, text=True, env=NO_GPU)
    cases = [((), USAGE), ((tab,), USAGE), ((tab, src, src), USAGE), (("-v", "-C", "-T2"), USAGE),
             (("-x", tab, src), "tab2prof: -x is an illegal option\n"),
             (("-vq", tab, src), "tab2prof: -q is an illegal option\n"),
             (("-Tx", tab, src), "tab2prof: -T 'x' argument is not an integer\n"),
             (("-T", tab, src), "tab2prof: -T '' argument is not an integer\n"),
             (("-b1e6", tab, src), "tab2prof: -b '1e6' argument is not an integer\n"),
             (("-T0", tab, src), "tab2prof: Number of threads must be positive (0)\n"),
             (("-b0", tab, src), "tab2prof: Bases per device batch must be positive (0)\n"),
             ((tab, os.path.join(d, "nothing")),
              "tab2prof: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d),
             (("-N" + os.path.join(d, "no_such_dir", "out"), tab, src),
              "tab2prof: Cannot open %s/no_such_dir/out.prof for 'w'\n" % d)]
    for args, msg in cases:
        r = go(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(os.path.join(d, "reads.rel.class"))           # the .class cannot be created: a directory has its name
    before = listing(d)
    r = go("-C", tab, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tab2prof: Cannot open %s/reads.rel.class for 'w'\n" % d)
    assert listing(d) == before                            # the stub opened before it is gone again


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "ktab_reader_check.cpp")
    out = os.path.join(ROOT, "tests", "_ktab_reader_check")
    deps = [src] + [os.path.join(ROOT, "classpro_amd", "csrc", "host", f) for f in ("ktab_reader.h", "host_io.h")]
    return build_if_changed(out, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                  "-o", out, src, "-lz"], deps)


@pytest.mark.parametrize("K,piece", [(12, 1), (12, 7), (12, 100), (12, 10**6), (21, 64)])
def test_reader_under_the_sanitizers(checker, tmp_path, K, piece):
    """Two and three prefix bytes, three parts, pieces that end inside a part, at its end and past the table."""
    from classpro_amd import fastk
    d, ents = str(tmp_path), KO.table(mixed_reads(K), K)
    fastk.write_fastk_ktab(d, "tab", K, 1, [k for k, _ in ents], [c for _, c in ents], 3)
    ib = KO.ibyte_of(K)
    n, pbyte, isize = len(ents), ((K + 3) >> 2) - ib + 2, 8 << (8 * ib)
    for name in ("tab", "tab.ktab"):
        r = subprocess.run([checker, os.path.join(d, name), str(piece)], capture_output=True, env=ASAN)
        assert r.returncode == 0 and r.stderr == b"", r.stderr.decode(errors="replace")[-2000:]
        head, rest = r.stdout.split(b"\n", 1)
        assert head == b"%d 3 1 %d %d %d" % (K, ib, pbyte, n)
        assert rest[:isize] == KO.index(ents, K).astype("<i8").tobytes()
        assert rest[isize:isize + n * pbyte] == KO.records(ents, K)
        assert rest[isize + n * pbyte:] == b"pieces %d\n" % -(-n // piece)


def test_reader_under_the_sanitizers_small_index_and_empty_parts(checker, tmp_path):
    from classpro_amd import fastk
    ents = KO.table(mixed_reads(8), 8)[:2]
    fastk.write_fastk_ktab(str(tmp_path), "t", 8, 1, [k for k, _ in ents], [c for _, c in ents], 5)
    r = subprocess.run([checker, str(tmp_path / "t"), "1"], capture_output=True, env=ASAN)
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == b"8 5 1 1 3 2\n" + KO.index(ents, 8).astype("<i8").tobytes() + KO.records(ents, 8) + b"pieces 2\n"
    fastk.write_fastk_ktab(str(tmp_path), "e", 8, 1, [], [], 1)
    r = subprocess.run([checker, str(tmp_path / "e"), "4"], capture_output=True, env=ASAN)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"8 1 1 1 3 0\n" + bytes(8 << 8) + b"pieces 0\n"


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_under_the_sanitizers(checker, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    msg = spoil(d, how)
    r = subprocess.run([checker, os.path.join(d, "tab"), "64"], capture_output=True, text=True, env=ASAN)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "ktab_reader_check: " + msg), how

"""Fixing reads from a k-mer table, the part that needs no GPU: the oracle of tests/fix_oracle.py on reads built by hand
whose records are written out, the identity between the NONE positions before and after, the first-principles case (reads
with spaced errors come back as the genome's pieces, every one of them), the rule of classpro_amd/csrc/fx_rule.h on the host
under AddressSanitizer and UBSan against the oracle (tests/fx_rule_check.cpp), the exports, and every error tabfix reports
before it touches the GPU (exact stderr, exit 1, nothing on stdout, no file created).  Everything is integers and bytes: the
tolerance is zero."""
import os
import random
import shutil
import subprocess

import pytest

import fix_oracle as FO
from conftest import ROOT, build_if_changed
from test_tabprof_host import NO_GPU, SPOILED, good, listing, spoil          # noqa: F401  (good: a table at K = 12 and a source)

TOOL = os.path.join(ROOT, "classpro_amd", "tabfix")
USAGE = ("Usage: tabfix [-v] [-d<int(1)>] [-b<int(67108864)>] [-o<out_root>]\n"
         "              <table>[.ktab][:<lo>-<hi>] <source>[.db|.dam|.f[ast][aq][.gz]]\n")

T = b"ACGGTCATTGCACTAGGATCCGTA"                             # 24 bases, every 5-mer once
H = b"ACGGTCAAAAGCACTAGGATCCGTA"                            # with a homopolymer of four
R = b"ACGGTCAGAGCCTAGGATCCGTA"                              # with two copies of AG
C3 = b"TCACCGACTCTCCTCGTGGTGAGCAC"


def edit(t, p, d, ins):
    return t[:p] + ins + t[p + d:]


# (name, K, D, the sequences of the table, the read, [(first, last, status, del, nacc, ins)])
HAND = [
    ("substitution", 5, 1, [T], edit(T, 11, 1, b"G"), [(7, 11, FO.ONE, 1, 1, b"A")]),
    ("substitution with -d0", 5, 0, [T], edit(T, 11, 1, b"G"), [(7, 11, FO.ONE, 1, 1, b"A")]),
    ("insertion", 5, 1, [T], edit(T, 11, 0, b"T"), [(7, 11, FO.ONE, 1, 1, b"")]),
    ("insertion of two", 5, 2, [T], edit(T, 11, 0, b"TG"), [(7, 12, FO.ONE, 2, 1, b"")]),
    ("insertion with -d0: no candidate but the substitutions", 5, 0, [T], edit(T, 11, 0, b"T"), [(7, 11, FO.NONE, 0, 0, b"")]),
    ("deletion", 5, 1, [T], edit(T, 11, 1, b""), [(7, 9, FO.ONE, 0, 1, b"A")]),
    ("homopolymer one longer", 5, 1, [H], edit(H, 8, 0, b"A"), [(6, 6, FO.ONE, 1, 1, b"")]),
    ("homopolymer one shorter", 5, 1, [H], edit(H, 8, 1, b""), [(5, 5, FO.ONE, 0, 1, b"A")]),
    ("tandem copy lost", 5, 2, [R], edit(R, 6, 2, b""), [(4, 5, FO.ONE, 0, 1, b"AG")]),
    ("tandem copy lost, D too small", 5, 1, [R], edit(R, 6, 2, b""), [(4, 5, FO.NONE, 0, 0, b"")]),
    ("tandem copy gained", 5, 2, [R], edit(R, 6, 0, b"AG"), [(6, 7, FO.ONE, 2, 1, b"")]),
    ("open at the start", 5, 1, [T], edit(T, 1, 1, b"T"), [(0, 1, FO.OPEN, 0, 0, b"")]),
    ("open at the end", 5, 1, [T], edit(T, 22, 1, b"C"), [(18, 19, FO.OPEN, 0, 0, b"")]),
    ("an N behind the gap", 5, 1, [T], edit(edit(T, 11, 1, b"G"), 16, 1, b"N"), [(7, 11, FO.OPEN, 0, 0, b"")]),
    ("an N before the gap", 5, 1, [T], edit(edit(T, 11, 1, b"G"), 6, 1, b"N"), [(7, 11, FO.OPEN, 0, 0, b"")]),
    ("an N farther off", 5, 1, [T], edit(edit(T, 11, 1, b"G"), 17, 1, b"N"), [(7, 11, FO.ONE, 1, 1, b"A")]),
    ("three wrong bases: g = 3 > D", 5, 1, [T], edit(T, 10, 3, b"GGG"), [(6, 12, FO.NOCAND, 0, 0, b"")]),
    ("three wrong bases: g = 3 <= D", 5, 4, [T], edit(T, 10, 3, b"GGG"), [(6, 12, FO.NONE, 0, 0, b"")]),
    ("both alternatives in the table", 5, 1, [T, edit(T, 11, 1, b"T")], edit(T, 11, 1, b"G"), [(7, 11, FO.MANY, 0, 2, b"")]),
    ("the k-mers across are not in the table", 5, 1, [T[:12], T[11:]], edit(T, 11, 1, b"G"), [(7, 11, FO.NONE, 0, 0, b"")]),
    ("a clash with D = 3", 5, 3, [C3], b"TCACGCGACTCTCCTCGTGGTGCTAAGCAC",
     [(0, 4, FO.OPEN, 0, 0, b""), (18, 18, FO.CLASH, 3, 1, b""), (20, 24, FO.CLASH, 3, 1, b"")]),
]


@pytest.mark.parametrize("which", range(len(HAND)))
def test_hand_cases(which):
    name, K, D, tabs, s, want = HAND[which]
    assert 20 <= len(s) <= 30
    ents = FO.table(tabs, K)
    off, recs, tally = FO.read_fixes(ents, [s], K, D)
    assert [(r[0], r[1], r[3], r[4], r[6], r[7].rstrip(b"\0")) for r in recs] == want, name
    assert off == [0, len(want)] and sum(tally) == len(want) and all(r[5] == len(r[7].rstrip(b"\0")) for r in recs)
    fixed = FO.apply([s], off, recs, K)[0]
    if all(w[2] == FO.ONE for w in want):
        at = s.find(b"N")                                  # the read comes back, but for an N it holds
        assert fixed == (tabs[0] if at < 0 else edit(tabs[0], at, 1, b"N")) != s, name
    else:
        assert fixed == s, name                            # nothing is applied


def test_the_clash_is_two_ones_that_overlap():
    """Without the rule both fixes of the clash case are ONE, and the bases the first removes reach behind the second's e."""
    name, K, D, tabs, s, want = HAND[-1]
    present = {k for k, _ in FO.table(tabs, K)}
    (i1, j1, _), (i2, j2, _) = FO.gaps_of(FO.marks_of(s, K, present))[1:]
    a1 = [c for c in FO.candidates(s, K, i1, j1, D) if FO.accepted(s, K, i1, c[0], c[1], present)]
    a2 = [c for c in FO.candidates(s, K, i2, j2, D) if FO.accepted(s, K, i2, c[0], c[1], present)]
    assert len(a1) == len(a2) == 1 and i1 + K - 1 + a1[0][0] > i2 + K - 1
    assert len(FO.candidates(s, K, i2, j2, D)) <= 2 * D + 3


def test_candidates_are_different_strings():
    rng = random.Random(5)
    for _ in range(300):
        K, D = rng.choice([5, 7, 9]), rng.randint(0, 4)
        s = bytes(rng.choice(FO.ACGT[:2 + rng.randint(0, 2)]) for _ in range(60))
        i = rng.randint(1, 20)
        j = i + rng.randint(0, K + 4)
        cand = FO.candidates(s, K, i, j, D)
        assert len(cand) <= 2 * D + 3
        assert len({FO.edited(s, i + K - 1, d, ins) for d, ins in cand}) == len(cand)


def isolated(recs, K):
    """Whether the identity of the NONE positions is a theorem for this read: every applied fix stands alone.  A fix at e
    that removes del bases takes the k-mer positions [i, max(e+del, e)-1] of the read away and puts its checked window in
    their place; the window reads the bases [i, e+del+K-2].  So (1) no other gap may hold one of the positions taken away:
    the next gap begins behind e+del-1; and (2) no other applied edit may touch a base of the window: the next applied fix
    has e'' >= e+del+K-1, which also keeps this edit out of the window of the next.  Then every k-mer of the corrected read
    that holds an edited base lies in the window of that edit alone and is the string that was checked, every other k-mer is
    a k-mer of the read, and the positions taken away hold the L absent ones of the gap and present ones."""
    for k, r in enumerate(recs):
        if r[3] != FO.ONE:
            continue
        e, d = r[0] + K - 1, r[4]
        if k + 1 < len(recs) and recs[k + 1][0] <= e + d - 1:
            return False
        if any(x[3] == FO.ONE and x[0] + K - 1 < e + d + K - 1 for x in recs[k + 1:]):
            return False
    return True


@pytest.mark.parametrize("K,D", [(9, 1), (9, 4), (15, 2), (21, 3)])
def test_none_positions_after_the_fixes(K, D):
    """Unspaced errors: in every read whose applied fixes stand alone (`isolated`), the NONE positions afterwards number
    those before less the L of the applied gaps; the applied edits of every read are disjoint and ascending (apply_one
    asserts it).  Without the condition the identity is no theorem: at K = 9 with D = 1 the reads below lose 1178 NONE
    positions to fixes whose gaps hold 1135, because a removal of more than g+1 bases takes positions of the next gap
    with it."""
    rng = random.Random(K * 10 + D)
    g = FO.genome(K + D, 6000)
    ents = FO.table([g], K)
    present = {k for k, _ in ents}
    seqs = []
    for _ in range(60):
        a = rng.randrange(len(g) - 300)
        s = bytearray(g[a:a + 300])
        for _e in range(rng.randint(1, 12)):
            p = rng.randrange(len(s))
            kind = rng.randrange(3)
            if kind == 0:
                s[p] = rng.choice([c for c in FO.ACGT if c != s[p]])
            elif kind == 1:
                s[p:p] = bytes(rng.choice(FO.ACGT) for _ in range(rng.randint(1, D)))
            else:
                del s[p:p + rng.randint(1, 2)]
        seqs.append(bytes(s))
    off, recs, tally = FO.read_fixes(ents, seqs, K, D)
    fixed = FO.apply(seqs, off, recs, K)
    assert tally[FO.ONE] > 30 and sum(tally) - tally[FO.ONE] - tally[FO.OPEN] > 10
    alone = 0
    for r, s in enumerate(seqs):
        mine = recs[off[r]:off[r + 1]]
        if not isolated(mine, K):
            continue
        alone += 1
        applied = sum(x[1] - x[0] + 1 for x in mine if x[3] == FO.ONE)
        assert FO.none_count([fixed[r]], K, present) == FO.none_count([s], K, present) - applied, (r, mine)
    assert alone > len(seqs) // 2 and any(x[3] == FO.ONE for r in range(len(seqs)) for x in recs[off[r]:off[r + 1]])


@pytest.mark.parametrize("K,D,kinds,seed", [(21, 1, FO.KINDS1, 1), (21, 1, FO.KINDS1, 2), (40, 3, FO.KINDS3, 3), (21, 2, FO.KINDS3, 1)])
def test_spaced_errors_give_the_reads_back(K, D, kinds, seed):
    """Errors 3K apart on a genome with homopolymers and tandem repeats: every gap is fixed, every read comes back."""
    g, truth, reads, made = FO.read_set(seed, K, D, kinds, nreads=12 if K == 40 else 20)
    assert made == set(kinds) and all(a != b for a, b in zip(truth, reads))
    ents = FO.table([g], K)
    off, recs, tally = FO.read_fixes(ents, reads, K, D)
    assert tally[FO.ONE] == sum(tally) > 100
    assert FO.apply(reads, off, recs, K) == truth


def test_command_text():
    K = 5
    seqs = [h[4] for h in HAND[:4]] + [HAND[-1][4], b"ACG", b""]
    names = ["r%d" % i for i in range(len(seqs))]
    line, fasta, tsv = FO.tabfix(FO.table([T, C3], K), names, seqs, K, 1)
    assert line == ("tabfix: 7 sequences, 7 gaps, 3 fixed (2 substitutions, 1 insertions removed, 0 deletions filled), "
                    "0 ambiguous, 2 unfixed, 1 open, 1 without candidate, 0 clashes\n")
    assert tsv == b"r0\t11\tG\tA\nr1\t11\tG\tA\nr2\t11\tT\t\n"
    assert fasta.startswith(b">r0 (null)\n" + T + b"\n>r1 (null)\n" + T + b"\n") and fasta.endswith(b">r5 (null)\nACG\n>r6 (null)\n\n")


# ---- fx_rule.h on the host ----

def test_rule_on_the_host():
    """classpro_amd/csrc/fx_rule.h compiles for the host: tests/fx_rule_check.cpp runs its candidates and windows over random
    closed gaps and its apply map over random edit lists in walks of 64 bases, under AddressSanitizer and UBSan; what it
    prints is what the oracle gives."""
    src = os.path.join(ROOT, "tests", "fx_rule_check.cpp")
    exe = os.path.join(ROOT, "tests", "_fx_rule_check")
    inc = os.path.join(ROOT, "classpro_amd", "csrc")
    build_if_changed(exe, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + inc,
                           "-o", exe, src], [src, os.path.join(inc, "fx_rule.h")])
    n = 3000
    r = subprocess.run([exe, str(n), "7"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "wild %d" % n
    at, gaps, lists, ncand, applied = 0, 0, 0, 0, 0
    while lines[at] != "wild %d" % n:
        f = lines[at].split()
        at += 1
        if f[0] == "G":
            K, D, ln, i, j = map(int, f[1:6])
            e = i + K - 1
            s = b"A" * (e - 4) + f[6].encode() + b"A" * (ln - e - 1)
            want = []
            for d, ins in FO.candidates(s, K, i, j, D):
                hi = e + len(ins) - 1 if ins else e - 1
                want.append("c %d %d %s %d %d" % (d, len(ins), ins.decode() or "-", i, min(hi, ln - d + len(ins) - K)))
            have = []
            while lines[at] != "end":
                have.append(lines[at])
                at += 1
            at += 1
            assert have == want, lines[at - len(have) - 2]
            gaps, ncand = gaps + 1, ncand + len(want)
        else:
            assert f[0] == "A"
            K, ln, nrec = map(int, f[1:4])
            recs = []
            for k in range(nrec):
                x = lines[at + k].split()
                first, status, d, nins = map(int, x[1:5])
                ok = status == FO.ONE and d <= 4 and nins <= 4 and first + K - 1 + d <= ln
                recs.append((first, 0, 0, FO.ONE if ok else FO.NONE, d, nins, 0, b"" if x[5] == "-" else x[5].encode()))
                applied += ok
            s, out = lines[at + nrec].encode(), lines[at + nrec + 1].encode()
            at += nrec + 2
            assert len(s) == ln and out == FO.apply_one(s, recs, K), (K, ln, recs)
            lists += 1
    assert gaps == lists == n and ncand > 3 * n and applied > 3 * n


# ---- the exports ----

def test_library_exports(built):
    from classpro_amd import _lib
    from classpro_amd.api import SortedKmers
    L = _lib.lib()
    assert {"cp_kmer_sorted_read_fixes", "cp_apply_fixes"} <= set(_lib.SYMBOLS)
    assert len(L.cp_kmer_sorted_read_fixes.argtypes) == 14 and len(L.cp_apply_fixes.argtypes) == 12
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    assert "enum { CP_FIX_NONE = 0, CP_FIX_ONE = 1, CP_FIX_MANY = 2, CP_FIX_OPEN = 3, CP_FIX_NOCAND = 4, CP_FIX_CLASH = 5" in hdr
    assert ("typedef struct cp_kmer_fix { int64_t first, last; int32_t read; uint8_t status, del, nins, nacc; char ins[8]; } "
            "cp_kmer_fix;") in hdr
    assert hdr.index("Runs of k-mer states along reads (tabtrack)") < hdr.index("Fixing reads from a k-mer table (tabfix)") \
        < hdr.index("Count comparison of sorted k-mers")
    assert SortedKmers.FIX_TALLY == FO.STATUS
    assert (SortedKmers.FIX_NONE, SortedKmers.FIX_ONE, SortedKmers.FIX_MANY, SortedKmers.FIX_OPEN, SortedKmers.FIX_NOCAND,
            SortedKmers.FIX_CLASH) == (FO.NONE, FO.ONE, FO.MANY, FO.OPEN, FO.NOCAND, FO.CLASH)
    import ctypes as C
    count = C.c_int64(-7)                                  # the errors that come before the device
    assert L.cp_kmer_sorted_read_fixes(None, 1, None, 1, None, None, 0, 0, None, 0, None, C.byref(count), None, None) == -1
    assert b"cp_kmer_sorted_read_fixes" in L.cp_last_error()
    assert L.cp_apply_fixes(None, None, -1, 0, 21, None, None, None, 0, None, C.byref(count), None) == -1
    assert b"cp_apply_fixes" in L.cp_last_error() and count.value == -7
    S = SortedKmers.__new__(SortedKmers)
    S.s = None
    with pytest.raises(ValueError):
        S.read_fixes(None)
    with pytest.raises(ValueError):
        S.apply_fixes(None, None, None)


# ---- tabfix before the GPU ----

def run(*args):
    return subprocess.run([TOOL] + list(args), capture_output=True, text=True, env=NO_GPU)


def test_usage_errors_before_the_gpu(built, good, tmp_path):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    a, src, out = os.path.join(d, "tab"), os.path.join(d, "reads.fasta"), os.path.join(d, "out")
    before = listing(d)
    cases = [((), USAGE), ((a,), USAGE), (("-v", "-d2", a), USAGE), ((a, src, src), USAGE),
             (("-x", a, src), "tabfix: -x is an illegal option\n"),
             (("-vq", a, src), "tabfix: -q is an illegal option\n"),
             (("-dx", a, src), "tabfix: -d 'x' argument is not an integer\n"),
             (("-d", a, src), "tabfix: -d '' argument is not an integer\n"),
             (("-b1e3", a, src), "tabfix: -b '1e3' argument is not an integer\n"),
             (("-d5", a, src), "tabfix: Largest indel must lie in [0, 4] (5)\n"),
             (("-d-1", "-o" + out, a, src), "tabfix: Largest indel must lie in [0, 4] (-1)\n"),
             (("-b0", a, src), "tabfix: Bases per device batch must be positive (0)\n"),
             ((a + ":0-3", src), "tabfix: Count range of %s needs 1 <= lo <= hi (0-3)\n" % a),
             (("-o" + out, a + ":5-2", src), "tabfix: Count range of %s needs 1 <= lo <= hi (5-2)\n" % a),
             ((a + ":3", src), "tabfix: Cannot open %s:3.ktab [errno=2]\n" % a),                  # no range: part of the path
             (("-o" + out, os.path.join(d, "nothing"), src), "tabfix: Cannot open %s/nothing.ktab [errno=2]\n" % d),
             (("-o" + out, a, os.path.join(d, "nothing")),
              "tabfix: Cannot open %s/nothing as a .db|.dam or .f{ast}[aq][.gz] file\n" % d),
             (("-o" + os.path.join(d, "no_such_dir", "out"), a, src), "tabfix: Cannot open %s/no_such_dir/out.fixed.fasta for 'w'\n" % d)]
    for args, msg in cases:
        r = run(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args
    os.mkdir(out + ".fixes.tsv")                           # a directory has the second file's name: the first is not left behind
    before = listing(d)
    r = run("-o" + out, a, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabfix: Cannot open %s.fixes.tsv for 'w'\n" % out)
    assert listing(d) == before


@pytest.mark.parametrize("how", SPOILED)
def test_reader_errors_before_the_gpu(built, good, tmp_path, how):
    d = str(tmp_path / "case")
    shutil.copytree(good[0], d)
    msg = spoil(d, how)                                    # spoils `tab`
    before = listing(d)
    r = run("-d2", "-o" + os.path.join(d, "out"), os.path.join(d, "tab") + ":2-", os.path.join(d, "reads"))
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "tabfix: " + msg), how
    assert listing(d) == before

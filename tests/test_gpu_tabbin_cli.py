"""`tabbin` on a real MI355X (`-m gpu`): stdout, the summary line and the three files of -o byte for byte against
tests/readhits_oracle.py for a plain and a gzipped FASTA, with -u, -m, operand ranges and batches of a few reads, the -v
line, and the identity with tabop: two raw tables give the hits and calls that their two differences give."""
import gzip
import os
import random
import re
import subprocess

import pytest

import ktab_oracle as KO
import readhits_oracle as RO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_gpu_tabprof_cli import write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
K = 21
BIN = os.path.join(ROOT, "classpro_amd")


def tabbin(*args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, "tabbin")] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    """Two tables that share k-mers and differ in others, counts 1 to 3, and thirteen reads made of pieces of both read
    sets: reads that lean to either side, one with an N, one of K bases, one shorter than K and an empty one."""
    import torch
    from classpro_amd import fastk
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = str(tmp_path_factory.mktemp("tabbin_cli"))
    rng = random.Random(3)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    ra, rb = mixed_reads(K, 5), mixed_reads(K, 7)
    shared = rnd(600)
    p, q = KO.table(ra + [shared, rnd(2000)], K), KO.table(rb + [shared, shared], K)     # A's marker set is the larger one
    for name, ents, parts in (("P", p, 3), ("Q", q, 1)):
        fastk.write_fastk_ktab(d, name, K, 1, [x for x, _ in ents], [c for _, c in ents], parts)
    seqs = [ra[2][:1200], rb[2][:900], ra[1][:300] + rb[1][:300] + ra[1][300:600] + rb[1][300:350], shared[:200] + ra[0],
            rb[0][:K], rnd(K - 1), b"", ra[2][1000:1400] + b"N" + rb[2][1000:1500], rnd(300), rb[3] + shared[300:],
            ra[4][:100] + rb[4][:100], ra[3], rb[2][2000:]]
    names = ["read%d/%d" % (i, len(s)) for i, s in enumerate(seqs)]
    write_fasta(os.path.join(d, "reads.fasta"), names, seqs)
    with gzip.open(os.path.join(d, "zipped.fa.gz"), "wb") as f:
        f.write(open(os.path.join(d, "reads.fasta"), "rb").read())
    return dict(dir=d, p=p, q=q, names=names, seqs=seqs)


def test_output_against_the_oracle(case, tmp_path):
    d, t = case["dir"], str(tmp_path)
    p, q, names, seqs = case["p"], case["q"], case["names"], case["seqs"]
    P, Q = os.path.join(d, "P"), os.path.join(d, "Q.ktab")
    before = listing(d)
    out, summary, fasta = RO.tabbin(p, q, names, seqs, K)
    calls = [line.split("\t")[7] for line in out.splitlines()]
    assert len(calls) == 13 and {"A", "B", "U"} == set(calls) and " 0 reads with switches" not in summary
    assert RO.tabbin(p, q, names, seqs, K, normalise=False)[0] != out                  # a read with nA == nB: -u makes it U
    assert tabbin(P, Q, os.path.join(d, "reads")) == (out, summary)
    assert tabbin(P, Q, os.path.join(d, "zipped.fa.gz")) == (out, summary)
    assert listing(d) == before                            # without -o no file is written
    runs = [((), {}), (("-u",), dict(normalise=False)), (("-m3",), dict(min_markers=3)),
            (("-u", "-m400"), dict(normalise=False, min_markers=400)), (("-b700",), {}), (("-b1", "-u"), dict(normalise=False))]
    seen = set()
    for i, (flags, kw) in enumerate(runs):
        want_out, want_err, want_fa = RO.tabbin(p, q, names, seqs, K, **kw)
        root = os.path.join(t, "run%d" % i)
        assert tabbin("-o" + root, *flags, P, Q, os.path.join(d, "zipped")) == (want_out, want_err), flags
        assert sorted(os.listdir(t)) == sorted("run%d.%s.fasta" % (j, b) for j in range(i + 1) for b in "ABU")
        for b in "ABU":
            assert open("%s.%s.fasta" % (root, b), "rb").read() == want_fa[b], (flags, b)
        seen.add(want_out)
    assert len(seen) == 4                                  # the flags change the calls, the batches do not
    for ar, br, sa, sb in (((2, None), None, ":2-", ""), (None, (None, 1), "", ":-1"), ((2, 3), (1, 2), ":2-3", ":1-2")):
        want_out, want_err, want_fa = RO.tabbin(p, q, names, seqs, K, ar, br)
        assert want_out not in seen
        root = os.path.join(t, "range")
        assert tabbin("-o" + root, P + sa, Q + sb, os.path.join(d, "reads.fasta")) == (want_out, want_err), (sa, sb)
        assert all(open("%s.%s.fasta" % (root, b), "rb").read() == want_fa[b] for b in "ABU")
    empty = os.path.join(t, "empty.fasta")                 # no reads: the summary, three empty files
    open(empty, "w").close()
    assert tabbin("-o" + os.path.join(t, "none"), P, Q, empty) == ("", "tabbin: 0 reads, 0 A, 0 B, 0 U, 0 reads with switches\n")
    assert [os.path.getsize(os.path.join(t, "none.%s.fasta" % b)) for b in "ABU"] == [0, 0, 0]


def test_verbose_line(case):
    d, p, q = case["dir"], case["p"], case["q"]
    out, err = tabbin("-v", "-b1000", os.path.join(d, "P"), os.path.join(d, "Q:2-"), os.path.join(d, "reads"))
    want_out, summary, _ = RO.tabbin(p, q, case["names"], case["seqs"], K, None, (2, None))
    lines = err.splitlines(True)
    assert out == want_out and lines[0] == summary and len(lines) == 2
    m = re.fullmatch(r"A (\d+) entries, B (\d+) entries, (\d+) only in A, (\d+) only in B, (\d+) in both, (\d+) bases, "
                     r"(\d+) batches\n", lines[1])
    assert m, err
    oa, ob = RO.only(p, q, None, (2, None))
    both = len(RO.present(p, None) & RO.present(q, (2, None)))
    batches = held = 0                                     # a batch goes out once it holds 1000 bases, the rest at the end
    for s in case["seqs"]:
        held += len(s)
        if held >= 1000:
            batches, held = batches + 1, 0
    batches += held > 0
    assert [int(x) for x in m.groups()] == [len(p), len(q), oa, ob, both, sum(len(s) for s in case["seqs"]), batches]
    assert both > 0 and oa > ob > 0 and 3 < batches < 13


def test_raw_tables_against_their_differences(case, tmp_path):
    """`tabbin P Q` and `tabbin P_sub_Q Q_sub_P` with the operands built by tabop: the same nA and nB, and the same calls
    with and without -u (the differences are the marker sets, so their sizes are the weights in both runs)."""
    d, t = case["dir"], str(tmp_path)
    P, Q, src = os.path.join(d, "P"), os.path.join(d, "Q"), os.path.join(d, "reads")
    for x, y, name in ((P, Q, "P_sub_Q"), (Q, P, "Q_sub_P")):
        r = subprocess.run([os.path.join(BIN, "tabop"), x, "sub", y, os.path.join(t, name)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    for flags in ((), ("-u",), ("-m5",)):
        raw = [line.split("\t") for line in tabbin(*flags, P, Q, src)[0].splitlines()]
        dif = [line.split("\t") for line in tabbin(*flags, os.path.join(t, "P_sub_Q"), os.path.join(t, "Q_sub_P"), src)[0].splitlines()]
        assert len(raw) == len(dif) == 13
        pick = lambda rows: [(r[0], r[1], r[2], r[3], r[5], r[6], r[7], r[8]) for r in rows]       # all but nBoth
        assert pick(raw) == pick(dif)
        assert all(r[4] == "0" for r in dif) and any(r[4] != "0" for r in raw)
        assert {r[7] for r in raw} >= {"A", "B"}

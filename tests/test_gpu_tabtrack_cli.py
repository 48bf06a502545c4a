"""`tabtrack` on a real MI355X (`-m gpu`): stdout, the summary line and the BED file of both modes byte for byte against
tests/runs_oracle.py for a plain FASTA, its .gz and a .db, with operand ranges, -m, batches of a few reads and a sequence
longer than a batch, an empty source and -v; the identity of runs - 1 with tabbin's switches, and of the QV over all
sequences with what cp_kmer_qv gives from tab2prof's tally."""
import gzip
import os
import random
import re
import subprocess

import pytest

import ktab_oracle as KO
import runs_oracle as UO
from conftest import ROOT
from test_gpu_ktab import mixed_reads
from test_gpu_tabprof_cli import write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
K = 21
BIN = os.path.join(ROOT, "classpro_amd")


def tool(name, *args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


def tabtrack(*args):
    return tool("tabtrack", *args)


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    """The two tables and the thirteen reads of tests/test_gpu_tabbin_cli.py (pieces of both read sets, one with an N, one
    of K bases, one shorter than K, an empty one), one more whose five B markers lie between two long runs of A markers, and
    the reads of upper-case A C G T with a base as a .db."""
    import torch
    from classpro_amd import dazz, fastk
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = str(tmp_path_factory.mktemp("tabtrack_cli"))
    rng = random.Random(3)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    ra, rb = mixed_reads(K, 5), mixed_reads(K, 7)
    shared = rnd(600)
    p, q = KO.table(ra + [shared, rnd(2000)], K), KO.table(rb + [shared, shared], K)
    for name, ents, parts in (("P", p, 3), ("Q", q, 1)):
        fastk.write_fastk_ktab(d, name, K, 1, [x for x, _ in ents], [c for _, c in ents], parts)
    seqs = [ra[2][:1200], rb[2][:900], ra[1][:300] + rb[1][:300] + ra[1][300:600] + rb[1][300:350], shared[:200] + ra[0],
            rb[0][:K], rnd(K - 1), b"", ra[2][1000:1400] + b"N" + rb[2][1000:1500], rnd(300), rb[3] + shared[300:],
            ra[4][:100] + rb[4][:100], ra[3], rb[2][2000:],
            ra[2][1500:1800] + rb[2][1500:1525] + ra[2][1800:2100]]
    names = ["read%d/%d" % (i, len(s)) for i, s in enumerate(seqs)]
    write_fasta(os.path.join(d, "reads.fasta"), names, seqs)
    with gzip.open(os.path.join(d, "zipped.fa.gz"), "wb") as f:
        f.write(open(os.path.join(d, "reads.fasta"), "rb").read())
    db_seqs = [s for s in seqs if s and b"N" not in s]
    files = [(len(db_seqs), "reads.fasta", "m1")]
    db_heads = [h[1:] for h in dazz.db_headers(files, dazz.write_db(d, "based", db_seqs, files))]
    return dict(dir=d, p=p, q=q, heads=UO.headers_of(names), seqs=seqs, db_seqs=db_seqs, db_heads=db_heads)


def test_absence_against_the_oracle(case, tmp_path):
    d, t = case["dir"], str(tmp_path)
    p, heads, seqs = case["p"], case["heads"], case["seqs"]
    P = os.path.join(d, "P")
    before = listing(d)
    out, summary, bed = UO.absence(p, heads, seqs, K)
    lines = [x.split("\t") for x in out.splitlines()]
    assert len(lines) == 14 and {"inf", "-"} <= {x[5] for x in lines} and any(re.fullmatch(r"\d+\.\d{4}", x[5]) for x in lines)
    assert bed.count(b"\n") > 10 and " QV inf" not in summary and " QV -" not in summary
    assert tabtrack(P, os.path.join(d, "reads")) == (out, summary)
    assert tabtrack(P + ".ktab", os.path.join(d, "zipped.fa.gz")) == (out, summary)
    assert listing(d) == before                            # without -o no file is written
    seen = {out}
    for i, (flags, sfx, rng) in enumerate(((("-b1000",), "", None), (("-b1",), ":2-", (2, None)), ((), ":-1", (None, 1)),
                                           (("-v", "-b700"), ":3-", (3, None)))):
        want = UO.absence(p, heads, seqs, K, rng)
        root = os.path.join(t, "run%d" % i)
        got_out, got_err = tabtrack("-o" + root, *flags, P + sfx, os.path.join(d, "zipped"))
        assert (got_out, got_err.splitlines(True)[0]) == want[:2], (flags, sfx)
        assert sorted(os.listdir(t)) == ["run%d.missing.bed" % j for j in range(i + 1)]
        assert open(root + ".missing.bed", "rb").read() == want[2], (flags, sfx)
        seen.add(want[0])
    assert len(seen) == 4                                  # the ranges change the track, the batches do not
    m = re.fullmatch(r"A (\d+) entries, (\d+) bases, (\d+) batches, (\d+) runs brought down\n", got_err.splitlines(True)[1])
    assert m and [int(x) for x in m.groups()[:2]] == [len(p), sum(len(s) for s in seqs)] and 3 < int(m.group(3)) < 14
    want = UO.absence(p, case["db_heads"], case["db_seqs"], K)                         # a .db: other headers, no other bytes
    assert tabtrack("-o" + os.path.join(t, "db"), P, os.path.join(d, "based.db")) == want[:2]
    assert open(os.path.join(t, "db.missing.bed"), "rb").read() == want[2] and b"m1/" in want[2]
    empty = os.path.join(t, "empty.fasta")                 # no sequences: the summary, an empty file
    open(empty, "w").close()
    assert tabtrack("-o" + os.path.join(t, "none"), P, empty) == ("", "tabtrack: 0 sequences, 0 k-mers, 0 missing in 0 runs, QV -\n")
    assert os.path.getsize(os.path.join(t, "none.missing.bed")) == 0


def test_phase_blocks_against_the_oracle(case, tmp_path):
    d, t = case["dir"], str(tmp_path)
    p, q, heads, seqs = case["p"], case["q"], case["heads"], case["seqs"]
    P, Q = os.path.join(d, "P"), os.path.join(d, "Q.ktab")
    before = listing(d)
    out, summary, bed = UO.phase(p, q, heads, seqs, K)
    assert " 0 runs" not in summary and " 0 dropped" in summary and not summary.endswith("N50 0\n") and bed.count(b"\n") > 10
    assert tabtrack(P, Q, os.path.join(d, "reads")) == (out, summary)
    assert listing(d) == before                            # without -o no file is written
    runs = [(("-m1", "-b700"), {}), (("-m2",), dict(min_n=2)), (("-m30", "-b1000"), dict(min_n=30)), (("-b1", "-m400"), dict(min_n=400)),
            (("-m2",), dict(min_n=2, a_range=(2, None))), ((), dict(b_range=(None, 1))),
            (("-m3",), dict(min_n=3, a_range=(2, 3), b_range=(1, 2)))]
    seen = set()
    for i, (flags, kw) in enumerate(runs):
        want = UO.phase(p, q, heads, seqs, K, **kw)
        ar, br = kw.get("a_range"), kw.get("b_range")
        sfx = [":%s-%s" % tuple("" if x is None else x for x in r) if r else "" for r in (ar, br)]
        root = os.path.join(t, "run%d" % i)
        assert tabtrack("-o" + root, *flags, P + sfx[0], Q + sfx[1], os.path.join(d, "zipped")) == want[:2], flags
        assert sorted(os.listdir(t)) == sorted("run%d.blocks.bed" % j for j in range(i + 1))
        assert open(root + ".blocks.bed", "rb").read() == want[2], flags
        seen.add(want[:2])
    assert len(seen) == 7                                  # -m and the ranges change the blocks, the batches do not
    runs_m, dropped_m, blocks_m = (int(x) for x in re.search(r"(\d+) runs, (\d+) dropped, (\d+) blocks", UO.phase(p, q, heads, seqs, K, min_n=30)[1]).groups())
    assert dropped_m > 0 and blocks_m < runs_m - dropped_m  # a dropped run between two runs of the other side: they merge
    assert any(" 0 dropped" not in s for _, s in seen)
    want = UO.phase(p, q, case["db_heads"], case["db_seqs"], K, min_n=2)
    assert tabtrack("-m2", "-o" + os.path.join(t, "db"), P, Q, os.path.join(d, "based")) == want[:2]
    assert open(os.path.join(t, "db.blocks.bed"), "rb").read() == want[2]
    empty = os.path.join(t, "empty.fasta")
    open(empty, "w").close()
    assert tabtrack("-o" + os.path.join(t, "none"), P, Q, empty) == (
        "", "tabtrack: 0 sequences, 0 A and 0 B markers, 0 runs, 0 dropped, 0 blocks, block N50 0\n")
    assert os.path.getsize(os.path.join(t, "none.blocks.bed")) == 0
    out_v, err_v = tabtrack("-v", "-b1000", P, Q + ":2-", os.path.join(d, "reads"))
    lines = err_v.splitlines(True)
    assert (out_v, lines[0]) == UO.phase(p, q, heads, seqs, K, b_range=(2, None))[:2] and len(lines) == 2
    m = re.fullmatch(r"A (\d+) entries, B (\d+) entries, (\d+) bases, (\d+) batches, (\d+) runs brought down\n", lines[1])
    batches = held = 0                                     # a batch goes out once it holds 1000 bases, the rest at the end
    for s in seqs:
        held += len(s)
        if held >= 1000:
            batches, held = batches + 1, 0
    batches += held > 0
    assert m and [int(x) for x in m.groups()[:4]] == [len(p), len(q), sum(len(s) for s in seqs), batches]
    assert len(seqs[0]) > 1000 and 3 < batches < 14        # the first sequence is longer than a batch


def test_against_tabbin_and_tab2prof(case, tmp_path):
    d, t = case["dir"], str(tmp_path)
    P, Q, src = os.path.join(d, "P"), os.path.join(d, "Q"), os.path.join(d, "reads")
    for sa, sb in (("", ""), (":2-", ""), (":2-3", ":1-2")):
        track = [x.split("\t") for x in tabtrack("-m1", P + sa, Q + sb, src)[0].splitlines()]
        binned = [x.split("\t") for x in tool("tabbin", P + sa, Q + sb, src)[0].splitlines()]
        assert len(track) == len(binned) == 14
        assert [max(int(x[4]) - 1, 0) for x in track] == [int(x[6]) for x in binned]   # runs - 1 == switches
        assert [x[2:4] for x in track] == [x[2:4] for x in binned] and any(int(x[6]) > 0 for x in binned)
    from classpro_amd.api import kmer_qv
    _, err = tool("tab2prof", "-v", "-N" + os.path.join(t, "rel"), P, src)
    m = re.search(r"(\d+) cells present, (\d+) absent, (\d+) with other bytes\n", err)
    present, absent = int(m.group(1)), int(m.group(2))
    summary = tabtrack(P, src)[1]
    assert absent > 0 and summary.endswith("%d k-mers, %d missing in %d runs, QV %.4f\n" % (
        present + absent, absent, int(summary.split(" missing in ")[1].split(" ")[0]), kmer_qv(K, absent, present + absent)[0]))

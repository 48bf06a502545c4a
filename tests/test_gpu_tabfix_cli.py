"""`tabfix` on a real MI355X (`-m gpu`): the chain `kprof -t1 genome && tabfix -o<root> genome reads.fasta` on a genome of
20 kb and reads with spaced errors of every kind gives the summary line, the .fixed.fasta and the .fixes.tsv of
tests/fix_oracle.py byte for byte; batches of a few reads give the same files; with -d0 only substitutions are fixed; a
count range, -v, no -o and an empty source.  Everything is bytes: the tolerance is zero."""
import os
import re
import subprocess

import pytest

import fix_oracle as FO
from conftest import ROOT
from test_gpu_tabprof_cli import write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
K = 21
BIN = os.path.join(ROOT, "classpro_amd")


def tool(name, *args):
    """stderr of a run that must succeed and print nothing."""
    r = subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", (name, args, r.stderr)
    return r.stderr


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = str(tmp_path_factory.mktemp("tabfix_cli"))
    g, truth, reads, made = FO.read_set(4, K, 2, FO.KINDS1 + FO.KINDS3[3:], nreads=30, rlen=700, glen=20000)
    assert made == set(FO.KINDS1 + FO.KINDS3[3:])
    reads += [reads[3][:K - 1], b"", reads[5][:300] + b"N" + reads[5][300:], truth[7]]
    truth += [reads[-4], b"", reads[-2], truth[7]]
    names = ["read%d/%d" % (i, len(s)) for i, s in enumerate(reads)]
    write_fasta(os.path.join(d, "genome.fasta"), ["chr1"], [g])
    write_fasta(os.path.join(d, "reads.fasta"), names, reads)
    tool("kprof", "-k%d" % K, "-t1", os.path.join(d, "genome.fasta"))
    return dict(dir=d, ents=FO.table([g], K), names=names, reads=reads, truth=truth)


def test_against_the_oracle(case, tmp_path):
    d, t = case["dir"], str(tmp_path)
    G, src = os.path.join(d, "genome"), os.path.join(d, "reads.fasta")
    line, fasta, tsv = FO.tabfix(case["ents"], case["names"], case["reads"], K, 1)
    m = re.match(r"tabfix: 34 sequences, (\d+) gaps, (\d+) fixed \((\d+) substitutions, (\d+) insertions removed, (\d+) deletions filled\)", line)
    assert m and all(int(x) > 20 for x in m.groups()) and tsv.count(b"\n") == int(m.group(2))
    before = listing(d)
    assert tool("tabfix", G, src) == line                  # without -o: the line, no file
    assert listing(d) == before
    root = os.path.join(t, "one")
    assert tool("tabfix", "-o" + root, G + ".ktab", os.path.join(d, "reads")) == line
    assert sorted(os.listdir(t)) == ["one.fixed.fasta", "one.fixes.tsv"]
    assert open(root + ".fixed.fasta", "rb").read() == fasta and open(root + ".fixes.tsv", "rb").read() == tsv
    for i, flags in enumerate((("-b1000",), ("-b1", "-d1"), ("-v", "-b3000"))):      # several batches: the same files
        root = os.path.join(t, "b%d" % i)
        err = tool("tabfix", "-o" + root, *flags, G, src)
        assert err.splitlines(True)[0] == line, flags
        assert open(root + ".fixed.fasta", "rb").read() == fasta and open(root + ".fixes.tsv", "rb").read() == tsv, flags
    v = re.fullmatch(r"(\d+) entries, (\d+) bases in, (\d+) out, (\d+) batches, \d+\.\d{3} s on the device\n", err.splitlines(True)[1])
    out_bases = sum(len(x) for x in fasta.split(b"\n") if not x.startswith(b">"))
    assert v and [int(x) for x in v.groups()[:3]] == [len(case["ents"]), sum(len(s) for s in case["reads"]), out_bases]
    assert 3 < int(v.group(4)) < 34
    # the errors spaced 3K apart that -d1 can undo are undone: those reads are the genome's pieces again
    got = [x for x in fasta.split(b"\n") if not x.startswith(b">")][:-1]
    assert len(got) == 34 and sum(a == b for a, b in zip(got, case["truth"])) >= 10 and got[31] == b""


def test_indel_limits_and_ranges(case, tmp_path):
    d, t = case["dir"], str(tmp_path)
    G, src = os.path.join(d, "genome"), os.path.join(d, "reads.fasta")
    seen = set()
    for i, (flags, sfx, D, rng) in enumerate(((("-d0",), "", 0, None), (("-d2",), "", 2, None), (("-d4", "-b5000"), ":1-1", 4, (1, 1)),
                                              (("-d1",), ":2-", 1, (2, None)))):
        line, fasta, tsv = FO.tabfix(case["ents"], case["names"], case["reads"], K, D, rng)
        root = os.path.join(t, "run%d" % i)
        assert tool("tabfix", "-o" + root, *flags, G + sfx, src) == line, flags
        assert open(root + ".fixed.fasta", "rb").read() == fasta and open(root + ".fixes.tsv", "rb").read() == tsv, flags
        seen.add(line)
        if D == 0:                                         # only substitutions are fixed
            assert re.search(r" (\d+) fixed \(\1 substitutions, 0 insertions removed, 0 deletions filled\)", line) and " 0 fixed" not in line
            assert all(len(x.split(b"\t")[2]) == len(x.split(b"\t")[3]) == 1 for x in tsv.splitlines())
        if D == 2:                                         # every read with spaced errors comes back
            got = [x for x in fasta.split(b"\n") if not x.startswith(b">")][:-1]
            assert got[:30] == case["truth"][:30]
    assert len(seen) == 3                                  # -d4 finds what -d2 finds here; -d0 and the range do not
    empty = os.path.join(t, "empty.fasta")                 # no sequences: the line, two empty files
    open(empty, "w").close()
    assert tool("tabfix", "-o" + os.path.join(t, "none"), G, empty) == (
        "tabfix: 0 sequences, 0 gaps, 0 fixed (0 substitutions, 0 insertions removed, 0 deletions filled), 0 ambiguous, 0 unfixed, "
        "0 open, 0 without candidate, 0 clashes\n")
    assert os.path.getsize(os.path.join(t, "none.fixed.fasta")) == os.path.getsize(os.path.join(t, "none.fixes.tsv")) == 0

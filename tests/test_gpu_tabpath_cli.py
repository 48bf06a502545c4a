"""`tabpath` on a real MI355X (`-m gpu`): a `kprof -t`-style table written with fastk.write_fastk_ktab -- a path, a bubble,
a closed chain, a homopolymer run, a sequence joined to its reverse complement -- and a source as FASTA and as gzipped
FASTQ whose reads run along all of them, one of them three times round the closed chain; whole, with a count range, and
with -b small enough for several batches.  The two stdout lines and the bytes of the .gaf and .gfa files are those of
tests/path_oracle.py; the .gfa without its RC tags is tabgraph's file for the same table; without -o nothing is created;
eight fresh processes in a row print the same two lines."""
import gzip
import os
import random
import re
import subprocess

import pytest

import path_oracle as PO
import unitig_oracle as UO
from conftest import ROOT
from test_gpu_unitigs import mixed_graph
from test_paths_host import random_reads
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "classpro_amd")
K = 21


def tool(name, *args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd import fastk
    rng = random.Random(K)
    seqs = mixed_graph(rng, K)
    seqs += [seqs[0][50:50 + K + 5], seqs[0][300:300 + K]] * 2     # counts of 3 inside the first path
    ents = UO.table(seqs, K)
    d = str(tmp_path_factory.mktemp("tabpath_cli"))
    fastk.write_fastk_ktab(d, "graph", K, 1, [x for x, _ in ents], [c for _, c in ents], 3)
    ring = seqs[3][:70]                                            # the closed chain of mixed_graph, three times round
    reads = [ring * 3 + ring[:K - 1], seqs[1], PO.rcs(seqs[2]), "ACGT", seqs[0][:200] + "N" + seqs[0][201:]]
    reads += random_reads(rng, seqs, 60, 300)
    names = ["read%d/%d" % (i, len(r)) for i, r in enumerate(reads)]
    with open(os.path.join(d, "reads.fasta"), "w") as f:
        for n, r in zip(names, reads):
            f.write(">%s some words\n" % n)
            f.write("".join(r[i:i + 60] + "\n" for i in range(0, len(r), 60)))
    with gzip.open(os.path.join(d, "fq.fastq.gz"), "wt") as f:
        for n, r in zip(names, reads):
            f.write("@%s\twords\n%s\n+\n%s\n" % (n, r, "I" * len(r)))
    return dict(dir=d, ents=ents, reads=reads, names=names)


@pytest.mark.parametrize("src,spec,rng_,batch", [("reads.fasta", "", None, None), ("fq.fastq.gz", "", None, "-b1000"),
                                                  ("reads", ":2-", (2, None), "-b1"), ("fq", ":1000-", (1000, None), None)])
def test_lines_and_files_against_the_oracle(case, tmp_path, src, spec, rng_, batch):
    d, ents, reads, names, t = case["dir"], case["ents"], case["reads"], case["names"], str(tmp_path)
    P = PO.Paths(ents, K, rng_)
    before = listing(d)
    args = ([batch] if batch else []) + ["-g", "-o" + os.path.join(t, "p"), os.path.join(d, "graph") + spec, os.path.join(d, src)]
    out, err = tool("tabpath", *args)
    assert (out, err) == (P.lines(reads), "")
    assert sorted(os.listdir(t)) == ["p.gaf", "p.gfa"] and listing(d) == before
    gaf = open(os.path.join(t, "p.gaf"), "rb").read()
    gfa = open(os.path.join(t, "p.gfa"), "rb").read()
    assert gaf == P.gaf(reads, names) and gfa == P.gfa(reads)
    tool("tabgraph", os.path.join(d, "graph") + spec, os.path.join(t, "g"))
    assert re.sub(rb"\tRC:i:\d+\n", b"\n", gfa) == open(os.path.join(t, "g.gfa"), "rb").read()
    if rng_ is None:
        first = gaf.split(b"\n")[0].split(b"\t")                   # three times round the closed chain: one walk of four or three
        assert first[:5] == [b"read0/%d" % len(reads[0]), b"%d" % len(reads[0]), b"0", b"%d" % len(reads[0]), b"+"]
        assert len(re.findall(rb"[<>]\d+", first[5])) in (3, 4) and len(set(re.findall(rb"[<>]\d+", first[5]))) == 1
        assert gaf.count(b"\n") > len(reads) // 2 and b"RC:i:0\n" in gfa and re.search(rb"\dM\tRC:i:[1-9]", gfa)
    if rng_ == (2, None):
        assert 0 < len(P.utgs) < len(UO.unitigs(ents, K)) and gaf
    if rng_ == (1000, None):
        assert gaf == b"" and gfa == b"H\tVN:Z:1.0\n"
        assert out.endswith("0 on the graph, 0 segments, 0 walks, 0 of 0 unitigs touched, 0 of 0 links crossed\n")
    out2, err = tool("tabpath", "-o" + os.path.join(t, "p"), os.path.join(d, "graph.ktab") + spec, os.path.join(d, src))
    assert (out2, err) == (out, "") and open(os.path.join(t, "p.gaf"), "rb").read() == gaf       # over the file of the first run


def test_nothing_created_without_o_and_verbose(case, tmp_path):
    d, ents, reads = case["dir"], case["ents"], case["reads"]
    P = PO.Paths(ents, K, (1, 2))
    before = listing(d)
    r = subprocess.run([os.path.join(BIN, "tabpath"), "-v", "-b5000", os.path.join(d, "graph") + ":1-2", os.path.join(d, "reads")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert (r.returncode, r.stdout) == (0, P.lines(reads)), r.stderr
    assert os.listdir(str(tmp_path)) == [] and listing(d) == before
    assert re.fullmatch(r"K %d: %d entries, %d bases, \d+ batches, %d segments brought down; \d+\.\d{3} s on the device for the "
                        r"graph, \d+\.\d{3} s for the paths\n" % (K, len(ents), sum(len(x) for x in reads),
                                                                 P.batch(reads)[2]["segments"]), r.stderr), r.stderr


def test_eight_fresh_processes_print_the_oracles_lines(case, tmp_path):
    """A guard against a counter that is zeroed out of order: the first case of
    test_lines_and_files_against_the_oracle eight times, each a process of its own -- the wrong count that was seen ("0 of 11
    unitigs touched") came from the first calls of a fresh process.  A wrong-count check, bounded and not retried: it stops at
    the first run whose lines differ.  It cannot show that such a race is absent, only that it did not happen in these runs."""
    d, ents, reads, t = case["dir"], case["ents"], case["reads"], str(tmp_path)
    want = PO.Paths(ents, K, None).lines(reads)
    assert " 0 of " not in want
    for run in range(8):
        out, err = tool("tabpath", "-g", "-o" + os.path.join(t, "p"), os.path.join(d, "graph"), os.path.join(d, "reads.fasta"))
        assert (out, err) == (want, ""), "run %d of 8" % run

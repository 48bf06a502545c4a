"""`tabphase` on a real MI355X (`-m gpu`): the chain `kprof -t2 reads && tabphase reads reads.fasta out` on the two-haplotype
genome of tests/phase_oracle.py gives the two lines and the sites.tsv of the oracle byte for byte and the two tables entry
for entry; batches of a few reads, a count range and -m change nothing they should not; without <out_root> nothing is
created; `tabtrack out.A out.B` on the two haplotypes gives one block each and no switch.  The tolerance is zero."""
import os
import random
import re
import subprocess

import pytest

import ktab_oracle as KO
import phase_oracle as PO
from conftest import ROOT
from test_gpu_tabprof_cli import write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
K = 21
BIN = os.path.join(ROOT, "classpro_amd")


def tool(name, *args):
    r = subprocess.run([os.path.join(BIN, name)] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (name, args, r.stderr)
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = str(tmp_path_factory.mktemp("tabphase_cli"))
    h1, h2, snps = PO.genome(random.Random(K), K)
    reads = PO.tiled_reads((h1, h2)) + [b"ACGT", b""]
    write_fasta(os.path.join(d, "reads.fasta"), ["read%d" % i for i in range(len(reads))], reads)
    write_fasta(os.path.join(d, "haps.fasta"), ["hap1", "hap2"], [h1, h2])
    tool("kprof", "-k%d" % K, "-t2", os.path.join(d, "reads.fasta"))
    T = [(x, c) for x, c in PO.table(reads, K) if c >= 2]
    return dict(dir=d, T=T, reads=reads, snps=snps)


def table_at(torch, d, root):
    from classpro_amd.api import SortedKmers
    S = SortedKmers.from_ktab(d, root)
    ents = list(zip(((S.hi.cpu().numpy().astype(object) << 63) | S.lo.cpu().numpy().astype(object)).tolist(), S.counts.tolist()))
    S.close()
    return ents


def test_against_the_oracle(case, tmp_path):
    import torch
    d, t, reads = case["dir"], str(tmp_path), case["reads"]
    tab, src = os.path.join(d, "reads"), os.path.join(d, "reads.fasta")
    r = PO.phase(case["T"], K, [reads], None, 2)
    assert r["nsites"] == len(case["snps"]) and r["forest"]["blocks"] == 1
    want = "".join(PO.lines(r, len(reads)))
    before = listing(d)
    assert tool("tabphase", tab, src) == (want, "")        # without <out_root>: the lines, no file
    assert listing(d) == before
    root = os.path.join(t, "one")
    assert tool("tabphase", tab + ".ktab", os.path.join(d, "reads"), root) == (want, "")
    assert sorted(f for f in os.listdir(t) if not f.startswith(".")) == ["one.A.hist", "one.A.ktab", "one.B.hist", "one.B.ktab",
                                                                         "one.sites.tsv"]
    tsv = PO.sites_tsv(r, K)
    assert open(root + ".sites.tsv", "rb").read() == tsv and tsv.count(b"\n") == r["nsites"]
    assert table_at(torch, t, "one.A") == r["A"] and table_at(torch, t, "one.B") == r["B"] and r["A"] and r["B"]
    for i, flags in enumerate((("-b1000",), ("-b20000", "-T1"), ("-v", "-b100000", "-T7"))):      # several batches: the same
        root = os.path.join(t, "b%d" % i)
        out, err = tool("tabphase", *flags, tab, src, root)
        assert out == want, flags
        assert open(root + ".sites.tsv", "rb").read() == tsv, flags
        assert table_at(torch, t, "b%d.A" % i) == r["A"] and table_at(torch, t, "b%d.B" % i) == r["B"], flags
    v = re.fullmatch(r"K 21: (\d+) entries; (\d+) rounds, (\d+) forest edges, 0 bad keys; (\d+) batches, \d+\.\d{3} s on the device\n", err)
    assert v and [int(x) for x in v.groups()[:3]] == [len(case["T"]), r["forest"]["rounds"], r["forest"]["forest"]]
    assert 3 < int(v.group(4)) < len(reads)
    # the two haplotypes as contigs: one block each, no switch, and the two on opposite sides
    out, err = tool("tabtrack", os.path.join(t, "one.A"), os.path.join(t, "one.B"), os.path.join(d, "haps.fasta"))
    rows = [x.split() for x in out.splitlines()]
    assert len(rows) == 2 and all(x[4] == "1" and x[5] == "0" and x[6] == "1" for x in rows)
    assert sorted((int(x[2]) > 0, int(x[3]) > 0) for x in rows) == [(False, True), (True, False)]


def test_range_and_support(case, tmp_path):
    d, t, reads = case["dir"], str(tmp_path), case["reads"]
    tab, src = os.path.join(d, "reads"), os.path.join(d, "reads.fasta")
    seen = set()
    for i, (flags, sfx, rng, m) in enumerate(((("-m1",), "", None, 1), (("-m4",), ":3-", (3, None), 4), (("-m7",), ":2-4", (2, 4), 7))):
        r = PO.phase(case["T"], K, [reads], rng, m)
        want = "".join(PO.lines(r, len(reads)))
        root = os.path.join(t, "run%d" % i)
        assert tool("tabphase", *flags, tab + sfx, src, root) == (want, ""), flags
        assert open(root + ".sites.tsv", "rb").read() == PO.sites_tsv(r, K), flags
        seen.add(want)
    assert len(seen) == 3
    empty = os.path.join(t, "empty.fasta")                 # no sequences: every site is unlinked, two empty tables
    open(empty, "w").close()
    out, err = tool("tabphase", tab, empty, os.path.join(t, "none"))
    n = len(case["snps"])
    assert out == ("tabphase: %d k-mers, %d sites, 0 sequences, 0 markers, 0 links, 0 self\n"
                   "tabphase: 0 edges, 0 kept, 0 tied, 0 weak, 0 conflicts, 0 blocks, largest 0 sites, %d unlinked sites\n" % (2 * n, n, n))
    rows = open(os.path.join(t, "none.sites.tsv")).read().splitlines()
    assert len(rows) == n and all(x.split("\t")[1] == "-1" for x in rows)

"""`tab2prof` on a real MI355X (`-m gpu`): the ground-truth chain `kprof -t1 genome && tab2prof -C genome reads` byte for
byte against `genome2class -p genome reads`, a read set against its own table (kprof's own profile files; with -t2 the
k-mers seen once read 0), tables written elsewhere (three parts with an empty one, a class table of class2ktab), -N and
the -v line.  The expected cells come from tests/tabprof_oracle.py; everything is bytes: the tolerance is zero."""
import os
import re
import subprocess

import numpy as np
import pytest

import kprof_oracle as O
import ktab_oracle as KO
import tabprof_oracle as TO
import truth_oracle as TR
from conftest import ROOT

pytestmark = pytest.mark.gpu
K = 40
BIN = os.path.join(ROOT, "classpro_amd")


def run(tool, *args):
    r = subprocess.run([os.path.join(BIN, tool)] + list(args), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", (tool, args, r.stderr)
    return r.stderr


def write_fasta(path, names, seqs):
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + bytes(s) + b"\n")


def files(d, root):
    """{file name: bytes} of the files of `root` under d: <root>.* and .<root>.*"""
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))
            if f.startswith(root + ".") or f.startswith("." + root + ".")}


def cells_of(d, root):
    """The profile files of `root` under d, decoded: (K, flat uint16 cells of all reads, cells per read)."""
    from classpro_amd import fastk
    k, codes = fastk.read_fastk_codes(d, root)
    prof = [fastk.decode_profile(c) for c in codes]
    return k, TO.flat(prof), [len(p) for p in prof]


@pytest.fixture(scope="module")
def case(built, tmp_path_factory):
    """The diploid case of tests/truth_oracle.py as upper-case FASTA files, the reads' canonical counts and keys."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = TR.make_case(7, K)
    d = str(tmp_path_factory.mktemp("tabprof_cli"))
    genome = [TR.fold(g) for g in c["genome"]]
    write_fasta(os.path.join(d, "genome.fasta"), c["genome_names"], genome)
    write_fasta(os.path.join(d, "reads.fasta"), c["names"], c["seqs"])
    seqs = [bytes(s) for s in c["seqs"]]
    run("kprof", "-k%d" % K, "-t1", os.path.join(d, "genome.fasta"))
    run("kprof", "-k%d" % K, "-t1", "-T4", os.path.join(d, "reads.fasta"))
    return dict(dir=d, names=c["names"], seqs=seqs, cnt=O.count(seqs, K)[0], keys=TO.keys_of(seqs, K))


@pytest.mark.parametrize("threads", [1, 4])
def test_ground_truth_chain(case, tmp_path, threads):
    d = case["dir"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    os.mkdir(a)
    os.mkdir(b)
    run("tab2prof", "-C", "-T%d" % threads, "-N" + os.path.join(a, "truth"), os.path.join(d, "genome"),
        os.path.join(d, "reads.fasta"))
    run("genome2class", "-p", "-k%d" % K, "-T%d" % threads, "-N" + os.path.join(b, "truth"), os.path.join(d, "genome.fasta"),
        os.path.join(d, "reads.fasta"))
    got, want = files(a, "truth"), files(b, "truth")
    assert sorted(want) == sorted(["truth.class", "truth.prof"] + [".truth.%s.%d" % (x, p + 1) for x in ("pidx", "prof")
                                                                     for p in range(threads)])
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    assert got["truth.class"].count(b"H") > 1000 and got["truth.class"].count(b"R") > 1000


def test_own_table(case, tmp_path):
    """A read set against its own table gives kprof's own profile files; with -t2 the k-mers seen once read 0."""
    d, seqs = case["dir"], case["seqs"]
    own = str(tmp_path / "own")
    os.mkdir(own)
    run("tab2prof", "-T4", "-N" + os.path.join(own, "reads"), os.path.join(d, "reads.ktab"), os.path.join(d, "reads"))
    want = {f: x for f, x in files(d, "reads").items() if "ktab" not in f and not f.endswith((".hist", ".fasta"))}
    assert len(want) == 9 and files(own, "reads") == want
    two = str(tmp_path / "two")
    os.mkdir(two)
    write_fasta(os.path.join(two, "reads.fasta"), ["r%d" % i for i in range(len(seqs))], seqs)
    run("kprof", "-k%d" % K, "-t2", os.path.join(two, "reads.fasta"))
    run("tab2prof", os.path.join(two, "reads"), os.path.join(two, "reads"))            # the default root: reads.rel
    k, got, lens = cells_of(two, "reads.rel")
    cells, tally = TO.cells(KO.entries(case["cnt"], 2), seqs, K, keys=case["keys"])
    assert k == K and lens == [len(c) for c in cells] and np.array_equal(got, TO.flat(cells))
    ones = TO.flat(TO.cells(KO.entries(case["cnt"], 1), seqs, K, keys=case["keys"])[0]) == 1
    assert ones.sum() > 1000 and not got[ones].any() and got[~ones].min() == 0 and tally[1] == ones.sum()
    assert sorted(f for f in os.listdir(two) if ".rel." in f) == sorted(
        ["reads.rel.prof"] + [".reads.rel.%s.%d" % (x, p + 1) for x in ("pidx", "prof") for p in range(4)])


def test_other_tables(case, tmp_path):
    from classpro_amd import fastk
    d, seqs = case["dir"], case["seqs"]
    t = str(tmp_path)
    ents = KO.entries(case["cnt"], 30)[:2]                 # two entries in three parts: the first part is empty
    assert len(ents) == 2
    fastk.write_fastk_ktab(t, "few", K, 30, [x for x, _ in ents], [c for _, c in ents], 3)
    err = run("tab2prof", "-v", "-T2", "-b300000", "-N" + os.path.join(t, "sub.few"), os.path.join(t, "few.ktab"),
              os.path.join(d, "reads.fasta"))
    cells, tally = TO.cells(ents, seqs, K, keys=case["keys"])
    assert tally[0] >= 60 and tally[2] == K
    k, got, lens = cells_of(t, "sub.few")
    assert k == K and lens == [len(c) for c in cells] and np.array_equal(got, TO.flat(cells))
    m = re.fullmatch(r"(\d+) table entries, minval (\d+), (\d+) table parts, (\d+) reads, (\d+) bases, (\d+) profile parts, "
                     r"(\d+) cells present, (\d+) absent, (\d+) with other bytes\n", err)
    assert m, err
    assert [int(x) for x in m.groups()] == [2, 30, 3, len(seqs), sum(len(s) for s in seqs), 2] + tally
    # the haploid k-mers of the truth, a class table of class2ktab
    run("genome2class", "-k%d" % K, "-N" + os.path.join(t, "truth"), os.path.join(d, "genome.fasta"), os.path.join(d, "reads.fasta"))
    run("class2ktab", os.path.join(t, "truth.class"), os.path.join(d, "reads"))
    k, minval, _ib, keys, counts = fastk.read_fastk_ktab(t, "truth.H")
    assert (k, minval) == (K, 1) and len(keys) > 1000
    write_fasta(os.path.join(t, "reads.fa"), case["names"], seqs)
    run("tab2prof", "-T3", os.path.join(t, "truth.H"), os.path.join(t, "reads.fa"))     # the default root, beside the source
    cells, tally = TO.cells(list(zip(keys, counts.tolist())), seqs, K, keys=case["keys"])
    k, got, lens = cells_of(t, "reads.rel")
    assert k == K and lens == [len(c) for c in cells] and np.array_equal(got, TO.flat(cells))
    assert tally[0] > 1000 and tally[1] > 1000

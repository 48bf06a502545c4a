"""`tabop` on a real MI355X (`-m gpu`): the hap-mer chain of a trio (`kprof -t2` of mother, father and child, `tabop
mother sub father`, `tabop ... and child`, `tab2prof` of the result over the child's reads), count ranges, -csum, a class
table of class2ktab as an operand, an empty result, the run without an output root and the -v line.  Every file is
compared byte for byte with tests/ktab_oracle.py's files of the entries that tests/setop_oracle.py gives."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ktab_oracle as KO
import setop_oracle as SO
import tabprof_oracle as TO
import truth_oracle as TR
from conftest import ROOT
from test_gpu_tabprof_cli import cells_of, files, run, write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
K = 40
BIN = os.path.join(ROOT, "classpro_amd")


def tabop(*args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, "tabop")] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


def line(tally):
    return "tabop: %d only in A, %d only in B, %d in both, %d out\n" % tally


def hist_bytes(ents):
    low, high, ilow, ihigh, h = SO.hist(ents)
    return struct.pack("<iii", K, low, high) + struct.pack("<qq", ilow, ihigh) + h.astype("<i8").tobytes()


def want_files(root, ents, minval, threads):
    """{file name: bytes} that tabop leaves for a result of these entries."""
    nparts = max(1, min(threads, len(ents)))
    out = {(".%s.ktab.%d" % (root, p) if p else root + ".ktab"): x for p, x in KO.files(clamped(ents), K, minval, nparts).items()}
    out[root + ".hist"] = hist_bytes(ents)
    return out


def clamped(ents):
    return [(x, min(c, KO.MAXC)) for x, c in ents]


def tiled(seq, n=2000, step=500):
    return [seq[s:s + n] for s in range(0, len(seq) - n + 1, step)]


@pytest.fixture(scope="module")
def trio(built, tmp_path_factory):
    """Three read sets at 4x without errors.  The four contigs of tests/truth_oracle.py's diploid case stand for four
    haplotypes: the mother has hapA_1 and hapB_1 (SNPs apart), the father hapA_2 and hapB_2, the child one of each."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = TR.make_case(11, K)
    hap = {n: TR.fold(g)[:10000] for n, g in zip(c["genome_names"], c["genome"])}
    who = {"mother": ("hapA_1", "hapB_1"), "father": ("hapA_2", "hapB_2"), "child": ("hapA_1", "hapB_2")}
    d = str(tmp_path_factory.mktemp("setop_cli"))
    out = dict(dir=d)
    for name, haps in who.items():
        seqs = [bytes(r) for h in haps for r in tiled(hap[h])]
        write_fasta(os.path.join(d, name + ".fasta"), ["%s_%d" % (name, i) for i in range(len(seqs))], seqs)
        run("kprof", "-k%d" % K, "-t2", os.path.join(d, name + ".fasta"))
        out[name] = (seqs, clamped(KO.table(seqs, K, 2)))
        assert len(out[name][1]) > 8000
    write_fasta(os.path.join(d, "genome.fasta"), list(who["child"]), [hap[h] for h in who["child"]])
    return out


@pytest.mark.parametrize("threads", [1, 4])
def test_trio_chain(trio, tmp_path, threads):
    d, t = trio["dir"], str(tmp_path)
    (_, mother), (_, father), (reads, child) = trio["mother"], trio["father"], trio["child"]
    m_only, tally1 = SO.combine(mother, father, "sub")
    mat, tally2 = SO.combine(m_only, child, "and")
    assert 0 < tally1[2] < 3000 and len(m_only) > 8000 and 1000 < len(mat) < len(m_only) - 1000
    out, err = tabop("-T%d" % threads, os.path.join(d, "mother"), "sub", os.path.join(d, "father.ktab"), os.path.join(t, "m_only"))
    assert (out, err) == (line(tally1), "")
    out, err = tabop("-T%d" % threads, os.path.join(t, "m_only"), "and", os.path.join(d, "child"), os.path.join(t, "child.mat"))
    assert (out, err) == (line(tally2), "")
    for root, ents in (("m_only", m_only), ("child.mat", mat)):
        got, want = files(t, root), want_files(root, ents, 2, threads)
        assert sorted(got) == sorted(want), root
        for f in want:
            assert got[f] == want[f], f
    run("tab2prof", os.path.join(t, "child.mat"), os.path.join(d, "child.fasta"))
    cells, tally = TO.cells(mat, reads, K)
    k, got, lens = cells_of(d, "child.rel")
    assert k == K and lens == [len(x) for x in cells] and np.array_equal(got, TO.flat(cells))
    assert tally[0] > 5000 and tally[1] > 5000             # the maternal haplotype is painted, the paternal one is not


def test_ranges_rules_and_other_tables(trio, tmp_path):
    from classpro_amd import fastk
    d, t = trio["dir"], str(tmp_path)
    mother, father, (reads, child) = trio["mother"][1], trio["father"][1], trio["child"]
    # a range on each operand; the rule does not matter for xor
    want, tally = SO.combine(mother, child, "xor", "left", (3, None), (None, 4))
    assert 0 < tally[2] and 0 < tally[0] and 0 < tally[1] and len({c for _, c in mother}) > 3
    out, _ = tabop("-T3", "-cmax", os.path.join(d, "mother:3-"), "xor", os.path.join(d, "child.ktab:-4"), os.path.join(t, "x"))
    assert out == line(tally) and files(t, "x") == want_files("x", want, 2, 3)
    # -csum: the pooled table of mother and child; -cmin over what they share
    for rule, op in (("sum", "or"), ("min", "and")):
        want, tally = SO.combine(mother, child, op, rule)
        assert max(c for _, c in want) > max(c for _, c in mother) or rule == "min"
        out, _ = tabop("-c" + rule, os.path.join(d, "mother"), op, os.path.join(d, "child"), os.path.join(t, rule))
        assert out == line(tally) and files(t, rule) == want_files(rule, want, 2, 4)
    # a class table of class2ktab as an operand: the haploid k-mers of the child's genome that the mother's reads hold
    run("genome2class", "-k%d" % K, "-N" + os.path.join(t, "truth"), os.path.join(d, "genome.fasta"), os.path.join(d, "child.fasta"))
    run("class2ktab", os.path.join(t, "truth.class"), os.path.join(d, "child"))
    k, minval, _ib, keys, counts = fastk.read_fastk_ktab(t, "truth.H")
    hap = list(zip(keys, counts.tolist()))
    assert (k, minval) == (K, 1) and len(hap) > 5000
    want, tally = SO.combine(hap, mother, "and")
    assert 2000 < len(want) < len(hap) - 2000
    out, _ = tabop(os.path.join(t, "truth.H"), "and", os.path.join(d, "mother"), os.path.join(t, "truth.H.mat"))
    assert out == line(tally) and files(t, "truth.H.mat") == want_files("truth.H.mat", want, 1, 4)
    # an empty result still gets its stub, one empty part and a histogram of zeros
    want, tally = SO.combine(mother, mother, "sub")
    assert want == [] and tally == (0, 0, len(mother), 0)
    out, _ = tabop("-T4", os.path.join(d, "mother"), "sub", os.path.join(d, "mother"), os.path.join(t, "none"))
    got = files(t, "none")
    assert out == line(tally) and got == want_files("none", [], 2, 4) and sorted(got) == [".none.ktab.1", "none.hist", "none.ktab"]
    assert len(fastk.read_fastk_ktab(t, "none")[3]) == 0


def test_without_an_output_root_and_verbose(trio, tmp_path):
    d = trio["dir"]
    mother, father = trio["mother"][1], trio["father"][1]
    before = listing(d)
    here = sorted(os.listdir("."))
    for op in ("and", "or", "sub", "xor"):
        tally = SO.combine(mother, father, op, "left", None, (3, None))[1]
        assert tabop(os.path.join(d, "mother"), op, os.path.join(d, "father:3-")) == (line(tally), "")
    assert listing(d) == before and sorted(os.listdir(".")) == here
    out, err = tabop("-v", os.path.join(d, "mother"), "and", os.path.join(d, "father"))
    tally = SO.combine(mother, father, "and")[1]
    assert out == line(tally)
    m = re.fullmatch(r"K (\d+): A (\d+) entries, minval (\d+), (\d+) parts; B (\d+) entries, minval (\d+), (\d+) parts; "
                     r"result (\d+) entries, minval (\d+), (\d+) parts\n", err)
    assert m, err
    assert [int(x) for x in m.groups()] == [K, len(mother), 2, 4, len(father), 2, 4, tally[3], 2, 0]
    out, err = tabop("-v", "-T2", os.path.join(d, "mother"), "or", os.path.join(d, "father"), str(tmp_path / "u"))
    assert [int(x) for x in re.findall(r"\d+", err)][-3:] == [len(mother) + len(father) - tally[2], 2, 2]
    assert listing(d) == before

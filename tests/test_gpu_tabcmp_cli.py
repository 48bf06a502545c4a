"""`tabcmp` on a real MI355X (`-m gpu`): the evaluation of an assembly against its reads (`kprof -t1` of both, `tabcmp -q
asm reads`), with and without an output root, with count ranges, -wa, -wb, -x and -y, the -v line, and the reads against
themselves.  The stdout lines and the bytes of the .cmp file are those of tests/cmphist_oracle.py over the entries of
tests/ktab_oracle.py; QV and completeness are parsed and compared with the oracle's."""
import math
import os
import re
import subprocess

import pytest

import cmphist_oracle as CO
import ktab_oracle as KO
import truth_oracle as TR
from conftest import ROOT
from test_gpu_tabprof_cli import run, write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
K = 40
BIN = os.path.join(ROOT, "classpro_amd")
QV_LINE = re.compile(r"^tabcmp: QV (\S+) error (\S+) completeness (\S+) %$")


def tabcmp(*args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, "tabcmp")] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


def line(keys):
    return "tabcmp: %d only in A, %d only in B, %d in both\n" % CO.tally(keys)


def clamped(ents):
    return [(x, min(c, KO.MAXC)) for x, c in ents]


def tiled(seq, n=2000, step=500):
    return [seq[s:s + n] for s in range(0, len(seq) - n + 1, step)]


@pytest.fixture(scope="module")
def pair(built, tmp_path_factory):
    """Reads at 4x without errors over two haplotypes of tests/truth_oracle.py's diploid case, and an assembly of them:
    the first haplotype with three wrong bases, and only four fifths of the second."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = TR.make_case(11, K)
    hap = {n: bytes(TR.fold(g)[:10000]) for n, g in zip(c["genome_names"], c["genome"])}
    h1, h2 = hap["hapA_1"], hap["hapB_2"]
    bad = bytearray(h1)
    for p in (1500, 5000, 5007):
        bad[p] = b"ACGT"[(b"ACGT".index(bad[p]) + 1) % 4]
    d = str(tmp_path_factory.mktemp("tabcmp_cli"))
    sets = dict(asm=[bytes(bad), h2[:8000]], reads=tiled(h1) + tiled(h2))
    out = dict(dir=d)
    for name, seqs in sets.items():
        write_fasta(os.path.join(d, name + ".fasta"), ["%s_%d" % (name, i) for i in range(len(seqs))], seqs)
        run("kprof", "-k%d" % K, "-t1", os.path.join(d, name + ".fasta"))
        out[name] = clamped(KO.table(seqs, K, 1))
    assert len(out["asm"]) > 15000 and len(out["reads"]) > 15000
    return out


def check_qv(text, asm, reads, a_range=None, b_range=None, xmax=8, ymax=1000):
    """The second line of -q against the oracle: the fields carry four decimals, so 1e-4 absolute."""
    m = QV_LINE.match(text)
    assert m, text
    wa = CO.matrix(asm, reads, xmax, ymax, "a", a_range, b_range)
    keys = CO.matrix(asm, reads, xmax, ymax, "keys", a_range, b_range)
    qv, err = CO.qv(K, int(wa[:, 0].sum()), int(wa.sum()))
    comp = CO.completeness(keys)
    got_qv, got_err, got_comp = (float(x) for x in m.groups())
    assert (got_qv == qv) if math.isinf(qv) else abs(got_qv - qv) <= 1e-4
    assert abs(got_err - err) <= 0.5e-3 * err + 1e-300     # %.3e: four significant digits
    assert abs(got_comp - comp) <= 1e-4
    return got_qv, got_comp


def test_assembly_against_reads(pair, tmp_path):
    d, t, asm, reads = pair["dir"], str(tmp_path), pair["asm"], pair["reads"]
    keys = CO.matrix(asm, reads, 8, 1000)
    only_a, only_b, both = CO.tally(keys)
    assert 80 < only_a <= 3 * K and only_b > 1000 and both > 15000       # three wrong bases, a fifth of a haplotype missing
    before = listing(d)
    out, err = tabcmp(os.path.join(d, "asm"), os.path.join(d, "reads.ktab"))
    assert (out, err) == (line(keys), "") and listing(d) == before and os.listdir(t) == []
    out, err = tabcmp("-q", os.path.join(d, "asm"), os.path.join(d, "reads"), os.path.join(t, "eval"))
    first, second = out.splitlines(keepends=True)
    assert first == line(keys) and err == ""
    qv, comp = check_qv(second.rstrip("\n"), asm, reads)
    assert 30 < qv < 45 and 85 < comp < 99
    assert os.listdir(t) == ["eval.cmp"] and open(os.path.join(t, "eval.cmp"), "rb").read() == CO.cmp_text(keys, "keys")
    assert listing(d) == before


def test_weights_bounds_ranges_and_verbose(pair, tmp_path):
    d, t, asm, reads = pair["dir"], str(tmp_path), pair["asm"], pair["reads"]
    a, b = os.path.join(d, "asm"), os.path.join(d, "reads")
    for flag, w in (("-wa", "a"), ("-wb", "b"), ("-wkeys", "keys")):
        out, err = tabcmp(flag, "-x2", "-y3", a, b, os.path.join(t, w))
        assert (out, err) == (line(CO.matrix(asm, reads, 2, 3)), "")
        assert open(os.path.join(t, w + ".cmp"), "rb").read() == CO.cmp_text(CO.matrix(asm, reads, 2, 3, w), w)
    # solid read k-mers only, and the assembly's single-copy k-mers
    assert len({c for _, c in reads}) > 3
    keys = CO.matrix(asm, reads, 8, 1000, "keys", (1, 1), (3, None))
    assert all(CO.tally(keys))
    out, err = tabcmp("-q", "-wa", a + ":1-1", b + ".ktab:3-", os.path.join(t, "solid"))
    first, second = out.splitlines(keepends=True)
    assert first == line(keys) and err == ""
    check_qv(second.rstrip("\n"), asm, reads, (1, 1), (3, None))
    assert open(os.path.join(t, "solid.cmp"), "rb").read() == CO.cmp_text(CO.matrix(asm, reads, 8, 1000, "a", (1, 1), (3, None)), "a")
    # -v
    wb = CO.matrix(asm, reads, 4, 2, "b")
    out, err = tabcmp("-v", "-wb", "-x4", "-y2", a, b)
    assert out == line(CO.matrix(asm, reads, 4, 2))
    assert err == "K %d: A %d entries; B %d entries; xmax 4, ymax 2; %d non-zero cells\n" % (K, len(asm), len(reads), int((wb != 0).sum()))
    # a range that empties B: completeness has no denominator
    out, _ = tabcmp("-q", a, b + ":30000-")
    first, second = out.splitlines()
    assert first + "\n" == line(CO.matrix(asm, [], 8, 1000)) and QV_LINE.match(second).group(3) == "nan"


def test_reads_against_themselves(pair, tmp_path):
    d, reads = pair["dir"], pair["reads"]
    out, err = tabcmp("-q", os.path.join(d, "reads"), os.path.join(d, "reads"), os.path.join(str(tmp_path), "self"))
    first, second = out.splitlines()
    keys = CO.matrix(reads, reads, 8, 1000)
    assert first + "\n" == line(keys) and CO.tally(keys) == (0, 0, len(reads)) and err == ""
    assert second == "tabcmp: QV inf error 0.000e+00 completeness 100.0000 %"
    assert open(os.path.join(str(tmp_path), "self.cmp"), "rb").read() == CO.cmp_text(keys, "keys")

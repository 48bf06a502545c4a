"""`tabhet` on a real MI355X (`-m gpu`): reads at 4x over two haplotypes that differ by planted SNPs, `kprof -t1` of them,
then `tabhet` with and without an output root, with -a, -t and a count range, and `tab2prof` of the paired k-mers over the
reads.  The stdout line, the bytes of the .het file and the files of -t are those of tests/hetpairs_oracle.py over the
entries of tests/ktab_oracle.py."""
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import hetpairs_oracle as HO
import ktab_oracle as KO
import setop_oracle as SO
import tabprof_oracle as TO
from conftest import ROOT
from test_gpu_tabprof_cli import cells_of, files, run, write_fasta
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "classpro_amd")


def tabhet(*args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, "tabhet")] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


def want_files(root, ents, K, minval, threads):
    """{file name: bytes} that tabhet -t leaves for a result of these entries, without the .het."""
    nparts = max(1, min(threads, len(ents)))
    out = {(".%s.ktab.%d" % (root, p) if p else root + ".ktab"): x for p, x in KO.files(ents, K, minval, nparts).items()}
    low, high, ilow, ihigh, h = SO.hist(ents)
    out[root + ".hist"] = struct.pack("<iii", K, low, high) + struct.pack("<qq", ilow, ihigh) + h.astype("<i8").tobytes()
    return out


@pytest.fixture(scope="module", params=[21, 40])
def diploid(request, built, tmp_path_factory):
    """Two haplotypes of 6000 bases with a SNP every 150 and two SNPs 7 apart, reads of 2000 every 500 over both."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    K = request.param
    rng = random.Random(K)
    h1 = bytearray(rng.choice(b"ACGT") for _ in range(6000))
    h2 = bytearray(h1)
    for p in list(range(100, 5900, 150)) + [3007]:
        h2[p] = b"ACGT"[(b"ACGT".index(h2[p]) + rng.randint(1, 3)) % 4]
    seqs = [bytes(h[s:s + 2000]) for h in (h1, h2) for s in range(0, 4001, 500)]
    d = str(tmp_path_factory.mktemp("tabhet_cli_%d" % K))
    write_fasta(os.path.join(d, "reads.fasta"), ["r%d" % i for i in range(len(seqs))], seqs)
    run("kprof", "-k%d" % K, "-t1", os.path.join(d, "reads.fasta"))
    ents = KO.table(seqs, K, 1)
    assert max(c for _, c in ents) < KO.MAXC
    return dict(K=K, dir=d, seqs=seqs, ents=ents)


def test_pairs_of_a_diploid_read_set(diploid, tmp_path):
    K, d, ents, t = diploid["K"], diploid["dir"], diploid["ents"], str(tmp_path)
    tal = HO.tally(ents, K)
    assert tal["unique"] >= 30 and tal["pairs"] >= tal["unique"]
    before = listing(d)
    out, err = tabhet(os.path.join(d, "reads"))
    assert (out, err) == (HO.line(tal), "") and listing(d) == before and os.listdir(t) == []
    out, err = tabhet(os.path.join(d, "reads.ktab"), os.path.join(t, "smudge"))
    assert (out, err) == (HO.line(tal), "")
    mat = HO.matrix(ents, K, 1000, 1000)
    assert mat.sum() == tal["unique"] and mat[1:5, 1:5].sum() > 20                  # both haplotypes at 4x or less
    assert os.listdir(t) == ["smudge.het"] and open(os.path.join(t, "smudge.het"), "rb").read() == HO.het_text(mat)
    assert listing(d) == before


@pytest.mark.parametrize("threads", [1, 4])
def test_table_of_the_paired_kmers(diploid, tmp_path, threads):
    K, d, ents, seqs, t = diploid["K"], diploid["dir"], diploid["ents"], diploid["seqs"], str(tmp_path)
    mem = HO.members(ents, K)
    out, err = tabhet("-t", "-T%d" % threads, os.path.join(d, "reads"), os.path.join(t, "het"))
    assert (out, err) == (HO.line(HO.tally(ents, K)), "")
    got, want = files(t, "het"), want_files("het", mem, K, 1, threads)
    want["het.het"] = HO.het_text(HO.matrix(ents, K, 1000, 1000))
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    if threads == 1:                                       # the markers go straight into tab2prof
        run("tab2prof", "-N" + os.path.join(t, "marks"), os.path.join(t, "het"), os.path.join(d, "reads.fasta"))
        cells, tally = TO.cells(mem, seqs, K)
        k, prof, lens = cells_of(t, "marks")
        assert k == K and lens == [len(x) for x in cells] and np.array_equal(prof, TO.flat(cells))
        assert tally[0] > 100 and tally[1] > 10000


def test_all_pairs_ranges_bounds_and_verbose(diploid, tmp_path):
    K, d, ents, t = diploid["K"], diploid["dir"], diploid["ents"], str(tmp_path)
    out, err = tabhet("-a", "-x3", "-y5", os.path.join(d, "reads"), os.path.join(t, "all"))
    assert (out, err) == (HO.line(HO.tally(ents, K, None, False)), "")
    assert open(os.path.join(t, "all.het"), "rb").read() == HO.het_text(HO.matrix(ents, K, 3, 5, None, False))
    for spec, rng_ in ((":2-", (2, None)), (":-3", (None, 3)), (":3-4", (3, 4))):
        tal = HO.tally(ents, K, rng_, False)
        mem = HO.members(ents, K, rng_, False)
        out, err = tabhet("-v", "-a", "-t", "-T2", os.path.join(d, "reads") + spec, os.path.join(t, "r"))
        assert out == HO.line(tal)
        assert re.fullmatch(r"K %d: %d entries; %d paired k-mers, %d out; xmax 1000, ymax 1000; \d+\.\d{3} s on the device\n"
                            % (K, len(ents), tal["paired"], len(mem)), err), err
        got, want = files(t, "r"), want_files("r", mem, K, 1, 2)
        want["r.het"] = HO.het_text(HO.matrix(ents, K, 1000, 1000, rng_, False))
        assert got == want
    assert HO.tally(ents, K, (3, 4), False) != HO.tally(ents, K, (2, None), False)

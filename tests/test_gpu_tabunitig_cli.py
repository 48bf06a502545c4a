"""`tabunitig` on a real MI355X (`-m gpu`): tables written with fastk.write_fastk_ktab -- a bubble, paths, a closed chain, a
homopolymer run -- with and without a count range and with and without an output root, and `kprof -t1` of a small FASTA
followed by `tabunitig`.  The stdout line and the bytes of the .unitigs.fa file are those of tests/unitig_oracle.py."""
import os
import random
import re
import subprocess

import pytest

import ktab_oracle as KO
import unitig_oracle as UO
from conftest import ROOT
from test_gpu_tabprof_cli import run, write_fasta
from test_gpu_unitigs import circle, mixed_graph
from test_tabprof_host import listing
from test_unitig_host import rnd

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "classpro_amd")


def tabunitig(*args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, "tabunitig")] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


@pytest.fixture(scope="module", params=[21, 40])
def graph(request, built, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd import fastk
    K = request.param
    rng = random.Random(K)
    seqs = mixed_graph(rng, K)
    seqs += [seqs[0][50:50 + K + 5], seqs[0][300:300 + K]] * 2     # counts of 3 inside the first path
    ents = UO.table(seqs, K)
    d = str(tmp_path_factory.mktemp("tabunitig_cli_%d" % K))
    fastk.write_fastk_ktab(d, "graph", K, 1, [x for x, _ in ents], [c for _, c in ents], 3)
    return dict(K=K, dir=d, ents=ents)


@pytest.mark.parametrize("spec,rng_", [("", None), (":1-1", (1, 1)), (":2-", (2, None)), (":-2", (None, 2)), (":1000-", (1000, None))])
def test_line_and_file_against_the_oracle(graph, tmp_path, spec, rng_):
    K, d, ents, t = graph["K"], graph["dir"], graph["ents"], str(tmp_path)
    utgs = UO.unitigs(ents, K, rng_)
    want = UO.line(ents, K, rng_, utgs)
    before = listing(d)
    out, err = tabunitig(os.path.join(d, "graph") + spec)
    assert (out, err) == (want, "") and listing(d) == before and os.listdir(t) == []
    out, err = tabunitig(os.path.join(d, "graph.ktab") + spec, os.path.join(t, "g"))
    assert (out, err) == (want, "")
    assert os.listdir(t) == ["g.unitigs.fa"] and listing(d) == before
    text = open(os.path.join(t, "g.unitigs.fa"), "rb").read()
    assert text == UO.fasta(utgs)
    if rng_ is None:
        assert text.count(b" CL:Z:circular\n") == 2 and len(utgs) > 8       # the closed chains are in the file
    if rng_ == (1000, None):
        assert text == b"" and want.startswith("tabunitig: 0 k-mers, 0 unitigs, 0 bases, 0 circular, longest 0, N50 0")


def test_verbose(graph, tmp_path):
    K, d, ents = graph["K"], graph["dir"], graph["ents"]
    t = UO.tally(ents, K, (1, 2))
    out, err = tabunitig("-v", os.path.join(d, "graph") + ":1-2", os.path.join(str(tmp_path), "v"))
    assert out == UO.line(ents, K, (1, 2))
    assert re.fullmatch(r"K %d: %d entries; %d tips, %d branching, %d isolated; \d+ jump rounds; \d+\.\d{3} s on the device\n"
                        % (K, len(ents), t["tips"], t["branching"], t["isolated"]), err), err


def test_kprof_then_tabunitig(built, tmp_path):
    """Reads over a closed sequence and over two haplotypes: `kprof -t1`, then the unitigs of its table."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    K = 21
    d = str(tmp_path)
    rng = random.Random(1)
    h1 = rnd(rng, 3000)
    h2 = h1[:1500] + "ACGT"[("ACGT".index(h1[1500]) + 1) % 4] + h1[1501:]
    ring = circle(rnd(rng, 500), K)
    seqs = [h[s:s + 1000] for h in (h1, h2) for s in range(0, 2001, 500)] + [ring, ring[100:400]]
    write_fasta(os.path.join(d, "reads.fasta"), ["r%d" % i for i in range(len(seqs))], [s.encode() for s in seqs])
    run("kprof", "-k%d" % K, "-t1", os.path.join(d, "reads.fasta"))
    ents = KO.table([s.encode() for s in seqs], K, 1)
    assert ents == UO.table(seqs, K)
    utgs = UO.unitigs(ents, K)
    assert sum(u[2] for u in utgs) == 1 and len(utgs) == 5
    out, err = tabunitig(os.path.join(d, "reads"), os.path.join(d, "asm"))
    assert (out, err) == (UO.line(ents, K, None, utgs), "")
    assert open(os.path.join(d, "asm.unitigs.fa"), "rb").read() == UO.fasta(utgs)

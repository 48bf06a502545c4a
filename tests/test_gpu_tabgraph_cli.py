"""`tabgraph` on a real MI355X (`-m gpu`): a `kprof -t`-style table written with fastk.write_fastk_ktab -- a path, a bubble,
a closed chain, a homopolymer run, a sequence joined to its reverse complement -- whole, with a count range and with a
range that leaves nothing.  The two stdout lines and the bytes of the .gfa file are those of
tests/unitig_graph_oracle.py; no other file is created."""
import os
import random
import re
import subprocess

import pytest

import unitig_graph_oracle as GO
import unitig_oracle as UO
from conftest import ROOT
from test_gpu_unitigs import mixed_graph
from test_tabprof_host import listing

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "classpro_amd")
K = 21


def tabgraph(*args):
    """(stdout, stderr) of a run that must succeed."""
    r = subprocess.run([os.path.join(BIN, "tabgraph")] + list(args), capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout, r.stderr


@pytest.fixture(scope="module")
def graph(built, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd import fastk
    rng = random.Random(K)
    seqs = mixed_graph(rng, K)
    seqs += [seqs[0][50:50 + K + 5], seqs[0][300:300 + K]] * 2     # counts of 3 inside the first path
    ents = UO.table(seqs, K)
    d = str(tmp_path_factory.mktemp("tabgraph_cli"))
    fastk.write_fastk_ktab(d, "graph", K, 1, [x for x, _ in ents], [c for _, c in ents], 3)
    return dict(dir=d, ents=ents)


@pytest.mark.parametrize("spec,rng_", [("", None), (":2-", (2, None)), (":1000-", (1000, None))])
def test_lines_and_file_against_the_oracle(graph, tmp_path, spec, rng_):
    d, ents, t = graph["dir"], graph["ents"], str(tmp_path)
    L = GO.Links(ents, K, rng_)
    before = listing(d)
    out, err = tabgraph(os.path.join(d, "graph") + spec, os.path.join(t, "g"))
    assert (out, err) == (L.line(), "")
    assert os.listdir(t) == ["g.gfa"] and listing(d) == before
    text = open(os.path.join(t, "g.gfa"), "rb").read()
    assert text == L.gfa()
    if rng_ is None:
        assert text.count(b"\nL\t") == len(L.arcs) > 8 and L.tally()["self"] >= 4 and L.tally()["components"] >= 6
    if rng_ == (2, None):
        assert 0 < L.n < len(UO.unitigs(ents, K))
    if rng_ == (1000, None):
        assert text == b"H\tVN:Z:1.0\n"
        assert out == ("tabgraph: 0 k-mers, 0 unitigs, 0 bases, 0 circular, longest 0, N50 0\n"
                       "tabgraph: 0 links, 0 dead ends, 0 tip unitigs, 0 components, largest 0 bases\n")
    out2, err = tabgraph(os.path.join(d, "graph.ktab") + spec, os.path.join(t, "g"))       # over the file of the first run
    assert (out2, err) == (out, "") and open(os.path.join(t, "g.gfa"), "rb").read() == text


def test_verbose(graph, tmp_path):
    d, ents = graph["dir"], graph["ents"]
    t = UO.tally(ents, K, (1, 2))
    L = GO.Links(ents, K, (1, 2))
    out, err = tabgraph("-v", os.path.join(d, "graph") + ":1-2", os.path.join(str(tmp_path), "v"))
    assert out == L.line() and open(os.path.join(str(tmp_path), "v.gfa"), "rb").read() == L.gfa()
    assert re.fullmatch(r"K %d: %d entries; %d tips, %d branching, %d isolated; \d+ jump rounds; \d+\.\d{3} s on the device; "
                        r"\d+ label rounds; \d+\.\d{3} s links, \d+\.\d{3} s components\n"
                        % (K, len(ents), t["tips"], t["branching"], t["isolated"]), err), err
    assert os.listdir(str(tmp_path)) == ["v.gfa"]

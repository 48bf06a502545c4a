"""`tabclean` on a real MI355X (`-m gpu`): tables written with fastk.write_fastk_ktab -- reads with errors over a genome, and
a graph with an island, a tip and a bubble -- with and without a count range, every limit, one round and the defaults, with
and without an output root, and the result fed to `tabunitig`.  The stdout text is that of the loop of
tests/prune_oracle.py, the files are read back with fastk.read_fastk_ktab."""
import os
import re
import subprocess

import pytest

import prune_cases as PC
import prune_oracle as PR
import unitig_oracle as UO
from conftest import ROOT
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
def tables(built, tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd import fastk
    d = str(tmp_path_factory.mktemp("tabclean_cli"))
    _, seqs = PC.read_set(2, K, False)
    reads = UO.table(seqs, K)
    seqs, k9, _ = PC.limit_case()
    small = UO.table(seqs, k9)
    fastk.write_fastk_ktab(d, "reads", K, 2, [x for x, _ in reads], [c for _, c in reads], 3)
    fastk.write_fastk_ktab(d, "small", k9, 1, [x for x, _ in small], [c for _, c in small], 1)
    return dict(dir=d, reads=reads, small=small, k9=k9)


def check_files(t, root, k, minval, ents, parts):
    from classpro_amd import fastk
    assert sorted(os.listdir(t)) == sorted([".%s.ktab.%d" % (root, p + 1) for p in range(parts)] + [root + ".hist", root + ".ktab"])
    kk, mc, _, keys, counts = fastk.read_fastk_ktab(t, root)
    assert (kk, mc, keys, counts.tolist()) == (k, minval, [x for x, _ in ents], [c for _, c in ents])
    hk, low, high, _, _, h = fastk.read_fastk_hist(os.path.join(t, root + ".hist"))
    assert (hk, low, high) == (k, 1, 32767) and int(h.sum()) == len(ents)


@pytest.mark.parametrize("flags,spec,rng_,limits,rounds", [
    (["-t42", "-b41"], "", None, (0, 42, 41), 10), (["-b41", "-i30"], ":2-", (2, None), (30, 42, 41), 10),
    (["-t0", "-b41"], ":-20", (None, 20), (0, 0, 41), 10), (["-r1", "-b41"], "", None, (0, 42, 41), 1),
    (["-r2", "-t30", "-T2"], ":2-", (2, None), (0, 30, 0), 2), ([], "", None, (0, 42, 0), 10),
    (["-b41"], ":1000-", (1000, None), (0, 42, 41), 10)])
def test_text_and_files_against_the_oracle(tables, tmp_path, flags, spec, rng_, limits, rounds):
    d, ents, t = tables["dir"], tables["reads"], str(tmp_path)
    want, out_ents = PR.text(ents, K, rng_, limits, rounds)
    before = listing(d)
    out, err = tool("tabclean", *flags, os.path.join(d, "reads") + spec)              # a bare run creates nothing
    assert (out, err) == (want, "") and listing(d) == before and os.listdir(t) == []
    out, err = tool("tabclean", *flags, os.path.join(d, "reads.ktab") + spec, os.path.join(t, "clean"))
    assert (out, err) == (want, "") and listing(d) == before
    check_files(t, "clean", K, 2, out_ents, max(1, min(2 if "-T2" in flags else 4, len(out_ents))))
    if rounds == 1:
        assert want.count(": round ") == 1 and want.endswith(" 1 rounds\n")
    if rng_ == (1000, None):
        assert want.endswith("tabclean: 0 k-mers in, 0 out, 1 rounds\n")
    else:
        assert len(out_ents) < len(ents)


def test_every_rule_and_the_result_fed_to_tabunitig(tables, tmp_path):
    d, ents, k9, t = tables["dir"], tables["small"], tables["k9"], str(tmp_path)
    lim = 2 * k9
    want, out_ents = PR.text(ents, k9, None, (lim, lim, lim))
    assert "round 1: 7 unitigs, 1 islands, 1 tips, 1 bubbles" in want and "round 2: 1 unitigs, 0 islands, 0 tips, 0 bubbles, 0 k-mers" in want
    out, err = tool("tabclean", "-v", "-i%d" % lim, "-t%d" % lim, "-b%d" % lim, os.path.join(d, "small"), os.path.join(t, "one"))
    assert out == want
    assert re.fullmatch(r"(round \d+: \d+ entries; \d+\.\d{3} s wall\n){2}K %d: %d entries, minval 1, 1 parts; "
                        r"result %d entries, 4 parts\n" % (k9, len(ents), len(out_ents)), err), err
    check_files(t, "one", k9, 1, out_ents, 4)
    out, err = tool("tabunitig", os.path.join(t, "one"))
    assert (out, err) == (UO.line(out_ents, k9), "") and out.startswith("tabunitig: %d k-mers, 1 unitigs" % len(out_ents))
    out, err = tool("tabclean", os.path.join(t, "one"))                               # clean already: one round, the defaults
    assert out == PR.text(out_ents, k9, None, (0, lim, 0))[0] and out.endswith("%d out, 1 rounds\n" % len(out_ents))

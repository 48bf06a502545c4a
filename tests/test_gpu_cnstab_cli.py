"""`class2ktab` on a real MI355X (`-m gpu`): on the evaluation scenario with its oracle-written est.class, the four
tables and histograms byte for byte against fastk.write_fastk_ktab of the oracle's per-class entries and the oracle's
histograms, -T, -t, -a and -N, a .class.gz input, an emptied class, the H table through the reference's own readers,
and the -v text.  A table of K = 40 has a 128-MiB index, so directories are compared by size and SHA-256 and removed
when a test is done."""
import gzip
import hashlib
import os
import shutil
import subprocess

import pytest

import cns_oracle as C
import cnstab_oracle as CT
import eval_case
import kprof_oracle as O
import ktab_oracle as KO
from conftest import ROOT
from test_ktab_host import check_through_reference

pytestmark = pytest.mark.gpu
K = eval_case.K
TOOL = os.path.join(ROOT, "classpro_amd", "class2ktab")


@pytest.fixture(scope="module")
def scenario(built, tmp_path_factory):
    """(directory with est.class and the reads' profiles, the oracle's canonical label table)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    d = str(tmp_path_factory.mktemp("cnstab_cli"))
    eval_case.build_case(d, eval_case.oracle_labels, True)
    t, skipped = C.table(C.read_class(os.path.join(d, "est.class")), K, True)
    assert skipped == 0 and all(CT.select(t, l) for l in CT.LABELS)
    return d, t


def digest(d):
    out = {}
    for f in sorted(os.listdir(d)):
        p = os.path.join(d, f)
        if os.path.isfile(p):
            h = hashlib.sha256()
            with open(p, "rb") as fh:
                for blk in iter(lambda: fh.read(1 << 24), b""):
                    h.update(blk)
            out[f] = (os.path.getsize(p), h.hexdigest())
    return out


def expect(tmp, root, t, minval, pct, threads):
    """The digest of what fastk.write_fastk_ktab and the oracle's histograms give for the four classes."""
    from classpro_amd import fastk
    d = os.path.join(str(tmp), "want")
    h, il, ih = CT.class_hist(t)
    for i, l in enumerate(CT.LABELS):
        ents = CT.select(t, l, minval, pct)
        fastk.write_fastk_ktab(d, "%s.%s" % (root, l), K, minval, [x for x, _ in ents], [c for _, c in ents],
                               max(1, min(threads, len(ents))))
        with open(os.path.join(d, "%s.%s.hist" % (root, l)), "wb") as f:
            f.write(CT.hist_bytes(K, h[i], il[i], ih[i]))
    out = digest(d)
    shutil.rmtree(d)
    return out


def run(*args):
    r = subprocess.run([TOOL] + list(args), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    return r


@pytest.fixture(scope="module")
def run4(scenario, tmp_path_factory):
    """`class2ktab -v -T4` beside a copy of est.class: (directory, the run)."""
    d, _ = scenario
    out = str(tmp_path_factory.mktemp("cnstab_run4"))
    shutil.copy(os.path.join(d, "est.class"), out)
    r = run("-v", "-T4", os.path.join(out, "est.class"), os.path.join(d, "reads"))
    yield out, r
    shutil.rmtree(out)


def test_files_and_the_verbose_text(scenario, run4, tmp_path):
    _, t = scenario
    out, r = run4
    got = digest(out)
    del got["est.class"]
    want = expect(tmp_path, "est", t, 1, 0, 4)
    assert len(want) == 4 * (2 + 4) and got == want
    lines = r.stderr.splitlines()
    assert len(lines) == 5 and all(x.startswith("class2ktab: ") for x in lines)
    st = C.stats(t, 0)
    assert ("K = %d canonical: %d k-mer positions, %d distinct k-mers, %d unanimous, 0 skipped"
            % (K, st["n_kmers"], st["n_distinct"], st["n_unanimous"])) in lines[0]
    for i, l in enumerate(CT.LABELS):
        n = len(CT.select(t, l))
        assert lines[1 + i].startswith("class2ktab: class %s: %d k-mers, %d table entries (minval 1, agreement 0%%), "
                                       "%d occurrences, 4 table parts" % (l, n, n, st["cns_total"][i]))


def test_the_h_table_through_the_reference_readers(scenario, run4):
    _, t = scenario
    out, _ = run4
    L = KO.ref_lib()
    if L is None:
        pytest.skip("the reference's own readers (oracle/_ref) are not built here")
    ents = CT.select(t, "H")
    other = [x for x, _ in CT.select(t, "D")[:30]]         # k-mers of another class are not in this table
    flip = [KO.key_of(O.canon(KO.text_of(x ^ 1, K).upper().encode())) for x, _ in ents[:30]]
    check_through_reference(L, out, "est.H", K, 1, ents, other + flip)


def test_one_thread(scenario, tmp_path):
    d, t = scenario
    out = str(tmp_path / "out")
    os.mkdir(out)
    r = run("-T1", "-N" + os.path.join(out, "est"), os.path.join(d, "est.class"), os.path.join(d, "reads.prof"))
    assert r.stderr == ""
    want = expect(tmp_path, "est", t, 1, 0, 1)
    assert len(want) == 4 * 3 and digest(out) == want
    shutil.rmtree(out)


def test_cutoff_agreement_and_root(scenario, tmp_path):
    d, t = scenario
    before = sorted(os.listdir(d))
    sub = str(tmp_path / "sub")
    os.mkdir(sub)
    run("-t2", "-a67", "-T3", "-N" + os.path.join(sub, "other"), os.path.join(d, "est.class"), os.path.join(d, "reads"))
    want = expect(tmp_path, "other", t, 2, 67, 3)
    plain = expect(tmp_path, "other", t, 1, 0, 3)
    got = digest(sub)
    assert got == want and sorted(os.listdir(d)) == before
    hists = {f: x for f, x in got.items() if f.endswith(".hist")}
    assert len(hists) == 4 and hists == {f: x for f, x in plain.items() if f.endswith(".hist")}
    assert {f: x for f, x in got.items() if "ktab" in f} != {f: x for f, x in plain.items() if "ktab" in f}
    shutil.rmtree(sub)


def test_gz_input_and_an_emptied_class(scenario, tmp_path):
    """est.class.gz: the default root drops .class.gz.  -t32767 empties every class: a stub and one empty part each."""
    d, t = scenario
    out = str(tmp_path / "gz")
    os.mkdir(out)
    with open(os.path.join(d, "est.class"), "rb") as f, gzip.open(os.path.join(out, "est.class.gz"), "wb") as g:
        g.write(f.read())
    run("-t32767", os.path.join(out, "est.class.gz"), os.path.join(d, "reads"))
    got = digest(out)
    del got["est.class.gz"]
    want = expect(tmp_path, "est", t, 32767, 0, 4)
    assert len(want) == 4 * 3 and got == want
    assert all(got[".est.%s.ktab.1" % l][0] == 12 for l in CT.LABELS)
    shutil.rmtree(out)

"""`kprof -t` on a real MI355X (`-m gpu`): the k-mer table files byte for byte against fastk.write_fastk_ktab of the
oracle's table, the other files untouched by -t, -f with -t, -k and -N, the files through the reference's own readers,
and the usage errors, which are reported before the GPU is touched."""
import os
import subprocess

import pytest

import kprof_oracle as O
import ktab_oracle as KO
from conftest import ROOT
from test_ktab_host import check_through_reference

pytestmark = pytest.mark.gpu
K = 40
KPROF = os.path.join(ROOT, "classpro_amd", "kprof")
NO_GPU = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


@pytest.fixture(scope="module")
def small(built):
    """The 60 kbp / 30x set of the kprof tests and its canonical counts at K = 40."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd import synth
    ds = synth.make_dataset(genome_len=60000, cov=30, read_len=6000, seed=11)
    seqs = [bytes(s) for s in ds["seqs"]]
    return ds["names"], seqs, O.count(seqs, K)[0]


def write_fasta(d, names, seqs):
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "reads.fasta")
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + s + b"\n")
    return path


def run(d, names, seqs, *args):
    src = write_fasta(d, names, seqs)
    r = subprocess.run([KPROF] + list(args) + [src], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    return r


def files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def expect_ktab(tmp, root, k, minc, ents, nparts):
    """{file name: bytes} of what fastk.write_fastk_ktab writes from the oracle's entries."""
    from classpro_amd import fastk
    d = os.path.join(tmp, "want_%s_%d_%d" % (root, minc, nparts))
    fastk.write_fastk_ktab(d, root, k, minc, [x for x, _ in ents], [c for _, c in ents], nparts)
    return files(d)


@pytest.mark.parametrize("threads", [1, 4])
def test_table_files_and_the_others_untouched(small, tmp_path, threads):
    names, seqs, cnt = small
    plain, tab = str(tmp_path / "plain"), str(tmp_path / "tab")
    run(plain, names, seqs, "-T%d" % threads)
    r = run(tab, names, seqs, "-v", "-t1", "-T%d" % threads)
    ents = KO.entries(cnt, 1)
    assert "%d table entries, minval 1, ibyte 3, %d table parts" % (len(ents), threads) in r.stderr
    got, base = files(tab), files(plain)
    want = expect_ktab(str(tmp_path), "reads", K, 1, ents, threads)
    assert len(want) == 1 + threads
    assert {f: b for f, b in got.items() if "ktab" in f} == want
    assert {f: b for f, b in got.items() if "ktab" not in f} == base and len(base) == 3 + 2 * threads


def test_filter_with_table(small, tmp_path):
    names, seqs, cnt = small
    a, b = str(tmp_path / "f"), str(tmp_path / "u")
    run(a, names, seqs, "-f1", "-t2")
    run(b, names, seqs, "-t2")
    fa, fb = files(a), files(b)
    assert fa == fb
    assert {f: x for f, x in fa.items() if "ktab" in f} == expect_ktab(str(tmp_path), "reads", K, 2, KO.entries(cnt, 2), 4)


def test_other_k_and_root_through_the_reference_readers(small, tmp_path):
    names, seqs, _ = small
    seqs = seqs[:6] + [b"ACGTAC", seqs[6][:300] + b"N" + seqs[6][300:600], b""]
    names = ["r%d" % i for i in range(len(seqs))]
    d = str(tmp_path / "in")
    sub = str(tmp_path / "sub")
    os.mkdir(sub)
    run(d, names, seqs, "-k21", "-t1", "-T3", "-N" + os.path.join(sub, "other"))
    ents = KO.table(seqs, 21)
    got = files(sub)
    assert {f: x for f, x in got.items() if "ktab" in f} == expect_ktab(str(tmp_path), "other", 21, 1, ents, 3)
    assert sorted(os.listdir(d)) == ["reads.fasta"]
    L = KO.ref_lib()
    if L is None:
        pytest.skip("the reference's own readers (oracle/_ref) are not built here")
    check_through_reference(L, sub, "other", 21, 1, ents, [KO.key_of(O.canon(KO.text_of(x ^ 1, 21).upper().encode())) for x, _ in ents[:50]])


def test_fewer_entries_than_threads(small, tmp_path):
    """Two table entries and -T4: one entry per part, two parts."""
    d = str(tmp_path)
    seqs = [b"ACGTTGCATGCATGCAAGTCAG"]
    run(d, ["r"], seqs, "-k21", "-t1")
    ents = KO.table(seqs, 21)
    assert len(ents) == 2
    assert {f: x for f, x in files(d).items() if "ktab" in f} == expect_ktab(d, "reads", 21, 1, ents, 2)
    e = str(tmp_path / "none")                             # no entry at all: one empty part
    run(e, ["r"], seqs, "-k21", "-t2")
    assert {f: x for f, x in files(e).items() if "ktab" in f} == expect_ktab(d, "reads", 21, 2, [], 1)


def test_usage_errors_do_not_touch_the_gpu(small, tmp_path):
    d = str(tmp_path)
    src = write_fasta(d, ["r1"], [b"ACGTACGTAC"])
    env = dict(os.environ, **NO_GPU)
    go = lambda *a: subprocess.run([KPROF] + list(a) + [src], capture_output=True, text=True, env=env)
    for bad, msg in (("-t0", "kprof: Table cutoff must lie in [1, 32767] (0)\n"),
                     ("-t40000", "kprof: Table cutoff must lie in [1, 32767] (40000)\n"),
                     ("-t-3", "kprof: Table cutoff must lie in [1, 32767] (-3)\n"),
                     ("-tx", "kprof: -t 'x' argument is not an integer\n"),
                     ("-t", "kprof: -t '' argument is not an integer\n")):
        r = go(bad)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), bad
    r = go("-t1", "-f1")
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("kprof: -t1 needs") and "-t2 or more" in r.stderr
    r = go("-k4", "-t1")
    assert r.returncode == 1 and r.stderr.startswith("kprof: -t needs a K-mer length of at least 5 (4)")
    r = go("-t1", "-N" + os.path.join(d, "no_such_dir", "out"))
    assert r.returncode == 1 and r.stderr == "kprof: Cannot open %s/no_such_dir/out.hist for 'w'\n" % d
    assert sorted(os.listdir(d)) == ["reads.fasta"]
    os.mkdir(os.path.join(d, "reads.ktab"))                # the stub cannot be created: a directory has its name
    r = go("-t1")
    assert r.returncode == 1 and r.stderr == "kprof: Cannot open %s/reads.ktab for 'w'\n" % d

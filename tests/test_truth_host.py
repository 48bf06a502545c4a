"""genome2class without a GPU: the brute-force oracle of tests/truth_oracle.py against an independent numpy
restatement (case fold, overlapping pieces), against prof2class run on the oracle's relative profiles, the label mix of
the case the GPU tests use, and the built command's error contract -- reported before the GPU is touched."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import kprof_oracle as O
import truth_oracle as TO
from conftest import ROOT

TOOLS = os.path.join(ROOT, "classpro_amd")
G2C = os.path.join(TOOLS, "genome2class")
REF = os.path.join(ROOT, "oracle", "_ref")
NO_GPU = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


@pytest.fixture(scope="module")
def case():
    return TO.make_case(5, K=40)


def numpy_keys(s, k, folded):
    """Canonical keys of one sequence as int64 (k <= 31) and which k-mers hold only A C G T (after the fold, if asked)."""
    code = np.full(256, 4, np.int64)
    for i, c in enumerate(b"ACGT"):
        code[c] = i
        if folded:
            code[c + 32] = i
    b = code[np.frombuffer(bytes(s), np.uint8)]
    n = max(len(b) - k + 1, 0)
    fw, rc, ok = np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, bool)
    for j in range(k):
        bj = b[j:j + n]
        ok &= bj < 4
        bj = np.minimum(bj, 3)
        fw = fw * 4 + bj
        rc = rc + ((3 - bj) << (2 * j))
    return np.minimum(fw, rc), ok


def numpy_rel(genome, reads, k):
    """Independent restatement: the genome's keys sorted and counted by np.unique, the reads' looked up by searchsorted."""
    gk = [numpy_keys(g, k, True) for g in genome]
    u, c = np.unique(np.concatenate([kk[ok] for kk, ok in gk]), return_counts=True)
    out = []
    for s in reads:
        kk, ok = numpy_keys(s, k, False)
        i = np.minimum(np.searchsorted(u, kk), len(u) - 1)
        hit = ok & (u[i] == kk)
        out.append(np.where(hit, np.minimum(c[i], O.MAXC), 0).astype(np.uint16))
    return out, u, c


@pytest.mark.parametrize("k", [2, 21, 31])
def test_oracle_agrees_with_numpy_restatement(case, k):
    genome = case["genome"]
    reads = case["seqs"][:40] + [b"", b"ACG", b"acgtACGTACGTACGTACGTACGTACGTACGTACGTAC", case["genome"][0][17900:19000]]
    want = TO.rel_profiles(genome, reads, k)
    got, u, c = numpy_rel(genome, reads, k)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    cnt = TO.genome_counter(genome, k)
    assert np.array_equal(np.sort(c), np.sort(np.array(list(cnt.values()), np.int64)))
    # the soft-masked stretch counts (fold), and a read that holds lower case itself does not
    masked = case["genome"][0][18000:18900]
    assert masked.islower() and TO.rel_profiles(genome, [masked.upper()], k)[0].min() >= 1
    assert not TO.rel_profiles(genome, [masked], k)[0].any()


@pytest.mark.parametrize("k", [21, 31])
def test_overlapping_pieces_count_every_kmer_once(case, k):
    genome = case["genome"]
    whole = TO.genome_counter(genome, k)
    for b in (1, 64, 1000, 7777, 10 ** 6):
        pieces = [p for g in genome for p in TO.cut(g, b, k)]
        assert all(len(p) <= b + k - 1 for p in pieces)
        assert TO.genome_counter(pieces, k) == whole, b
        if k == 21 and b >= 64:
            keys = [numpy_keys(p, k, True) for p in pieces]
            u, c = np.unique(np.concatenate([kk[ok] for kk, ok in keys]), return_counts=True)
            assert int(c.sum()) == sum(whole.values()) and len(u) == len(whole)
        if b >= 7777:
            continue
        assert len(pieces) > len(genome)
    assert isinstance(whole, Counter)


@pytest.mark.parametrize("k", [21, 40])
def test_case_holds_every_label(case, k):
    """A degenerate case cannot pass silently: at least 1000 k-mer positions of each of E, H, D and R."""
    c = case if k == 40 else TO.make_case(5, K=k)
    rel = TO.rel_profiles(c["genome"], c["seqs"], k)
    labs = [TO.labels(r, len(s), k) for r, s in zip(rel, c["seqs"])]
    n = TO.label_counts(labs)
    assert min(n) >= 1000, n
    lens = [len(s) for s in c["seqs"]]
    assert k - 1 in lens and any(l < k - 1 for l in lens) and sum(b"N" in s for s in c["seqs"]) == 1
    assert sum(lens) > 20 * 40000 and all(3000 <= l <= 8100 for l in lens if l >= k)
    assert any(b"N" in g for g in c["genome"]) and any(g != g.upper() for g in c["genome"])


def _prof2class_bins():
    out = [os.path.join(TOOLS, "prof2class")]
    if os.access(os.path.join(REF, "prof2class"), os.X_OK):
        out.append(os.path.join(REF, "prof2class"))
    return out


def test_oracle_text_is_what_prof2class_writes(built, case, tmp_path):
    """The oracle's relative profiles as FASTK files through prof2class (ours, and the reference's own binary when it is
    there): the .class it writes is class_text of the oracle's labels."""
    from classpro_amd import fastk
    k = 40
    names, seqs = case["names"][:30], case["seqs"][:30]
    cnt = TO.genome_counter(case["genome"], k)
    rel = TO.rel_profiles(case["genome"], seqs, k, counter=cnt)
    want = TO.class_text(names, seqs, [TO.labels(r, len(s), k) for r, s in zip(rel, seqs)])
    for n, tool in enumerate(_prof2class_bins()):
        d = os.path.join(str(tmp_path), str(n))
        fastk.write_fastk(d, "reads.truth", k, rel, O.hist(cnt), nparts=2)
        fastk.write_fasta(os.path.join(d, "reads.fasta"), names, seqs)
        r = subprocess.run([tool, os.path.join(d, "reads.truth.prof"), os.path.join(d, "reads.fasta")], capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stderr
        assert open(os.path.join(d, "reads.truth.class"), "rb").read() == want, tool


def test_command_is_built(built):
    assert os.path.exists(G2C) and os.access(G2C, os.X_OK), "classpro_amd/genome2class was not built"


def test_error_contract_without_a_gpu(built, tmp_path):
    """HIP sees no device here, so a command that touched the GPU first could not answer like this."""
    d = str(tmp_path)
    env = dict(os.environ, **NO_GPU)
    gen, src = os.path.join(d, "genome.fasta"), os.path.join(d, "reads.fasta")
    with open(gen, "wb") as f:
        f.write(b">c1\nACGTACGTACGGATTACA\n")
    with open(src, "wb") as f:
        f.write(b">r1\nACGTACGTAC\n")
    run = lambda *a: subprocess.run([G2C] + list(a), capture_output=True, text=True, env=env)
    usage = ("Usage: genome2class [-v] [-p] [-k<int(40)>] [-T<int(4)>] [-b<int(67108864)>] [-N<out_root>] [-A<est.class>]\n"
             "                    <genome>[.f[ast][aq][.gz]|.db|.dam] <source>[.db|.dam|.f[ast][aq][.gz]]\n")
    for a in ([], ["-v"], [gen], [gen, src, src]):
        r = run(*a)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", usage), a
    r = run("-q", gen, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "genome2class: -q is an illegal option\n")
    for k in ("1", "64", "100"):
        r = run("-k" + k, gen, src)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "genome2class: K-mer length must lie in [2, 63] (%s)\n" % k)
    for bad, msg in (("-k0", "K-mer length must be positive (0)"), ("-T0", "Number of threads must be positive (0)"),
                     ("-T-2", "Number of threads must be positive (-2)"),
                     ("-b0", "Bases per device batch must be positive (0)"),
                     ("-b-5", "Bases per device batch must be positive (-5)"),
                     ("-kx", "-k 'x' argument is not an integer"), ("-b", "-b '' argument is not an integer"),
                     ("-A", "-A needs a path (-A<est.class>)")):
        r = run(bad, gen, src)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "genome2class: %s\n" % msg), bad
    cannot = "genome2class: Cannot open %s/nope as a .db|.dam or .f{ast}[aq][.gz] file\n" % d
    for a in ([os.path.join(d, "nope"), src], [gen, os.path.join(d, "nope")]):
        r = run(*a)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", cannot), a
    for flags, ext in (([], "class"), (["-p"], "class")):
        r = run("-N" + os.path.join(d, "no_such_dir", "out"), *flags, gen, src)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", "genome2class: Cannot open %s/no_such_dir/out.%s for 'w'\n" % (d, ext))
    os.mkdir(os.path.join(d, "o"))
    os.mkdir(os.path.join(d, "o", "x.prof"))                       # the .class can be made, the profile stub cannot
    r = run("-p", "-N" + os.path.join(d, "o", "x"), gen, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "genome2class: Cannot open %s/o/x.prof for 'w'\n" % d)
    r = run("-A" + os.path.join(d, "no.class"), "-N" + os.path.join(d, "o", "y"), gen, src)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "genome2class: Cannot open %s/no.class [errno=2]\n" % d)
    assert sorted(os.listdir(d)) == ["genome.fasta", "o", "reads.fasta"]


def test_python_mirror_is_present():
    from classpro_amd import api
    from classpro_amd._lib import SYMBOLS
    assert callable(api.KmerCounts.rel_labels) and "cp_kmer_counts_rel_labels" in SYMBOLS

"""The per-class k-mer tables without a GPU: the restatement of tests/cnstab_oracle.py against the count-table oracles
(the four classes partition the canonical k-mers of the reads, their histograms sum to the reads' histogram), the
agreement arithmetic, and every usage error of class2ktab, which is reported before the GPU is touched and leaves
nothing behind.  Everything is integers and bytes: the tolerance is zero."""
import os
import subprocess

import numpy as np
import pytest

import cns_oracle as C
import cnstab_oracle as CT
import eval_case
import kprof_oracle as O
import ktab_oracle as KO
from conftest import ROOT

K = eval_case.K
TOOL = os.path.join(ROOT, "classpro_amd", "class2ktab")
NO_GPU = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
USAGE = ("Usage: class2ktab [-v] [-T<int(4)>] [-t<int(1)>] [-a<int(0)>] [-N<out_root>] <estimate>.class[.gz] "
         "<fastk_root>[.prof]\n")


@pytest.fixture(scope="module")
def scenario(built, tmp_path_factory):
    """The evaluation scenario with its oracle-written est.class: (directory, label table, canonical counts)."""
    d = str(tmp_path_factory.mktemp("cnstab"))
    case = eval_case.build_case(d, eval_case.oracle_labels, True)
    t, skipped = C.table(C.read_class(os.path.join(d, "est.class")), K, True)
    assert skipped == 0
    return d, t, O.count([bytes(s) for s in case["seqs"]], K)[0]


def test_classes_partition_the_count_table(scenario):
    _, t, cnt = scenario
    per = [CT.select(t, l) for l in CT.LABELS]
    assert all(len(p) > 0 for p in per)
    merged = sorted(e for p in per for e in p)
    assert merged == KO.entries(cnt) == CT.select(t)
    assert len({k for k, _ in merged}) == len(merged) == sum(len(p) for p in per)
    for l, p in zip(CT.LABELS, per):
        assert all(CT.LABELS[C.consensus_label(t[k])] == l and sum(t[k]) == c for k, c in p)


def test_histograms_sum_to_the_count_histogram(scenario):
    _, t, cnt = scenario
    h, il, ih = CT.class_hist(t)
    low, high, ilow, ihigh, want = O.hist(cnt)
    assert (low, high) == (1, CT.MAXC)
    assert np.array_equal(h.sum(0), want) and int(il.sum()) == ilow and int(ih.sum()) == ihigh
    assert [int(x.sum()) for x in h] == [len(CT.select(t, l)) for l in CT.LABELS]


def test_filters_shrink_a_class(scenario):
    _, t, _ = scenario
    base = [len(CT.select(t, l)) for l in CT.LABELS]
    for kw in (dict(min_total=2), dict(min_pct=67)):
        got = [CT.select(t, l, **kw) for l in CT.LABELS]
        assert all(len(g) <= b for g, b in zip(got, base)) and any(len(g) < b for g, b in zip(got, base))
        for l, g in zip(CT.LABELS, got):
            assert set(g) <= set(CT.select(t, l))
    unanimous = [k for k, c in t.items() if sum(c) == max(c)]
    assert sorted(k for k, _ in CT.select(t, None, 1, 100)) == sorted(unanimous)


def test_agreement_arithmetic():
    t = {1: [2, 1, 0, 0], 2: [1, 1, 0, 0], 3: [0, 0, 5, 0], 4: [1, 1, 1, 1], 5: [0, 3, 0, 1]}
    assert [k for k, _ in CT.select(t, "E")] == [1] and [k for k, _ in CT.select(t, "H")] == [2, 5]
    assert (1, 3) in CT.select(t, "E", 1, 66) and CT.select(t, "E", 1, 67) == []
    assert (2, 2) in CT.select(t, "H", 1, 50) and (2, 2) not in CT.select(t, "H", 1, 51)
    assert CT.select(t, None, 1, 100) == [(3, 5)]
    assert CT.select(t, "R") == [(4, 4)] and CT.select(t, "R", 1, 25) == [(4, 4)] and CT.select(t, "R", 1, 26) == []
    assert CT.select(t, None, 4) == [(3, 5), (4, 4), (5, 4)] and CT.select(t, "H", 1, 75) == [(5, 4)]
    h, il, ih = CT.class_hist(t)
    assert h[1, 1] == 1 and h[1, 3] == 1 and h[0, 2] == 1 and il.tolist() == [0, 0, 0, 0] and ih.tolist() == [0] * 4
    h, il, ih = CT.class_hist({7: [40000, 0, 0, 0], 8: [1, 0, 0, 0], 9: [0, 0, 0, 32767]})
    assert h[0, CT.MAXC - 1] == 1 and ih.tolist() == [40000, 0, 0, 32767] and il.tolist() == [1, 0, 0, 0]


def listing(d):
    return sorted(os.path.join(r, f)[len(d):] for r, ds, fs in os.walk(d) for f in fs + ds)


def test_usage_errors_do_not_touch_the_gpu(scenario):
    from classpro_amd import fastk
    d = scenario[0]
    est, root = os.path.join(d, "est.class"), os.path.join(d, "reads")
    fastk.write_fastk(d, "k4", 4, [np.zeros(3, np.uint16)], (1, CT.MAXC, 0, 0, np.zeros(CT.MAXC, np.int64)))
    os.makedirs(os.path.join(d, "blocked", "out.D.hist"), exist_ok=True)     # a directory has the name of an output
    before = listing(d)
    env = dict(os.environ, **NO_GPU)
    go = lambda *a: subprocess.run([TOOL] + list(a), capture_output=True, text=True, env=env)
    cases = [((), USAGE), ((est,), USAGE), ((est, root, root), USAGE),
             (("-q", est, root), "class2ktab: -q is an illegal option\n"),
             (("-vZ", est, root), "class2ktab: -Z is an illegal option\n"),
             (("-tx", est, root), "class2ktab: -t 'x' argument is not an integer\n"),
             (("-t", est, root), "class2ktab: -t '' argument is not an integer\n"),
             (("-t0", est, root), "class2ktab: Table cutoff must lie in [1, 32767] (0)\n"),
             (("-t32768", est, root), "class2ktab: Table cutoff must lie in [1, 32767] (32768)\n"),
             (("-a-1", est, root), "class2ktab: Agreement must lie in [0, 100] (-1)\n"),
             (("-a101", est, root), "class2ktab: Agreement must lie in [0, 100] (101)\n"),
             (("-a5x", est, root), "class2ktab: -a '5x' argument is not an integer\n"),
             (("-T0", est, root), "class2ktab: Number of threads must be positive (0)\n"),
             (("-T-2", est, root), "class2ktab: Number of threads must be positive (-2)\n"),
             ((os.path.join(d, "nothere.class"), root), "class2ktab: Cannot open %s/nothere.class [errno=2]\n" % d),
             ((est, os.path.join(d, "nothere")), "class2ktab: Cannot open %s/nothere.prof\n" % d),
             ((est, os.path.join(d, "k4")), "class2ktab: needs a K-mer length of at least 5 (4): a k-mer table has one to "
                                             "three prefix bytes\n"),
             (("-N" + os.path.join(d, "no_such_dir", "out"), est, root),
              "class2ktab: Cannot open %s/no_such_dir/out.E.ktab for 'w'\n" % d),
             (("-N" + os.path.join(d, "blocked", "out"), est, root),
              "class2ktab: Cannot open %s/blocked/out.D.hist for 'w'\n" % d)]
    for args, msg in cases:
        r = go(*args)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), args
        assert listing(d) == before, args

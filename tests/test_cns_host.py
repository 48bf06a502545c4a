"""class2cns without flags (the reference's src/class2cns.c: host only, no GPU) against the Python restatement of
tests/cns_oracle.py, and the restatement itself: its `sort | uniq -c` against coreutils, its fixed-point consistency
against exact fractions."""
import gzip
import os
import random
import shutil
import subprocess
from fractions import Fraction

import pytest

import cns_oracle as O
import eval_case
from conftest import ROOT

CNS = os.path.join(ROOT, "classpro_amd", "class2cns")


@pytest.fixture(scope="module", params=[True, False], ids=["with_short_read", "no_short_read"])
def scenario(request, built, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cns%d" % request.param))
    eval_case.build_case(d, eval_case.oracle_labels, request.param)
    return d


def run(args):
    return subprocess.run([CNS] + args, capture_output=True)


def test_dump_matches_restatement(scenario):
    d = scenario
    est = os.path.join(d, "est.class")
    recs = O.read_class(est)
    want = O.dump(recs, eval_case.K)
    r = run([est, os.path.join(d, "reads")])
    assert r.returncode == 0 and r.stderr == b""
    assert r.stdout == want
    # .class.gz through the same reader, and the root given with its .prof suffix
    with open(est, "rb") as f, gzip.open(est + ".gz", "wb") as g:
        g.write(f.read())
    r = run([est + ".gz", os.path.join(d, "reads.prof")])
    assert r.returncode == 0 and r.stdout == want


def test_dump_sort_uniq_pinned_to_coreutils(scenario):
    if not (shutil.which("sort") and shutil.which("uniq")):
        pytest.skip("coreutils sort / uniq not on this machine")
    d = scenario
    est = os.path.join(d, "est.class")
    text = run([est, os.path.join(d, "reads")]).stdout
    env = dict(os.environ, LC_ALL="C")
    s = subprocess.run(["sort"], input=text, capture_output=True, env=env, check=True).stdout
    u = subprocess.run(["uniq", "-c"], input=s, capture_output=True, env=env, check=True).stdout
    assert u == O.sort_uniq(text)
    t, skipped = O.table(O.read_class(est), eval_case.K)
    assert skipped == 0
    assert O.uniq_table(t, eval_case.K) == u


def test_usage_and_errors(scenario):
    d = scenario
    est, root = os.path.join(d, "est.class"), os.path.join(d, "reads")
    for args in ([], [est], [est, root, root]):
        r = run(args)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr == b"Usage: class2cns [-v] [-c] [-u] [-x] [-C<out.class>] <estimate>.class <fastk_root>[.prof]\n"
    r = run(["-q", est, root])
    assert r.returncode == 1 and r.stderr == b"class2cns: -q is an illegal option\n"
    r = run(["-uZ", est, root])
    assert r.returncode == 1 and r.stderr == b"class2cns: -Z is an illegal option\n"
    r = run([os.path.join(d, "nothere.class"), root])
    assert r.returncode == 1 and r.stderr == b"class2cns: Cannot open %s [errno=2]\n" % os.path.join(d, "nothere.class").encode()
    r = run([est, os.path.join(d, "nothere")])
    assert r.returncode == 1 and r.stderr == b"class2cns: Cannot open %s.prof\n" % os.path.join(d, "nothere").encode()


def test_fixed_point_consistency_is_exact():
    rng = random.Random(7)
    edge = [[1, 0, 0, 0], [1, 1, 1, 1], [0, 0, 0, 2**32 - 1], [2**32 - 1] * 4, [2**32 - 2, 2**32 - 1, 5, 0], [3, 0, 2, 0]]
    for trial in range(200):
        n = rng.choice([1, 2, 3, 10, 100, 1000])
        cs = [c for c in ([rng.choice([0, 0, 1, 2, 3, 7, 2**31, 2**32 - 1]) for _ in range(4)] for _ in range(n)) if max(c)]
        if trial < len(edge):
            cs = cs + [edge[trial]]
        if not cs:
            continue
        s = O.s_fixed(cs)
        # every term is floor(total * 2^64 / max): exact against fractions
        assert s == sum((Fraction(sum(c), max(c)) * 2**64).__floor__() for c in cs)
        got = O.consistency(len(cs), s)
        assert got == float(Fraction(len(cs) << 64, s))                       # correctly rounded
        hm = len(cs) / sum(1.0 / (max(c) / sum(c)) for c in cs)                # agg2cons.py's hmean, in floats
        assert abs(got - hm) <= 1e-12 * hm
        assert abs(got - float(O.consistency_exact(cs))) <= 1e-12 * got


def test_consensus_tie_rule():
    assert O.consensus_label([1, 1, 0, 0]) == 1            # E = H: H
    assert O.consensus_label([0, 2, 2, 0]) == 2            # H = D: D
    assert O.consensus_label([0, 0, 3, 3]) == 3            # D = R: R
    assert O.consensus_label([4, 4, 4, 4]) == 3            # all four: R
    assert O.consensus_label([5, 4, 4, 4]) == 0

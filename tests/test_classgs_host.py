"""ClassGS without a GPU: the golden data of tests/golden/classgs.json (outputs of the reference's own ClassGS, written by
scripts/gen_classgs_golden.py) is pinned to the scenarios the tests regenerate, the built command reports usage errors
and unreadable inputs exactly as the reference does -- before it touches the GPU -- and the new entry points are part of
the ABI."""
import hashlib
import json
import os
import re
import subprocess

import pytest

import classgs_case as cc
from conftest import ROOT

GS = os.path.join(ROOT, "classpro_amd", "ClassGS")
NEW_SYMBOLS = ["cp_threshold_labels", "cp_acc_create", "cp_acc_add", "cp_acc_read", "cp_acc_destroy"]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "classgs.json")))


@pytest.mark.parametrize("tiny", [True, False], ids=["tiny", "notiny"])
@pytest.mark.parametrize("kind", cc.KINDS)
def test_restated_chain_reproduces_the_reference_output(kind, tiny, golden, tmp_path):
    """The scenario regenerated here is the one the golden was made from (input sha256), and the ten-line restatement of
    ClassGS.c:228-248 gives the reference's .GS.class on it, byte for byte (sha256, size, per-label counts)."""
    d = str(tmp_path)
    sc = cc.build_scenario(d, kind, tiny)
    assert cc.input_sha(d) == golden["scenarios"][cc.scenario_id(kind, tiny)]["input_sha256"]
    for thres in cc.THRESHOLDS:
        g = golden["cases"][cc.case_id(kind, tiny, thres)]
        data, counts = cc.expected_class(sc, thres)
        assert len(data) == g["size"] and hashlib.sha256(data).hexdigest() == g["sha256"], thres
        assert counts == g["counts"], thres
        distinct = sum(1 for ch in "EHDR" if g["counts"][ch] > 0)
        assert distinct >= 3 or thres == ("0", "0", "0"), (thres, g["counts"])
        assert g["returncode"] == 0
    if kind == "fasta" and tiny:
        c = golden["cases"][cc.case_id(kind, tiny, ("8", "25", "60"))]["counts"]
        assert (c["E"], c["H"], c["D"], c["R"]) == (90248, 164398, 339757, 602004)


def test_error_contract_matches_the_reference_without_a_gpu(built, golden, tmp_path):
    """4 arguments, -q, a missing source, a negative threshold, a FASTX read of 60001 bases, threshold strings that are
    not numbers: the reference's text and exit status.  HIP sees no device here, so a command that touched the GPU
    first could not answer like this."""
    assert os.path.exists(GS), "classpro_amd/ClassGS was not built"
    d = str(tmp_path)
    cc.build_error_dir(d)
    assert cc.input_sha(d) == golden["error_input_sha256"]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    assert set(golden["errors"]) == {n for n, _a in cc.ERROR_CASES}
    for name, args in cc.ERROR_CASES:
        g = golden["errors"][name]
        r = subprocess.run([GS] + [x.format(dir=d) for x in args], capture_output=True, text=True, env=env)
        assert r.returncode == g["returncode"] == 1, (name, r.stderr)
        assert r.stderr.replace(d, "{dir}") == g["stderr"], name
        assert r.stdout == g["stdout"] == "", name


def test_truth_file_that_cannot_be_opened(built, tmp_path):
    d = str(tmp_path)
    cc.build_error_dir(d)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([GS, "-A" + os.path.join(d, "nope.class"), os.path.join(d, "long"), "8", "25", "60"],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "ClassGS: Cannot open %s/nope.class" % d in r.stderr
    r = subprocess.run([GS, "-A", os.path.join(d, "long"), "8", "25", "60"], capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "-A needs a path" in r.stderr


def test_new_symbols_are_declared_listed_and_exported(built):
    from classpro_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpro_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), "%s is not declared in include/classpro_amd.h" % s
        assert s in _lib.SYMBOLS, "%s is not listed in classpro_amd._lib.SYMBOLS" % s
        assert hasattr(L, s), "libclasspro_amd.so does not export %s" % s


def test_python_mirror_is_present():
    from classpro_amd import api
    assert callable(api.threshold_labels) and hasattr(api.LabelAccuracy, "add") and hasattr(api.LabelAccuracy, "stats")

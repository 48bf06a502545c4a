"""Writes tests/golden/classgs.json from the reference's own ClassGS.

    python scripts/gen_classgs_golden.py --ref <directory of the reference's src>

The reference's ClassGS.c is compiled into a temporary directory outside the repository

    gcc -O3 -w -I$REF $REF/ClassGS.c $REF/libfastk.c $REF/DB.c $REF/QV.c -lm -lz -lpthread

and run on the scenarios of tests/classgs_case.py.  Recorded per case: sha256 and size of reads.GS.class, the
per-label character counts, stderr with the directory replaced by {dir}, the exit status, and the sha256 of the
inputs.  Every output is also compared with the restated chain of tests/classgs_case.py before it is recorded.  The
binary is removed with the temporary directory; only data goes into the repository.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import classgs_case as cc   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ref", required=True, help="directory holding the reference's ClassGS.c, libfastk.c, DB.c, QV.c")
    a = ap.parse_args()
    ref = os.path.abspath(a.ref)
    out = dict(scenarios={}, cases={}, errors={})
    with tempfile.TemporaryDirectory(prefix="classgs_golden") as tmp:
        exe = os.path.join(tmp, "ClassGS")
        subprocess.check_call(["gcc", "-O3", "-w", "-I" + ref] + [os.path.join(ref, f) for f in
                              ("ClassGS.c", "libfastk.c", "DB.c", "QV.c")] + ["-o", exe, "-lm", "-lz", "-lpthread"])
        for kind in cc.KINDS:
            for tiny in (True, False):
                d = os.path.join(tmp, cc.scenario_id(kind, tiny))
                os.mkdir(d)
                sc = cc.build_scenario(d, kind, tiny)
                out["scenarios"][cc.scenario_id(kind, tiny)] = dict(input_sha256=cc.input_sha(d), reads=len(sc["seqs"]))
                for thres in cc.THRESHOLDS:
                    r = subprocess.run([exe, os.path.join(d, "reads")] + list(thres), capture_output=True, text=True)
                    data = open(os.path.join(d, "reads.GS.class"), "rb").read()
                    want, counts = cc.expected_class(sc, thres)
                    assert r.returncode == 0 and data == want, (kind, tiny, thres, r.stderr)
                    out["cases"][cc.case_id(kind, tiny, thres)] = dict(
                        sha256=hashlib.sha256(data).hexdigest(), size=len(data), counts=counts,
                        stderr=r.stderr.replace(d, "{dir}"), returncode=r.returncode)
                    os.remove(os.path.join(d, "reads.GS.class"))
        d = os.path.join(tmp, "errors")
        os.mkdir(d)
        cc.build_error_dir(d)
        out["error_input_sha256"] = cc.input_sha(d)
        for name, args in cc.ERROR_CASES:
            r = subprocess.run([exe] + [x.format(dir=d) for x in args], capture_output=True, text=True)
            out["errors"][name] = dict(stderr=r.stderr.replace(d, "{dir}"), stdout=r.stdout, returncode=r.returncode)
    path = os.path.join(ROOT, "tests", "golden", "classgs.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d error cases" % (path, len(out["cases"]), len(out["errors"])))


if __name__ == "__main__":
    main()

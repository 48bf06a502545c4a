"""k_classify_unrel_grp commits the slots of a speculation round on the slots' own lanes: same classes, same labels.  `-m gpu`.

Interval classes after STAGE_CLASS_ALL and the label strings against the oracle's on the reads of
tests/unrel_paint_inputs.py (tests/test_unrel_paint_inputs.py shows that they reach the clash path, the set-change
path and the K = 8 size class), with the second sweep as shipped and evaluating everything (CLASSPRO_UNREL_SWEEP2=full),
from compact and from full records (CLASSPRO_COMPACT_REL=0): four runs, equal to each other and to the oracle.
"""
import numpy as np
import pytest

from unrel_paint_inputs import K, READ_LEN, HCOV, DCOV, inputs

pytestmark = pytest.mark.gpu


def test_commit_by_slot_lanes_equals_oracle(built, monkeypatch):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd.api import Classifier, Batch, STAGE_CLASS_ALL
    seqs, profs, recs = inputs()
    want_lab = b"".join(r["lab"] for r in recs)
    want_cls = b"".join(r["call"]["asgn"].tobytes() for r in recs)
    out = []
    for sweep2 in (None, "full"):
        for compact in (None, "0"):
            for name, v in (("CLASSPRO_UNREL_SWEEP2", sweep2), ("CLASSPRO_COMPACT_REL", compact)):
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, v)
            clf = Classifier(K, READ_LEN, HCOV, DCOV)
            b = Batch.from_reads(seqs, profs)
            lab = clf.classify(b).tobytes()
            clf.run(b, STAGE_CLASS_ALL)
            clf.check()
            ivs = clf.intervals(b)
            assert [len(iv) for iv, _ in ivs] == [len(r["call"]) for r in recs]
            out.append((lab, b"".join(iv["asgn"].tobytes() for iv, _ in ivs)))
            clf.close()
    monkeypatch.delenv("CLASSPRO_UNREL_SWEEP2", raising=False)
    monkeypatch.delenv("CLASSPRO_COMPACT_REL", raising=False)
    for k, o in enumerate(out):
        assert o[1] == want_cls, "interval classes, run %d" % k
        assert o[0] == want_lab, "labels, run %d" % k
    assert all(o == out[0] for o in out[1:])

"""k_classify_unrel_grp with a round's loads in flight together and its parameters outside the loop: same classes, same
labels as the oracle, byte for byte.  `-m gpu`.

The reads of tests/unrel_round_inputs.py (tests/test_unrel_round_inputs.py shows what they reach) through
STAGE_CLASS_ALL and the whole path: with the default tables, with a Skellam table of 1 MB (most look-ups outside it: the
early loads beside the on-the-spot recurrence) and with none (CLASSPRO_SKELLAM_TABLE_MB=0); from compact and from full
records (CLASSPRO_COMPACT_REL=0); with the second sweep evaluating everything (CLASSPRO_UNREL_SWEEP2=full).
"""
import pytest

from unrel_round_inputs import K, READ_LEN, HCOV, DCOV, inputs

pytestmark = pytest.mark.gpu

KNOBS = ("CLASSPRO_SKELLAM_TABLE_MB", "CLASSPRO_COMPACT_REL", "CLASSPRO_UNREL_SWEEP2")
RUNS = [(None, None, None), ("1", None, None), ("0", None, None), (None, "0", None), ("1", "0", None), ("0", "0", "full"),
        (None, None, "full")]


@pytest.mark.parametrize("skel_mb,compact,sweep2", RUNS)
def test_round_loads_equal_oracle(built, monkeypatch, skel_mb, compact, sweep2):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd.api import Classifier, Batch, STAGE_CLASS_ALL
    seqs, profs, recs = inputs()
    want_lab = b"".join(r["lab"] for r in recs)
    want_cls = b"".join(r["call"]["asgn"].tobytes() for r in recs)
    for name, v in zip(KNOBS, (skel_mb, compact, sweep2)):
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
    clf.close()
    assert [len(iv) for iv, _ in ivs] == [len(r["call"]) for r in recs]
    assert b"".join(iv["asgn"].tobytes() for iv, _ in ivs) == want_cls, "interval classes"
    assert lab == want_lab, "labels"

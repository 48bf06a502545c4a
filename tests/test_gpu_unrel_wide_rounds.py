"""k_classify_unrel_grp with four lanes per slot (eight slots per round for N <= 256, sixteen above): same classes, same
labels as the oracle, byte for byte.  `-m gpu`.

The reads of tests/unrel_wide_inputs.py (tests/test_unrel_wide_inputs.py shows what they reach) in one batch, in the
given and in the reversed order -- an odd number of reads, so the last wave of the main class holds one -- through
STAGE_CLASS_ALL and the whole path in five runs: the default knobs; the second sweep evaluating everything
(CLASSPRO_UNREL_SWEEP2=full); full records (CLASSPRO_COMPACT_REL=0); no tables (CLASSPRO_TABLES=0: both look-ups of a
lane take the out-of-line path); a Skellam table of 1 MB (most Skellam look-ups outside it, the binomial one inside: one
of a lane's two look-ups in its table, the other not).  Every run equals the oracle, and so every other run.
"""
import pytest

from unrel_wide_inputs import K, READ_LEN, HCOV, DCOV, inputs

pytestmark = pytest.mark.gpu

KNOBS = ("CLASSPRO_UNREL_SWEEP2", "CLASSPRO_COMPACT_REL", "CLASSPRO_TABLES", "CLASSPRO_SKELLAM_TABLE_MB")
RUNS = {"default": (None, None, None, None), "sweep2_full": ("full", None, None, None), "full_records": (None, "0", None, None),
        "no_tables": (None, None, "0", None), "skellam_1mb": (None, None, None, "1")}
_seen = {}                                                 # (classes, labels) of the runs so far, per order


@pytest.mark.parametrize("reverse", [False, True], ids=["given", "reversed"])
@pytest.mark.parametrize("run", list(RUNS))
def test_wide_rounds_equal_oracle(built, monkeypatch, run, reverse):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd.api import Classifier, Batch, STAGE_CLASS_ALL
    seqs, profs, recs = inputs()
    assert len(recs) % 2 == 1
    if reverse:
        seqs, profs, recs = seqs[::-1], profs[::-1], recs[::-1]
    want_lab = b"".join(r["lab"] for r in recs)
    want_cls = b"".join(r["call"]["asgn"].tobytes() for r in recs)
    for name, v in zip(KNOBS, RUNS[run]):
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
    cls = b"".join(iv["asgn"].tobytes() for iv, _ in ivs)
    assert cls == want_cls, "interval classes"
    assert lab == want_lab, "labels"
    first = _seen.setdefault(reverse, (cls, lab))
    assert (cls, lab) == first, "equal to the other runs"

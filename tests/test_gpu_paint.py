"""k_paint_labels alone: the label string of every read is its own intervals, painted.  `-m gpu`.

The labels of clf.classify(b) against the string rebuilt on the host from that same run's clf.intervals(b) -- K-1 'N',
then every interval's class letter over e-b positions -- on the compact path ((end, class) words) and on the
full-record path (CLASSPRO_COMPACT_REL=0), and against the oracle's labels.  The reads of tests/unrel_paint_inputs.py
(pieces of 16 bytes with three and more interval ends, every alignment of a read's first label, reads beyond the
kernel's interval table) and reads of K-1, K, K+1 and K+15 bases.
"""
import numpy as np
import pytest

from unrel_paint_inputs import K, READ_LEN, HCOV, DCOV, inputs, short_reads, labels_from_intervals

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("compact", [None, "0"], ids=["compact", "records"])
def test_labels_are_the_painted_intervals(built, monkeypatch, compact):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from classpro_amd.api import Classifier, Batch
    seqs, profs, recs = inputs()
    t_s, t_p = short_reads()
    want = [r["lab"] for r in recs] + [b"N" * len(t_s[0])]              # (no k-mer: ClassPro.c:209-226 prints N's)
    from oracle.oracle import Oracle
    O = Oracle(K, READ_LEN, HCOV, DCOV)
    want += [O.classify_read(s, p) for s, p in zip(t_s[1:], t_p[1:])]
    # the short reads in front as well: the reads behind them start at other alignments of the label buffer
    seqs, profs, want = t_s + list(seqs) + t_s, t_p + list(profs) + t_p, want[-4:] + want
    if compact is None:
        monkeypatch.delenv("CLASSPRO_COMPACT_REL", raising=False)
    else:
        monkeypatch.setenv("CLASSPRO_COMPACT_REL", compact)
    clf = Classifier(K, READ_LEN, HCOV, DCOV)
    b = Batch.from_reads(seqs, profs)
    lab = clf.classify(b)
    ivs = clf.intervals(b)
    clf.close()
    monkeypatch.delenv("CLASSPRO_COMPACT_REL", raising=False)
    so = b.seq_off_h
    assert max(len(iv) for iv, _ in ivs) > 511 and min(len(iv) for iv, _ in ivs) == 0
    for r, (iv, _) in enumerate(ivs):
        got = lab[so[r]:so[r + 1]].tobytes()
        assert got == labels_from_intervals(iv, int(so[r + 1] - so[r])), "read %d against its own intervals" % r
        assert got == want[r], "read %d against the oracle" % r

"""The two cell policies of classify_rel's DP (cp_class.h) give the same result: anchors of cp_dh_ratio looked up through
`eff` (cp_cell, what the sequential kernel and the one-read-per-wave class do) against the anchors' (end_pos, end_cnt)
pairs carried in the cells (cp_cell_anc, what the main class of k_classify_rel_grp does).  CPU only.

tests/rel_anchor_probe.cpp runs one direction of a read under either policy.  Compared per (read, direction): the
traceback's assignment, the assignment after the coverage heuristics, the back-pointers, the "absolutely repeat" flags,
whether the pass was repeated, and the bits of hdrr.

The two policies can only differ where a look-up lands on a stand-in (eff[k] != k: the anchor was set on an "only R
reachable" step, so the pair is the one carried by the pass and not the interval's own).  The probe counts those
look-ups; the test requires some in each direction.  Counted on these inputs: the adversarial reads give several hundred
per direction (872 forward and 854 backward with seed 7), the generated 10-kb set a handful (4 and 19); generated sets
without heterozygosity and the tail-run reads give none.
"""
import pytest

from rel_anchor_inputs import load_probe, standin_reads


@pytest.fixture(scope="module")
def probe():
    return load_probe()


def test_anchor_cells_equal_eff_lookups(harness, probe):
    rows = standin_reads(harness, probe)
    fw, bw = sum(r[4] for r in rows), sum(r[5] for r in rows)
    print("reads with M > 0: %d; cp_dh_ratio look-ups on a stand-in: %d forward, %d backward, in %d reads"
          % (len(rows), fw, bw, sum(1 for r in rows if r[4] or r[5])))
    assert len(rows) >= 200
    assert fw >= 1 and bw >= 1

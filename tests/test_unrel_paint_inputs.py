"""The inputs of tests/test_gpu_unrel_commit.py and tests/test_gpu_paint.py reach the paths those tests are about.  CPU.

Counted on the oracle's stage records, so that the GPU tests cannot pass on inputs that miss
  - the clash path of k_classify_unrel_grp's commit: two index-adjacent non-fixed intervals within four positions of each
    other in the update order (the slots of one round),
  - its set-change path: a reliable non-fixed interval that ends as H or D (it joins the reliable-H / reliable-D set),
  - the K = 8 class of that kernel (N > 256) and k_paint_labels' fallback (more than 511 intervals),
  - 16-byte pieces of the label buffer that hold three or more interval ends, at every alignment of a read's first label.
"""
import numpy as np

from unrel_paint_inputs import K, H_CLS, D_CLS, inputs, fixed, update_order


def test_inputs_reach_the_paths(built):
    seqs, profs, recs = inputs()
    assert len(recs) == 1250
    clash = setchange = big = fallback = pieces3 = 0
    aligns = set()
    off = 0                                                # the read's first label in the batch's label buffer
    for s, rec in zip(seqs, recs):
        io, call = rec["io"], rec["call"]
        N = len(io)
        order = update_order(io)
        hit = False
        for d in (1, 2, 3):
            hit = hit or bool(np.any(np.abs(order[d:] - order[:-d]) == 1))
        clash += hit
        nf = ~fixed(io)
        setchange += bool(np.any(nf & (io["is_rel"] != 0) & ((call["asgn"] == H_CLS) | (call["asgn"] == D_CLS))))
        big += N > 256
        fallback += N > 511
        ends = off + K - 1 + call["e"][:-1].astype(np.int64)     # the first label of the interval behind each end
        inside = ends[ends % 16 != 0] // 16                       # (an end on a piece's first byte changes nothing inside a piece)
        if len(inside):
            pieces3 += int((np.unique(inside, return_counts=True)[1] >= 3).sum())
        aligns.add(off % 16)
        off += len(s)
    print("clash-path reads %d, set-change reads %d, N > 256: %d, N > 511: %d, pieces with >= 3 ends %d, alignments %d"
          % (clash, setchange, big, fallback, pieces3, len(aligns)))
    assert clash >= 500
    assert setchange >= 40
    assert big >= 30
    assert fallback >= 10
    assert pieces3 >= 1000
    assert len(aligns) == 16

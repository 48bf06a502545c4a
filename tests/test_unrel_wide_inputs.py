"""The inputs of tests/test_gpu_unrel_wide_rounds.py reach what k_classify_unrel_grp can get wrong with four lanes per
slot: eight slots per round for N <= 256, sixteen above, a lane of a slot looking at two (four) earlier slots.  CPU.

Counted on the oracle's stage records (tests/unrel_wide_inputs.py: `wide_paths`), at least once each:
  - 0, 1, 7, 8, 9, 15, 16 and 17 non-fixed intervals in the main size class: no round, a round of one slot, one slot
    short of one and of two rounds, exactly one and two, and one slot into the next;
  - a read of more than 256 intervals whose number of non-fixed ones is no multiple of sixteen, and one with fewer than
    sixteen;
  - index neighbours 1 ... 7 positions apart in the update order, the one the first sweep takes first changing to or
    from H / D: the clash a lane sees at its first look (distance 1-4, slot j against a slot up to four in front) and at
    its second (5-7, and 4 where the earlier slot's number is the lane's role);
  - a reliable non-fixed interval that joins the H or the D set at the first, at a middle and at the last slot of a
    round of the first sweep;
  - more than 64 non-fixed intervals: a second sweep of more than one window, in both size classes;
  - a second sweep with a dirty position in the second half of a window of twice the round's positions.
The oracle accepts every read (`inputs` computes all of them; none is left out).
"""
import collections

from unrel_wide_inputs import inputs, wide_paths


def test_inputs_reach_the_wide_round_paths(built):
    seqs, profs, recs = inputs()
    assert len(seqs) == len(profs) == len(recs) == 1254 + 11        # (an odd number: the last wave of the main class holds one read)
    tot = collections.Counter()
    for rec in recs:
        tot.update(wide_paths(rec))
    print(sorted(tot.items()))
    for n in (0, 1, 7, 8, 9, 15, 16, 17):
        assert tot["nnf_%d" % n] >= 1, n
    for path in ("big_ragged", "big_few", "small_two_windows", "big_two_windows", "setc_first", "setc_middle", "setc_last",
                 "dirty_second_half"):
        assert tot[path] >= 1, path
    for d in range(1, 8):
        assert tot["near_%d" % d] >= 10, d

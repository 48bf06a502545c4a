"""The inputs of tests/test_gpu_unrel_round_loads.py reach what a round of k_classify_unrel_grp can get wrong once its
loads are issued together at the top and its parameters live outside the loop.  CPU.

Counted on the oracle's stage records (tests/unrel_round_inputs.py: `round_paths`), at least once each:
  - an update with no reliable H and no reliable D interval on either side (every estimate is its class's coverage, dcov
    the diploid one), and among those one where a class has no term at all on either side: the Poisson fallback, which
    now takes logfact of the two counts from the loads of the E term;
  - an update whose estimate falls back to the other class's neighbours;
  - a slot that leaves by max(cb,ce) >= REPEAT (it forms no address);
  - a sweep whose last round has fewer positions left than slots, with four slots (N <= 256) and with eight;
  - reads with no non-fixed interval, reads with N = 1;
  - index neighbours next to each other in the update order, the first of them changing to or from H / D: the round
    ends at slot 1 and the next one starts there.
The state-dependent ones are counted on the first update of the first sweep, the only one whose state the records hold;
"no round ends early" is decided from the records alone (no reliable non-fixed interval, no two index neighbours within
a round of each other).
"""
import collections

from unrel_round_inputs import inputs, round_paths


def test_inputs_reach_the_round_paths(built):
    seqs, profs, recs = inputs()
    assert len(recs) == 1254
    tot = collections.Counter()
    for rec in recs:
        tot.update(round_paths(rec))
    print(dict(tot))
    for path in ("no_rel", "poisson", "other_class", "repeat_exit", "short4", "short8", "all_fixed", "n1", "clash1"):
        assert tot[path] >= 1, path
    assert tot["short8"] >= 2 and tot["poisson"] >= 10 and tot["clash1"] >= 100

"""The main class of k_classify_rel_grp as it streams a read's interval records from global memory, keeps the transition
matrix in registers and carries the anchors' (end_pos, end_cnt) pairs in the DP cells (kernels.hip: rel_grp_lds<MAXM,8>,
rel_rec, rel_grp_pass with LD = 4), against the oracle.  `-m gpu`.

Compared as in tests/test_gpu_rel_grp_lanes.py, for every read of every batch, once as shipped and once with
CLASSPRO_COMPACT_REL=0: the forward and backward assignments, riv["asgn"] and iv["asgn"] after STAGE_CLASS_REL, and the label
bytes of `classify`.  Integers and bytes: equal or not.

  * anchors on a stand-in: the reads in which the CPU probe (tests/test_rel_anchor_cells.py) counts cp_dh_ratio look-ups
    that land on a stand-in, in either direction -- the only place where carried pairs and a look-up through `eff` differ;
  * block edges: a block is BLOCK_WAVES waves of 8 reads; batches of one block less a read, one block, one block and a
    read, two blocks and a read (a block's last waves then hold one read or none);
  * both ends of the stream: reads with M = 0, 1, 2 and 3, two of each, side by side in one wave (the record fetched one
    step ahead at the first and the last step of both directions);
  * the repeated pass: a batch in which some waves run the pass twice, so the stream starts over from the first record.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 40
HC, DC = 20, 40
WAVE_READS = 8
BLOCK_WAVES = 2            # REL_SMALL_WPB of kernels.hip
MAIN_MAXM = 112            # REL_SMALL_MAXM


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


class RefReads:
    """Reads with the oracle's per-read results, each computed once and kept."""

    def __init__(self, seqs, profs):
        from oracle.oracle import Oracle
        self.seqs, self.profs = seqs, profs
        self.O = Oracle(K, 20000, HC, DC)
        self._rel, self._full = {}, {}

    def rel(self, j):
        """(intvl, rintvl) of read j after find_rel_intvl: M = len(rintvl)."""
        if j not in self._rel:
            l, r = self.O.seq_context(self.seqs[j])
            iv = self.O.find_wall(self.profs[j], l, r)
            self._rel[j] = self.O.find_rel_intvl(iv, self.profs[j], l, r)
        return self._rel[j]

    def M(self, j):
        return len(self.rel(j)[1])

    def full(self, j):
        if j not in self._full:
            iv, riv = self.rel(j)
            ro, io, fw, bw = self.O.classify_rel(riv, iv, len(self.profs[j]))
            self._full[j] = dict(M=len(riv), fw=fw, bw=bw, riv=ro["asgn"].copy(), iv=io["asgn"].copy(),
                                 lab=self.O.classify_read(self.seqs[j], self.profs[j]))
        return self._full[j]


def ref_set(**kw):
    from classpro_amd import synth
    ds = synth.make_dataset(**kw)
    return RefReads(ds["seqs"], ds["profiles"])


@pytest.fixture(scope="module")
def set_long(built):          # its first reads: M 8-70
    return ref_set(genome_len=200000, cov=40, read_len=10000, seed=5)


@pytest.fixture(scope="module")
def set_short(built):         # its first 300 reads: M 0-9, most of them M <= 2
    return ref_set(genome_len=60000, cov=40, read_len=600, min_len=60, seed=4)


@pytest.fixture(scope="module")
def set_repeat(built):        # no heterozygosity: most forward passes end with D and no H
    return ref_set(genome_len=60000, cov=40, read_len=6000, seed=3, het=0.0)


def check_batches(monkeypatch, batches):
    """batches: lists of (RefReads, read index).  Every read of every batch, with compact and with full records."""
    from classpro_amd.api import Classifier, Batch, STAGE_CLASS_REL
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("CLASSPRO_COMPACT_REL", raising=False)
        else:
            monkeypatch.setenv("CLASSPRO_COMPACT_REL", env)
        clf = Classifier(K, 20000, HC, DC)
        for nb, batch in enumerate(batches):
            want = [S.full(j) for S, j in batch]
            b = Batch.from_reads([S.seqs[j] for S, j in batch], [S.profs[j] for S, j in batch])
            clf.run(b, STAGE_CLASS_REL)
            clf.check()
            got = clf.intervals(b)
            asg = clf.rel_asgn(b)
            assert len(got) == len(asg) == len(want)
            for r, ((iv, riv), (fw, bw), w) in enumerate(zip(got, asg, want)):
                where = "batch %d read %d (M = %d), CLASSPRO_COMPACT_REL=%s" % (nb, r, w["M"], env)
                assert len(riv) == w["M"], where
                assert np.array_equal(fw, w["fw"]) and np.array_equal(bw, w["bw"]), where
                assert np.array_equal(riv["asgn"], w["riv"]) and np.array_equal(iv["asgn"], w["iv"]), where
            lab = clf.classify(b)
            so = b.seq_off_h
            for r, w in enumerate(want):
                assert lab[so[r]:so[r + 1]].tobytes() == w["lab"], "labels of batch %d read %d (M = %d), CLASSPRO_COMPACT_REL=%s" % (nb, r, w["M"], env)
        clf.close()
    monkeypatch.delenv("CLASSPRO_COMPACT_REL", raising=False)


def test_anchors_on_stand_ins(torch_dev, harness, monkeypatch):
    """The reads of the CPU test with look-ups on a stand-in, those of the main class (M <= 112), in one batch."""
    from rel_anchor_inputs import load_probe, standin_reads
    rows = [r for r in standin_reads(harness, load_probe()) if (r[4] or r[5]) and r[3] <= MAIN_MAXM]
    fw, bw = sum(r[4] for r in rows), sum(r[5] for r in rows)
    print("%d reads, look-ups on a stand-in: %d forward, %d backward" % (len(rows), fw, bw))
    assert fw >= 1 and bw >= 1
    S = RefReads([r[1] for r in rows], [r[2] for r in rows])
    for j, r in enumerate(rows):
        assert S.M(j) == r[3], r[0]                          # the oracle's reliable intervals are the probe's
    check_batches(monkeypatch, [[(S, j) for j in range(len(rows))]])


@pytest.mark.parametrize("n", [WAVE_READS * BLOCK_WAVES - 1, WAVE_READS * BLOCK_WAVES, WAVE_READS * BLOCK_WAVES + 1,
                               2 * WAVE_READS * BLOCK_WAVES + 1])
def test_block_edges(torch_dev, set_long, monkeypatch, n):
    Ms = [set_long.M(j) for j in range(n)]
    assert 8 <= min(Ms) and max(Ms) <= MAIN_MAXM
    check_batches(monkeypatch, [[(set_long, j) for j in range(n)]])


def test_stream_ends(torch_dev, set_short, monkeypatch):
    """M = 0, 1, 2, 3, two reads of each, in one wave."""
    Ms = [set_short.M(j) for j in range(300)]
    pick = [j for m in (0, 1, 2, 3) for j in [k for k in range(300) if Ms[k] == m][:2]]
    assert sorted(Ms[j] for j in pick) == [0, 0, 1, 1, 2, 2, 3, 3]
    check_batches(monkeypatch, [pick_order(set_short, pick), pick_order(set_short, pick[::-1])])


def pick_order(S, idx):
    return [(S, j) for j in idx]


def test_repeated_pass(torch_dev, set_repeat, monkeypatch):
    """40 reads (five waves): in some waves a read asks for the pass again (its forward assignment has D and no H), and
    the wave repeats it for all its lanes."""
    n = 40
    ends_d = 0
    for j in range(n):
        fw = set_repeat.full(j)["fw"]
        ends_d += int(len(fw) > 0 and (fw == 3).any() and not (fw == 2).any())
    assert ends_d >= WAVE_READS, ends_d
    assert max(set_repeat.M(j) for j in range(n)) <= MAIN_MAXM
    check_batches(monkeypatch, [[(set_repeat, j) for j in range(n)]])

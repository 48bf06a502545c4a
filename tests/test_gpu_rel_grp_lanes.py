"""k_classify_rel_grp with eight reads per wave and four lanes per direction (kernels.hip: rel_grp_pass, LD = 4) against
the oracle, on the shapes at which that lane layout can go wrong.  `-m gpu`.

Compared, for every read of every batch, once as shipped and once with CLASSPRO_COMPACT_REL=0: the forward and backward
assignments, riv["asgn"] and iv["asgn"] after STAGE_CLASS_REL (the stage API: the COMPACT = 0 kernel), and the label bytes
of `classify` (the whole-path call: the COMPACT = 1 kernel unless the variable says otherwise).  Everything is integers and
bytes: equal or not.

  * partly filled waves, reads of different M in one wave: batches of 1, 7, 8, 9 and 17 reads (a wave holds 8: the second
    wave of a 9-read batch holds one read, the third of a 17-read batch too) from the heads of two sets, one with M 8-70
    and reads whose two passes disagree, one of short reads with M = 0, 1, 2, ... side by side;
  * the class edge: every read with 97 <= M <= 113 of a 24-kb set (M = 112 is the last interval count of the main class,
    M = 113 belongs to the one-read-per-wave class) plus the eight reads of fewest intervals (M 48-76), in one batch;
  * the repeated pass: reads that end the forward pass with D and no H (cp_rel_post1 asks for the pass again, and a wave
    repeats it for all its lanes when any of its sixteen (read, direction) pairs asks), in batches of 8 and of 150.
    (A -DCP_PROF_WALK build counts the pairs that repeat on these 150 reads: profiles/rel_grp_lanes_ab.txt.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 40
HC, DC = 20, 40
WAVE_READS = 8


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


class RefSet:
    """A generated read set with the oracle's per-read results, each computed once and kept."""

    def __init__(self, **kw):
        from classpro_amd import synth
        from oracle.oracle import Oracle
        ds = synth.make_dataset(**kw)
        self.seqs, self.profs = ds["seqs"], ds["profiles"]
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

    def differs(self, j):
        f = self.full(j)
        return not np.array_equal(f["fw"], f["bw"])


@pytest.fixture(scope="module")
def set_long(built):          # its first 150 reads: M 8-70, some with fw != bw
    return RefSet(genome_len=200000, cov=40, read_len=10000, seed=5)


@pytest.fixture(scope="module")
def set_short(built):         # its first 300 reads: M 0-9, most of them M <= 2
    return RefSet(genome_len=60000, cov=40, read_len=600, min_len=60, seed=4)


@pytest.fixture(scope="module")
def set_edge(built):          # 24-kb reads, M 48-251
    return RefSet(genome_len=300000, cov=40, read_len=24000, seed=11, het=0.004, err_sub=0.002)


@pytest.fixture(scope="module")
def set_repeat(built):        # no heterozygosity: most forward passes end with D and no H
    return RefSet(genome_len=60000, cov=40, read_len=6000, seed=3, het=0.0)


def check_batches(monkeypatch, batches):
    """batches: lists of (RefSet, read index).  Every read of every batch, with compact and with full records."""
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


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_partly_filled_waves_and_mixed_m(torch_dev, set_long, set_short, monkeypatch, n):
    """n reads from the head of each set, and a mixed batch that holds a read with M = 0, one with M = 1 and one whose
    forward and backward assignments differ next to reads from both heads (n = 1: each of the three alone)."""
    Ms = [set_short.M(j) for j in range(300)]
    m0, m1 = Ms.index(0), Ms.index(1)
    fb = next(j for j in range(150) if set_long.differs(j))
    special = [(set_short, m0), (set_short, m1), (set_long, fb)]
    assert set_short.full(m0)["M"] == 0 and set_short.full(m1)["M"] == 1 and set_long.differs(fb)
    assert 8 <= min(set_long.M(j) for j in range(17)) and max(set_long.M(j) for j in range(150)) <= 112
    batches = [[(set_long, j) for j in range(n)], [(set_short, j) for j in range(n)]]
    if n < len(special):
        batches += [[s] for s in special]
    else:
        fill = [x for j in range(n) for x in ((set_long, j), (set_short, j)) if x not in special]
        mixed = special + fill[:n - len(special)]
        assert len(mixed) == n and len(set(mixed)) == n
        Mm = [S.M(j) for S, j in mixed]
        assert 0 in Mm and 1 in Mm and any(S.differs(j) for S, j in mixed) and max(Mm) >= 8
        batches.append(mixed[::-1])
    # the short set alone already puts M = 0 beside live reads once a wave is full
    if n >= 7:
        assert 0 in Ms[:n] and max(Ms[:n]) > 0
    check_batches(monkeypatch, batches)


def test_class_edge(torch_dev, set_edge, monkeypatch):
    """Reads of the main class up to its last interval count beside reads the next class owns: the waves of either kernel
    hold lanes whose read belongs to the other."""
    n = len(set_edge.seqs)
    Ms = [set_edge.M(j) for j in range(n)]
    edge = [j for j in range(n) if 97 <= Ms[j] <= 113]
    small = sorted(range(n), key=lambda j: (Ms[j], j))[:8]    # the eight reads of fewest intervals (two of them below 60)
    assert 112 in [Ms[j] for j in edge] and 113 in [Ms[j] for j in edge]
    assert len(edge) >= 50 and min(Ms[j] for j in small) < 60 and max(Ms[j] for j in small) < 97
    # small reads spread among the large ones (the kernels take the reads by decreasing M; the batch order is the caller's)
    order = sorted(edge + small)
    check_batches(monkeypatch, [[(set_edge, j) for j in order]])


def test_repeated_pass(torch_dev, set_repeat, monkeypatch):
    """cp_rel_post1 repeats the pass for reads whose forward assignment has D and no H: in batches of 8 (one wave each,
    the last partly filled) and of 150 (19 waves)."""
    n = 150
    ends_d = 0
    for j in range(n):
        fw = set_repeat.full(j)["fw"]
        ends_d += int(len(fw) > 0 and (fw == 3).any() and not (fw == 2).any())
    assert ends_d >= n // 2, ends_d
    batches = [[(set_repeat, j) for j in range(o, min(o + WAVE_READS, n))] for o in range(0, n, WAVE_READS)]
    batches.append([(set_repeat, j) for j in range(n)])
    check_batches(monkeypatch, batches)

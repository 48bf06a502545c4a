"""The HIP path (through the C ABI) at both ends of the count-threshold table, against the REFERENCE's own text.  `-m gpu`.

tests/golden/thres.npz: the reference's calc_init_thres(NULL) at (H,D) = (93,187), CMAX = 255 -- the last column of
cthres[t][l][cout][s][e], the full width of the 256-wide petab rows and of the |ce-cb| <= 255 bound of the logp_trans
table -- and CMAX for every D (tests/test_oracle_thres.py).  tests/golden/cov_edges.npz (oracle/gen_golden.py): four
parameter sets, (K 40, H 93, D 187; CMAX 255), (40, 64, 128; 184), (40, 2, 5; 16), (21, 1, 2; 9) -- at the low end almost
every count is >= CMAX -- with the tables from the reference and, per read, what wall.npz and labels.npz hold together:
the find_wall + find_rel_intvl records with their doubles, status, labels and interval classes.  Reads per set:
  (a) 12 synth.make_dataset reads of <= 6000 bases at that coverage (genome 20 000 / 120 000, het 0.004, seed 7),
      14 adversarial_reads, 10 tail_run_reads, 30 tiny reads with jumping counts around the set's own levels;
  (b) threshold-edge reads: for 12 (t, l) -- HP l = 1, 2, 7, 13, 20; DS 2, 4, 7, 10; TS 2, 3, 6; a DS / TS context wins over HP
      only with l >= 2 -- a random read of 700 k-mers with one planted run; the profile is flat at cout on one side of the
      position where find_wall picks that context and at cin on the other; cin at the reference's INIT and FINAL entries
      and at each +- 1; SELF as a drop four k-mers before the read's end (the read's end closes the error interval:
      elsewhere a lone drop has no partner), OTHERS as a gain in the middle; cout in {3, 5, CMAX-2, CMAX-1, CMAX, CMAX+1}
      (l = 7 with cout 3 and 5 are the entries exact arithmetic cannot decide, tests/test_first_principles.py).
Conditions on the file (cov_edges.py; checked when it was written and again here), with the shares achieved:
  set (93,187): 99.9 % of reads return;  E 10.9  H 13.2  D  7.5  R 68.4 % of the generator reads' labelled bases;  69 % of 72 (t,l,cout)
  set (64,128): 99.5 %;                  E  8.4  H 12.7  D  9.7  R 69.3 %;                                          78 %
  set (2,5):    99.7 %;                  E  5.0  H 11.2  D 49.1  R 34.7 %;                                          88 %
  set (1,2):   100.0 %;                  E  1.3  H 11.4  D 65.1  R 22.2 %;                                          88 %
(floors: 90 % return; 3 % per class, 1 % at (1,2); half of the (t,l,cout) end differently -- other boundaries, reliability,
classes, or other error probabilities ever computed -- between cin one below and one above a threshold of theirs; a third
of the triples, cout >= CMAX, have no table entry at all).  The oracle equals the reference on every one of these reads.
Bar: bit-exact, the three doubles of a record included.
"""
import numpy as np
import pytest

import cov_edges
from conftest import load_golden
from test_gpu_reference import DBL_FIELDS, assert_aborts, classifier_for, reads_of_set

PAIRS = [(93, 187), (1, 2), (2, 5), (12, 25), (19, 38), (20, 40), (30, 57), (30, 60), (50, 99), (64, 128)]
SETS = [(40, 20000, 93, 187), (40, 20000, 64, 128), (40, 20000, 2, 5), (21, 20000, 1, 2)]


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


@pytest.fixture(scope="module")
def edges():
    """cov_edges.npz with every array decoded once (an NpzFile decodes an array each time it is indexed)."""
    g = load_golden("cov_edges.npz")
    return {k: g[k] for k in g.files}


def test_cov_edges_file_meets_its_conditions(edges):
    """No GPU: the parameter sets, the reference's tables in the file, and the three conditions on the reads."""
    from oracle.oracle import INTVL_DTYPE
    g, th = edges, load_golden("thres.npz")
    assert [tuple(int(x) for x in p) for p in g["psets"]] == [p + (0,) for p in SETS]      # (K, -r, H, D, default error model)
    for si, (K, rl, h, d) in enumerate(SETS):
        cmax = int(th["cmax_of_d"][d])
        assert g["cmax"][si] == cmax and np.array_equal(g["cthres"][si][:, :, :cmax], th["cthres"][:, :, :cmax])
        assert not g["cthres"][si][:, :, cmax:].any() and np.array_equal(g["pe"][si].view(np.uint64), th["pe_bits"])
        ret, cls, differ, ntri = cov_edges.edge_shares(g, si, INTVL_DTYPE)
        print("set (%d,%d): %.1f %% return; E %.1f H %.1f D %.1f R %.1f %%; %.0f %% of %d (t,l,cout) differ across a threshold"
              % (h, d, 100 * ret, 100 * cls["E"], 100 * cls["H"], 100 * cls["D"], 100 * cls["R"], 100 * differ, ntri))
        assert ret >= cov_edges.MIN_RETURN
        assert min(cls.values()) >= cov_edges.class_floor(h, d), cls
        assert differ >= cov_edges.MIN_DIFFER and ntri == 72
        em = g["edge_meta"][g["edge_row"][(g["set"] == si) & (g["kind"] == cov_edges.KIND_EDGE)]]
        assert set(int(c) for c in em[:, 2]) == {3, 5, cmax - 2, cmax - 1, cmax, cmax + 1}
        for t in (0, 1):                                  # the near-tie entries: l = 7 (pe = 0.1) with cout 3 and 5
            assert {3, 5} <= set(int(c) for c in em[(em[:, 0] == t) & (em[:, 1] == 7)][:, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("hd", PAIRS)
def test_exported_table_is_the_references(torch_dev, hd):
    from classpro_amd.api import Classifier
    th = load_golden("thres.npz")
    h, d = hd
    cmax = int(th["cmax_of_d"][d])
    clf = Classifier(40, 20000, h, d)
    ex = clf.export()
    clf.close()
    assert ex["cmax"] == cmax == ex["cov"][1]
    assert np.array_equal(ex["cthres"][:, :, :cmax], th["cthres"][:, :, :cmax])
    assert np.array_equal(ex["pe"].view(np.uint64), th["pe_bits"])
    assert np.array([ex["hc_erate"]]).view(np.uint64)[0] == th["hc_erate_bits"][0]


@pytest.mark.gpu
def test_too_high_coverage_raises(torch_dev):
    from classpro_amd.api import Classifier
    from classpro_amd._lib import ClassProError, CP_ERCOV
    assert load_golden("thres.npz")["cmax_of_d"][188] == -1          # the reference's exit(1)
    with pytest.raises(ClassProError) as ei:
        Classifier(40, 20000, 94, 188)
    assert ei.value.code == CP_ERCOV


def check_wall_and_rel(clf, g, idx, seqs, profs):
    """STAGE_WALL and STAGE_REL records of the reads the reference returns on (all of them in one batch) == the reference's;
    the reads it aborts on raise CP_EOVERFLOW, each on its own."""
    from classpro_amd.api import Batch, STAGE_WALL, STAGE_REL
    from oracle.oracle import INTVL_DTYPE
    st = g["status"][idx]
    assert_aborts(clf, [s for s, t in zip(seqs, st) if t == 1], [p for p, t in zip(profs, st) if t == 1])
    keep = [k for k, t in enumerate(st) if t == 0]
    b = Batch.from_reads([seqs[k] for k in keep], [profs[k] for k in keep])
    io, ro = g["intvl_off"], g["rintvl_off"]
    iv_all, rv_all = g["intvl"].view(INTVL_DTYPE), g["rintvl"].view(INTVL_DTYPE)
    clf.run(b, STAGE_WALL)                                  # find_wall alone: Intvl[N] before find_rel_intvl touches it
    clf.check()
    for k, (iv, _) in zip(keep, clf.intervals(b)):
        want = iv_all[io[idx[k]]:io[idx[k] + 1]]
        assert len(iv) == len(want), idx[k]
        for f in ("b", "e", "cb", "ce"):
            assert np.array_equal(iv[f], want[f]), (idx[k], f)
        for f in DBL_FIELDS:
            assert np.array_equal(iv[f].view(np.uint64), want[f].view(np.uint64)), (idx[k], f)
    clf.run(b, STAGE_REL)                                   # + find_rel_intvl / correct_wall_cnt
    clf.check()
    n_rel = 0
    for k, (iv, rv) in zip(keep, clf.intervals(b)):
        want, wantr = iv_all[io[idx[k]]:io[idx[k] + 1]], rv_all[ro[idx[k]]:ro[idx[k] + 1]]
        assert len(iv) == len(want) and len(rv) == len(wantr), idx[k]
        for f in ("b", "e", "cb", "ce", "is_rel"):
            assert np.array_equal(iv[f], want[f]), (idx[k], f)
        rel = want["is_rel"] != 0                           # corrected counts are defined for the reliable intervals
        for f in ("ccb", "cce"):
            assert np.array_equal(iv[f][rel], want[f][rel]), (idx[k], f)
        for f in ("b", "e", "cb", "ce", "ccb", "cce", "is_rel"):
            assert np.array_equal(rv[f], wantr[f]), (idx[k], f)
        for f in DBL_FIELDS:
            assert np.array_equal(iv[f].view(np.uint64), want[f].view(np.uint64)), (idx[k], f)
            assert np.array_equal(rv[f].view(np.uint64), wantr[f].view(np.uint64)), (idx[k], f)
        n_rel += len(rv)
    return n_rel


def check_labels(clf, g, idx, seqs, profs, reverse=True):
    """Labels and final interval classes == the reference's; the batch in reversed order gives the same bytes."""
    from classpro_amd.api import Batch, STAGE_CLASS_ALL
    st = g["status"][idx]
    keep = [k for k, t in enumerate(st) if t == 0]
    b = Batch.from_reads([seqs[k] for k in keep], [profs[k] for k in keep])
    lo, ao = g["labels_off"], g["asgn_off"]
    got = clf.classify(b)
    off = np.concatenate([[0], np.cumsum([len(seqs[k]) for k in keep])])
    for j, k in enumerate(keep):                            # per read, so that a failure names the read
        assert got[off[j]:off[j + 1]].tobytes() == g["labels"][lo[idx[k]]:lo[idx[k] + 1]].tobytes(), idx[k]
    clf.run(b, STAGE_CLASS_ALL)
    clf.check()
    for k, (iv, _) in zip(keep, clf.intervals(b)):
        assert np.array_equal(iv["asgn"], g["asgn"][ao[idx[k]]:ao[idx[k] + 1]]), idx[k]
    if reverse:
        rev = keep[::-1]
        b2 = Batch.from_reads([seqs[k] for k in rev], [profs[k] for k in rev])
        assert clf.classify(b2).tobytes() == b"".join(g["labels"][lo[idx[k]]:lo[idx[k] + 1]].tobytes() for k in rev)


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(4))
def test_wall_and_rel_stage_at_the_coverage_extremes(torch_dev, edges, si):
    g = edges
    clf, K = classifier_for(g, si)
    idx, seqs, profs = reads_of_set(g, si)
    assert check_wall_and_rel(clf, g, idx, seqs, profs) > 100
    clf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(4))
def test_labels_at_the_coverage_extremes(torch_dev, edges, si):
    g = edges
    clf, K = classifier_for(g, si)
    idx, seqs, profs = reads_of_set(g, si)
    check_labels(clf, g, idx, seqs, profs)
    clf.close()


@pytest.mark.gpu
def test_labels_without_tables_at_the_wide_end(torch_dev, edges, monkeypatch):
    """CMAX = 255 with CLASSPRO_TABLES=0: every petab / logp_trans value computed on the spot.  The same reference labels,
    so the look-ups and the direct path agree where the tables are at their widest."""
    from classpro_amd.api import Classifier
    g = edges
    monkeypatch.setenv("CLASSPRO_TABLES", "0")
    monkeypatch.delenv("CLASSPRO_SKELLAM_TABLE_MB", raising=False)
    K, rl, h, d = SETS[0]
    clf = Classifier(K, rl, h, d)
    tb = clf.tables()
    assert tb["skel"] == 0 and tb["uerr"] == 0 and tb["petab"] == 0, tb
    idx, seqs, profs = reads_of_set(g, 0)
    check_labels(clf, g, idx, seqs, profs, reverse=False)
    clf.close()
    monkeypatch.delenv("CLASSPRO_TABLES")
    clf = Classifier(K, rl, h, d)                           # (the default: with tables, as the tests above)
    tb = clf.tables()
    clf.close()
    assert tb["skel"] > 0 and tb["uerr"] > 0 and tb["petab"] > 0, tb

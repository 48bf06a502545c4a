"""The count-threshold table cthres[t][l][cout][INIT|FINAL][SELF|OTHERS] against the REFERENCE's own calc_init_thres
(wall.c:167-243), default error model.

tests/golden/thres.npz is what oracle/_ref/ref_thres wrote (oracle/ref_thres.c + the reference's wall.c without its GSL
include and polynomialfit, oracle/Makefile; calc_init_thres(NULL) never reaches the fit): the whole table at (H,D) =
(93,187), where CMAX = 255 is the last value before the reference's "Too high REPEAT coverage"; pe[3][21] and HC_ERATE by
their bit patterns; and, read from the executable for every D in 1..188, CMAX (-1: exit(1)).  An entry depends on
(pe[t][l], cout) alone, so that one table holds the table of every smaller CMAX as its prefix cout < CMAX
(oracle/gen_golden.py checked this on the reference for every D).

Checked here without a GPU: the oracle's restatement and the product's host fill (cp_host_fill_params through the host
harness) equal it, whole at (93,187) -- 3*21*256*2*2 = 64 512 bytes, 0 differences -- and as the prefix at nine smaller
coverage pairs, and both refuse (94,188).  With oracle/_ref present, Ref.thres reproduces the golden.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from oracle.oracle import Oracle, Ref, RefExit, ref_thres_available

SHAPE = (3, 21, 256, 2, 2)
PAIRS = [(93, 187), (1, 2), (2, 5), (12, 25), (19, 38), (20, 40), (30, 57), (30, 60), (50, 99), (64, 128)]

needs_ref = pytest.mark.skipif(not ref_thres_available(), reason="oracle/_ref/ref_thres not built (no reference tree)")


@pytest.fixture(scope="module")
def golden():
    g = load_golden("thres.npz")
    assert g["cthres"].shape == SHAPE and g["cthres"].dtype == np.uint8
    assert tuple(g["hd"]) == (93, 187) and int(g["cmax"]) == 255
    return g


def expect(golden, d):
    """(cmax, table) the reference builds at diploid coverage d: the golden's prefix cout < cmax, zero elsewhere."""
    cmax = int(golden["cmax_of_d"][d])
    assert 0 < cmax <= 255
    tab = np.zeros(SHAPE, np.uint8)
    tab[:, :, :cmax] = golden["cthres"][:, :, :cmax]
    return cmax, tab


def test_golden_is_a_whole_reference_table(golden):
    """What the other tests lean on: the file holds a whole table -- rows l = 1..lmax[t] and columns cout = 1..254 set, the
    rest zero -- D = 187 is the last coverage with a table, and CMAX = D + floor(5 sqrt(D)) for every D (util.c:9-11,
    ClassPro.c:547)."""
    ct, lmax = golden["cthres"], golden["lmax"]
    assert list(lmax) == [20, 10, 6]
    for t in range(3):
        assert not ct[t, 0].any() and not ct[t, lmax[t] + 1:].any()
        # a SELF entry is a cin >= 1 or cout itself: P(X > 0) = 1 - (1-pe)^cout >= pe >= 0.004 is above both thresholds
        assert (ct[t, 1:lmax[t] + 1, 1:255, :, 0] >= 1).all()
    assert not ct[:, :, 0].any() and not ct[:, :, 255].any()             # cout = 0 and cout = CMAX are never set
    cm = golden["cmax_of_d"]
    assert cm[188] == -1 and cm[187] == 255
    assert all(int(cm[d]) == d + int(np.sqrt(d) * 5) for d in range(1, 188))
    pe = golden["pe_bits"].view(np.float64)
    assert golden["hc_erate_bits"].view(np.float64)[0] == pe[0][1] == 0.004


@pytest.mark.parametrize("hd", PAIRS)
def test_oracle_table_is_the_references(built, golden, hd):
    h, d = hd
    cmax, want = expect(golden, d)
    O = Oracle(40, 20000, h, d)
    cov, _, ocmax, hc = O.scalars()
    assert ocmax == cmax == cov[1]
    got = O.cthres()
    assert np.array_equal(got[:, :, :cmax], want[:, :, :cmax])
    assert int((got != want).sum()) == 0                                 # ... and nothing beyond the prefix
    assert np.array_equal(O.pe().view(np.uint64), golden["pe_bits"])
    assert np.array([hc]).view(np.uint64)[0] == golden["hc_erate_bits"][0]
    assert list(O.lmax()) == list(golden["lmax"])


@pytest.mark.parametrize("hd", PAIRS)
def test_product_host_fill_is_the_references(harness, golden, hd):
    h, d = hd
    cmax, want = expect(golden, d)
    P = harness.hh_params_new(40, 20000, h, d)
    assert P
    try:
        got = np.ctypeslib.as_array(C.cast(harness.hh_params_cthres(C.c_void_p(P)), C.POINTER(C.c_uint8)), shape=SHAPE).copy()
    finally:
        harness.hh_params_free(C.c_void_p(P))
    assert np.array_equal(got[:, :, :cmax], want[:, :, :cmax])
    assert int((got != want).sum()) == 0


def test_too_high_coverage_is_refused(harness, built, golden):
    """(94,188): REPEAT coverage 256.  The reference exits (golden: -1), the oracle raises, the product returns CP_ERCOV."""
    assert golden["cmax_of_d"][188] == -1
    with pytest.raises(ValueError):
        Oracle(40, 20000, 94, 188)
    assert not harness.hh_params_new(40, 20000, 94, 188)
    assert harness.hh_params_new(40, 20000, 93, 187)                     # the last one that is accepted


@needs_ref
@pytest.mark.parametrize("hd", [(93, 187), (64, 128), (20, 40), (2, 5), (1, 2)])
def test_ref_thres_reproduces_the_golden(golden, hd):
    h, d = hd
    cmax, want = expect(golden, d)
    t = Ref.thres(h, d)
    assert t["cmax"] == cmax and np.array_equal(t["cthres"], want)
    assert np.array_equal(t["pe"].view(np.uint64), golden["pe_bits"]) and list(t["lmax"]) == list(golden["lmax"])
    assert np.array([t["hc_erate"]]).view(np.uint64)[0] == golden["hc_erate_bits"][0]


@needs_ref
def test_ref_thres_cmax_of_every_d(golden):
    """CMAX as the executable reports it, D = 1..188, and the reference's own message at 188."""
    for d in range(1, 188):
        assert Ref.thres(max(1, d // 2), d)["cmax"] == golden["cmax_of_d"][d], d
    with pytest.raises(RefExit) as ei:
        Ref.thres(94, 188)
    assert ei.value.message == "Too high REPEAT coverage (256) > 255"

"""The DP cells of the main class of k_classify_rel_grp in LDS (cp_class.h: cp_rel_cell_off, cp_cell_pack / cp_cell_unpack;
kernels.hip: rel_grp_lds<MAXM,8>).  CPU only, through tests/rel_cell_probe.cpp.

Slot enumeration.  A cell is four 16-byte pieces, each moved by one 128-bit LDS instruction that handles the same piece on
all 64 lanes.  Lane (g, d, s) = (lane / 8, (lane / 4) & 1, lane & 3) writes the cell of its own state and reads the cell of any
state of its own quad (its best predecessor; its own on an "only R reachable" step).  The hardware serves a 128-bit read in
four groups of sixteen lanes over 64 banks of 4 bytes and a 128-bit write in eight groups of eight consecutive lanes over
32 banks; two lanes of a group conflict when their accesses differ in address and share a bank (equal addresses
broadcast).  With 16-byte aligned pieces a bank quadruple is a slot: (offset / 16) mod 16 for reads, mod 8 for writes.
The test enumerates every lane group, for reads every assignment of a state to each lane of one quad (4^4) with each of
the group's other three quads at each of their four states (4^3), and asserts that no group ever has a conflict.  The
layout before this one -- 56-byte cells in (read, direction, buffer, state) order, stride 448 per (read, direction) --
must fail the same check (test_former_layout_has_conflicts: 16-byte accesses at the cells' 8-byte alignment).

Packed-cell round trip.  cp_cell_anc -> four pieces -> cp_cell_anc over the boundary values of every field.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
from conftest import ROOT, build_if_changed

READ_GROUPS_32 = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                  list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
READ_GROUPS = READ_GROUPS_32 + [[l + 32 for l in grp] for grp in READ_GROUPS_32]      # ds_read_b128: 4 x 16 lanes
WRITE_GROUPS = [list(range(8 * k, 8 * k + 8)) for k in range(8)]                      # ds_write_b128: 8 x 8 lanes
READ_BANKS, WRITE_BANKS = 64, 32
MAIN_MAXM = 112            # REL_SMALL_MAXM of kernels.hip
RECORD_BYTES = 6144        # what the kernel's two-wave block is sized by: 2 x 6 144 + 4 096 of libm tables = 16 384


@pytest.fixture(scope="module")
def probe():
    src = os.path.join(ROOT, "tests", "rel_cell_probe.cpp")
    out = os.path.join(ROOT, "tests", "_rel_cell_probe.so")
    csrc = os.path.join(ROOT, "classpro_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    build_if_changed(out, ["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src], deps)
    return C.CDLL(out)


def product_layout(probe):
    """off[g, d, buffer, s, p] of the product (one buffer)."""
    P = probe.rcp_pieces()
    off = np.zeros((8, 2, 1, 4, P), np.int64)
    for g, d, s, p in itertools.product(range(8), range(2), range(4), range(P)):
        off[g, d, 0, s, p] = probe.rcp_cell_off(g, d, s, p)
    return off, 16 * P


def former_layout():
    """56-byte cells, cell[read][direction][buffer][state]: 448 bytes per (read, direction); pieces of 16, 16, 16 and 8 bytes."""
    off = np.zeros((8, 2, 2, 4, 4), np.int64)
    for g, d, b, s, p in itertools.product(range(8), range(2), range(2), range(4), range(4)):
        off[g, d, b, s, p] = (g * 2 + d) * 448 + b * 224 + s * 56 + p * 16
    return off, 56


def conflicts(addr, nbanks):
    """addr[n, lanes]: byte addresses of one lane group's 16-byte accesses, a row per case.  How many rows hold two lanes
    with different addresses on a common bank."""
    addr = addr.astype(np.int16)                           # (a wave's cells lie within 8 KB)
    b = (addr // 4) % nbanks
    dist = (b[:, :, None] - b[:, None, :]) % np.int16(nbanks)
    share = (dist < 4) | (dist > nbanks - 4)
    differ = addr[:, :, None] != addr[:, None, :]
    return int((share & differ).any(axis=(1, 2)).sum())


def lane_gds(lane):
    return lane // 8, (lane // 4) & 1, lane & 3


def read_cases(off, group, buf, piece):
    """Every case of the enumeration for one read group: rows of 16 addresses."""
    quads = sorted({l // 4 for l in group})
    assert len(quads) == 4 and len(group) == 16
    lanes = [l for q in quads for l in range(4 * q, 4 * q + 4)]
    assert sorted(lanes) == sorted(group)
    one = np.array(list(itertools.product(range(4), repeat=4)))          # 4^4 choices for the four lanes of a quad
    others = np.array(list(itertools.product(range(4), repeat=3)))       # a state for each other quad
    rows = []
    for k, q in enumerate(quads):
        pick = np.zeros((len(one), len(others), 4, 4), np.int64)         # [case of q, case of the others, quad, lane of it]
        oq = [x for x in range(4) if x != k]
        pick[:, :, k, :] = one[:, None, :]
        for j, x in enumerate(oq):
            pick[:, :, x, :] = others[None, :, j, None]
        pick = pick.reshape(-1, 4, 4)
        addr = np.zeros_like(pick)
        for x, qq in enumerate(quads):
            g, d = qq // 2, qq & 1
            addr[:, x, :] = off[g, d, buf, :, piece][pick[:, x, :]]
        rows.append(addr.reshape(-1, 16))
    return np.concatenate(rows)


def count_all(off):
    nbuf, npiece = off.shape[2], off.shape[4]
    rd = wr = 0
    for buf in range(nbuf):
        for p in range(npiece):
            for grp in READ_GROUPS:
                rd += conflicts(read_cases(off, grp, buf, p), READ_BANKS)
            for grp in WRITE_GROUPS:
                a = np.array([[off[lane_gds(l)[0], lane_gds(l)[1], buf, lane_gds(l)[2], p] for l in grp]])
                wr += conflicts(a, WRITE_BANKS)
    return rd, wr


def test_lane_groups_cover_the_wave():
    for groups in (READ_GROUPS, WRITE_GROUPS):
        assert sorted(l for grp in groups for l in grp) == list(range(64))


def test_cells_tile_the_record(probe):
    off, cell = product_layout(probe)
    flat = off.reshape(-1)
    assert (flat % 16 == 0).all() and flat.min() == 0
    assert len(set(flat.tolist())) == flat.size                        # no two pieces of any two cells overlap
    assert flat.max() + 16 == probe.rcp_cells_bytes() == flat.size * 16 == 8 * 2 * 4 * cell
    rw = (MAIN_MAXM + 31) // 32
    assert probe.rcp_record_bytes(MAIN_MAXM) == probe.rcp_cells_bytes() + 8 * 2 * MAIN_MAXM + 8 * 2 * rw * 4 == RECORD_BYTES
    # ... and the kernel's record is declared with that size
    src = open(os.path.join(ROOT, "classpro_amd", "csrc", "kernels.hip")).read()
    assert "static_assert(sizeof(rel_grp_lds<REL_SMALL_MAXM,8>) == cp_rel_record_bytes(REL_SMALL_MAXM)" in src
    assert "#define REL_SMALL_MAXM %d " % MAIN_MAXM in src


def test_no_two_addresses_share_a_slot(probe):
    off, _ = product_layout(probe)
    rd, wr = count_all(off)
    print("cases with a conflict: %d of the reads, %d of the writes" % (rd, wr))
    assert rd == 0 and wr == 0


def test_former_layout_has_conflicts():
    """The mutant: the check sees the layout this one replaces."""
    off, _ = former_layout()
    rd, wr = count_all(off)
    print("former layout, cases with a conflict: %d of the reads, %d of the writes" % (rd, wr))
    assert rd > 0 and wr > 0


def round_trip(probe, dv, iv):
    dv_in, iv_in = np.array(dv, np.float64), np.array(iv, np.int32)
    dv_out, iv_out, pieces = np.zeros(2, np.float64), np.zeros(16, np.int32), np.zeros(64, np.uint8)
    vp = C.c_void_p
    probe.rcp_round_trip(dv_in.ctypes.data_as(vp), iv_in.ctypes.data_as(vp), dv_out.ctypes.data_as(vp),
                         iv_out.ctypes.data_as(vp), pieces.ctypes.data_as(vp))
    return dv_out, iv_out, pieces


def test_packed_cell_round_trip(probe):
    none = probe.rcp_none()
    assert none == -1
    inf = float("inf")
    doubles = [-inf, 0.0, -0.0, -1e-300, -745.13321910194122, 1.0, 0.49999999999999994]
    counts = [0, 1, 0x7fff, 0x8000, 65535]
    positions = [0, 1, 65535, -20, 65535 + 20]                 # interval ends, and the ends offset beyond either side
    indices = [none, 0, 1, 111, 127]
    pairs = [0, 0xffff, 0xffff0000 - (1 << 32), -1, 0x12345678]   # (end_pos | end_cnt << 16) as int32 bit patterns
    n = 0
    for j in range(5):
        for k in range(5):
            for dp, dhr in ((doubles[(j + k) % 7], doubles[(j * 3 + k) % 7]), (-inf, -inf)):
                iv = [positions[j], positions[(j + k) % 5], positions[(j + 2 * k) % 5],
                      counts[k], counts[(j + k) % 5], counts[(2 * j + k) % 5],
                      indices[j], indices[k], indices[(j + k) % 5], indices[(j + 2 * k) % 5],
                      pairs[j], pairs[k], pairs[(j + k) % 5], pairs[(j + 3 * k) % 5]]
                dv_out, iv_out, _ = round_trip(probe, [dp, dhr], iv)
                assert np.array([dp, dhr]).tobytes() == dv_out.tobytes(), (dp, dhr)
                assert iv_out[:14].tolist() == iv, (iv, iv_out)
                assert iv_out[14] == 0 and iv_out[15] == 0        # pos[E], cnt[E]: not kept
                n += 1
    # every boundary value has been in every field of its kind
    assert n == 50
    # where the fields lie: dp and dhr in the first piece, the counts in the last with its upper half unused
    _, _, pieces = round_trip(probe, [-inf, 1.0], [1, 2, 3, 65535, 65534, 65533, none, 5, 6, 7, 8, 9, 10, 11])
    assert pieces[:16].tobytes() == np.array([-inf, 1.0]).tobytes()
    assert pieces[16:28].tobytes() == np.array([1, 2, 3], np.int32).tobytes() and pieces[28:32].tolist() == [255, 5, 6, 7]
    assert pieces[32:48].tobytes() == np.array([8, 9, 10, 11], np.uint32).tobytes()
    assert pieces[48:54].tobytes() == np.array([65535, 65534, 65533], np.uint16).tobytes() and not pieces[54:].any()

"""Inputs of tests/test_wall_path_inputs.py and tests/test_gpu_wall_paths.py: small reads, built with fixed seeds, that
between them pass through every fork of k_wall_tasks / k_find_wall (classpro_amd/csrc/kernels.hip), and what the oracle
makes of them (computed once per process).

WHICH fork a read takes is decided by a dozen numbers of the read -- the ACCOUNT, counted by hh_wall_paths of
tests/host_harness.cpp in the very function that hh_classify_read runs, so it cannot drift from the orchestration that
is pinned to the reference's golden vectors -- and by the kernel's constants, restated below under the kernel's names.
`wall_paths` restates the kernel's predicates on those numbers; `ROWS` is the reach table: what the set must contain,
and how often.  tests/test_gpu_wall_paths.py ties the account to the device (the counts k_wall_tasks leaves per read
must equal n_c, n_t, n_live0 of the account).

The account of a read:
  n_c       candidates by the scan rule (min(c[i-1],c[i]) < REPEAT and |c[i-1]-c[i]| >= 3)
  n_t       tasks: passes (SELF, OTHERS) of a candidate whose threshold filter says CP_CF_LIVE
  n_live0   the SELF tasks among them
  x         distinct ends of the walk's SELF E-intervals that are no candidates ("off-list SELF walls")
  NSw, NO   E- and O-intervals after the walk
  NSd       E-intervals after sort and dedupe
  midx      ... after the multi-error search
  m1        runs of overlapping intervals before the one that holds the last interval (the lane-parallel merge unites
            these; the kernel's `Mm`)
  NSm       E-intervals after cp_merge_eintvl
  C         connected components of the final list
  overflow  cp_read_t::overflow (8: the reference's "# E-intvls >= plen" abort)

The building blocks (K = 40, hcov / dcov = 20 / 40; what each adds to the account of a flat diploid read, measured with
the account itself):
  tooth     K positions at 1             n_c +2, SELF +2, NSw = NSm = C +1       (unrel_round_inputs.comb_reads)
  plateau   30 positions at 20           n_c +2, no task
  to_h      the read ends at 20          n_c +1, no task
  to_3      the read ends at 3           n_c +1, SELF +1, no interval            (an odd number of SELF tasks)
  low3      K positions at 3             n_c +2, SELF +2, no interval
  o_tooth   K positions at 36            n_c +2, OTHERS +2, NO +2
  o_plat    100 positions at 35          n_c +2, OTHERS +1, NO +1
  dip       20 positions at 1            n_c +2, SELF +2, NSw +0, midx +1        (a multi-error interval)
  pair      2 at 2, 2 at 8, 40 at 1, 1 at 8, 10 at 4
                                         n_c +6, SELF +3, NSw +2, NSm +3, C +1: a run of two overlapping intervals
  burst     5 at 2, 41 at 1, 1 at 4, 1 at 2, 1 at 40, 60 at 20
                                         n_c +5, SELF +3, x +1, NSw +2, midx +4, NSm +5, C +1: a run of four
  end_drop  the read ends with 20 at 1   n_c +1, SELF +1, x +1, NSw +1           (a pair with the read's end)
  end_39    the read ends with 39 at 1   n_c +1, SELF +1, midx +1, x +0          (a multi-error interval to the read's end)
  start_39  the read starts with 39 at 1 n_c +1, SELF +1, midx +1, x +0          (... from the read's start)
  zigzag    40, 1, 40, 1, ...            every position a candidate and a SELF task, x = 2, one component; up to 8
            positions the reference aborts on it (NSm = plen)
The thresholds of a candidate depend on the low-complexity context of its bases, so what a motif adds depends on the
sequence under it: o_plat and a few teeth come out differently here and there under random bases (the table below is
asserted on the account, not on these sums), and pair, start_39 and end_39 are only used over the period-4 sequence
ACGTACGT..., which has no homopolymer, di- or tri-nucleotide run anywhere (`periodic`).

Rows (a) to (d) of the table -- what no read of the generated and adversarial sets reaches:
  (a) the list starts in LDS and moves to HBM during the multi-error search (midx > FW_EVL with n_live0 <= FW_EVL): REACHED
      by 33 and by 42 bursts (4 intervals before the merge for 3 SELF tasks).  Only through wave_wall_mult: a burst has an
      off-list SELF wall, and no motif was found (2 x 150000 random mixes of 3-10 segments) with more than one
      interval per SELF task and none, which cf_wall_mult's wave_grow would need.
  (b) the same during the merge (midx <= FW_EVL < NSm): REACHED by 26 bursts (fw_evl::put with big == 0).
  (c) cf with C > SCOMP: REACHED by 63 teeth + start_39 + end_39: 128 SELF tasks (the one-lane replay, list still in LDS),
      every end of the walk's intervals a candidate, 65 components.  With the flags on chip from the start it cannot
      happen: a component costs two SELF tasks except the two at the read's ends, so C <= n_live0/2+1 <= 63.
  (d) the lane-parallel merge refused by `NS+2*(m1+1) < lim` with NS <= 64: REACHED by 32 pairs (NS = 64, m1 = 31,
      lim = FW_EVL), flags on chip, and through lim = plen by reads of 5 and 7 k-mers with 3 and 5 intervals in one run
      (NS+2 = plen; found among random reads of 4-13 k-mers, kept as short5 and short7; the zigzags of 5 and 8 k-mers,
      which the reference aborts on, get there too).

The test `n_c <= 255` in k_find_wall's `onchip` (and `cf`) is never the deciding one: 3*n_c+2*SCOMP+1 <= U16 beside it
gives n_c <= (768-129)/3 = 213.
"""
import collections
import ctypes as C
import functools

import numpy as np

from adversarial import adversarial_reads

K, READ_LEN, HCOV, DCOV = 40, 20000, 20, 40
OTHER_K = (25, 101)                                        # row 12

# ---- the kernel's constants, named as in kernels.hip ----
LCAP0, LCAP1, FW_EVL, FW_XCAP = 256, 64, 128, 8
SCOMP, U16, WAVE, GRP_MAX_PLEN = 64, 768, 64, 65535
CP_MAX_N_HC = 5                                            # cp_types.h

ACCOUNT = ("n_c", "n_t", "n_live0", "x", "NSw", "NO", "NSd", "midx", "m1", "NSm", "C", "overflow")


def account(H, P, s, p):
    """hh_wall_paths of tests/host_harness.cpp for one read: dict of ACCOUNT."""
    out = np.zeros(len(ACCOUNT), np.int64)
    sb = np.frombuffer(s, np.uint8)
    p = np.ascontiguousarray(p, np.uint16)
    rc = H.hh_wall_paths(C.c_void_p(P), sb.ctypes.data_as(C.c_void_p), len(s), p.ctypes.data_as(C.c_void_p),
                         out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return dict(zip(ACCOUNT, (int(v) for v in out)))


def wall_paths(row, plen, K):
    """k_find_wall's forks for a read with account `row`: the kernel's predicates, in the kernel's order."""
    n_c, n_t, n_live0, x = row["n_c"], row["n_t"], row["n_live0"], row["x"]
    icap, ecap = 2 * n_c + 4, 16 * n_c + 64
    ccap = icap >> 1
    o = dict(icap=icap, ecap=ecap, ccap=ccap, others=n_t - n_live0)
    o["use_lds"] = (1 if 2 * n_live0 <= LCAP0 - 8 else 0) | (2 if 2 * (n_t - n_live0) <= LCAP1 - 8 else 0)
    o["big0"] = n_live0 > FW_EVL or ecap < FW_EVL                        # the E list in HBM from the start
    o["eligible"] = plen <= 65535 and n_c <= 255 and 3 * n_c + 2 * SCOMP + 1 <= U16 and not o["big0"]
    o["onchip0"] = o["use_lds"] == 3 and o["eligible"]                   # flags on chip at the start of the replay
    o["lane_replay"] = o["use_lds"] == 3
    o["bail"] = o["onchip0"] and x > FW_XCAP
    o["onchip"] = o["onchip0"] and not o["bail"]
    o["use_win"] = (not o["lane_replay"]) and K + 24 + CP_MAX_N_HC < 128
    # (neither replay moves the list: an append per SELF task at the most, and n_live0 <= FW_EVL while it is in LDS)
    o["cf"] = o["onchip"] or (o["eligible"] and x == 0)                  # the copy-in: every end of an E-interval a candidate
    o["copy_in"] = o["cf"] and not o["onchip"]
    o["unwall"] = "wave" if o["cf"] and not o["big0"] and row["NSw"] <= WAVE else ("cf" if o["cf"] else "arrays")
    o["on16"] = plen <= 65535 and 2 * n_c + 2 * SCOMP + 1 <= U16
    o["mult"] = "cf" if o["cf"] else ("arrays16" if o["on16"] else "arrays32")
    o["moves_in_mult"] = (not o["big0"]) and row["midx"] > FW_EVL        # (a)
    big1 = o["big0"] or o["moves_in_mult"]
    ns = max(row["NSd"], row["midx"])                                    # the list the merge starts from
    o["ns_merge"] = ns
    if not big1 and 2 <= ns <= WAVE:
        lim = min(ecap, plen, FW_EVL)
        o["merge"] = "lanes" if ns + 2 * (row["m1"] + 1) < lim else "refused"
    else:
        o["merge"] = "one_lane"
    o["moves_in_merge"] = (not big1) and row["NSm"] > FW_EVL             # (b)
    o["comps"] = "lanes" if row["NSm"] <= WAVE and ccap >= WAVE else "one_lane"
    o["smallc"] = o["on16"] and min(row["C"], ccap) <= SCOMP
    o["bounds"] = "counted" if o["cf"] and o["smallc"] else "merged"
    o["cleanup"] = "none" if o["onchip"] else ("whole" if row["overflow"] else "lists")
    o["aos_long"] = plen > GRP_MAX_PLEN
    return o


# ---- the reads ----
Read = collections.namedtuple("Read", "name seq prof")


def _read(name, parts, seed, K=K, periodic=False):
    rng = np.random.default_rng(seed)
    c = np.concatenate([np.full(n, v) for n, v in parts]).astype(np.uint16)
    bases = np.arange(len(c) + K - 1) % 4 if periodic else rng.integers(0, 4, len(c) + K - 1)
    return Read(name, bytes(b"ACGT"[v] for v in bases), c)


def motif_read(name, seed, K=K, gap=80, start=(), end=(), periodic=False, **motifs):
    """A flat diploid read with the given numbers of motifs (module docstring), shuffled, `gap` positions apart."""
    kinds = dict(tooth=[(K, 1)], plateau=[(30, HCOV)], low3=[(K, 3)], o_tooth=[(K, 36)], o_plat=[(100, 35)], dip=[(20, 1)],
                 pair=[(2, 2), (2, 8), (40, 1), (1, 8), (10, 4)], burst=BURST)
    rng = np.random.default_rng(seed)
    order = [k for k, n in motifs.items() for _ in range(n)]
    order = [order[i] for i in rng.permutation(len(order))]
    parts = list(start) + [(90, DCOV)]
    for k in order:
        parts += kinds[k] + [(30 if k == "plateau" else gap, DCOV)]
    parts += list(end)
    return _read(name, parts, seed + 1000, K, periodic)


TO_H, TO_3, END_DROP, END_39, START_39 = [(60, HCOV)], [(60, 3)], [(20, 1)], [(39, 1)], [(39, 1)]


def zigzag(plen):
    c = np.where(np.arange(plen) % 2 == 0, DCOV, 1).astype(np.uint16)
    rng = np.random.default_rng(plen)
    return Read("zigzag%d" % plen, bytes(b"ACGT"[v] for v in rng.integers(0, 4, plen + K - 1)), c)


def long_comb(name, plen, seed):
    """Ten teeth in a read of exactly `plen` k-mers, five at either end (the last positions are the ones beyond 16 bits)."""
    teeth = [(K, 1), (80, DCOV)] * 5
    parts = [(90, DCOV)] + teeth + [(0, DCOV)] + teeth[:-1] + [(3, DCOV)]        # (the last tooth ends three positions before plen)
    parts[11] = (plen - sum(n for n, _ in parts), DCOV)
    return _read(name, parts, seed)


def _adv(seed, idx, plen=None):
    s, p = adversarial_reads(seed)
    s, p = s[idx], p[idx]
    if plen is None:
        return Read("adv%d_%d" % (seed, idx), s, p)
    return Read("adv%d_%d_plen%d" % (seed, idx, plen), s[:plen + K - 1], np.ascontiguousarray(p[:plen]))   # a prefix


BURST = [(5, 2), (41, 1), (1, 4), (1, 2), (1, 40), (60, HCOV)]


def _adv_bursts(seed, idx, n):
    """An adversarial read, a flat, then n bursts over the periodic sequence: the read's own off-list SELF walls are the
    first of the list, the bursts' fill it and overflow it."""
    r = _adv(seed, idx)
    tail = np.concatenate([np.full(m, v) for m, v in [(300, DCOV)] + (BURST + [(80, DCOV)]) * n]).astype(np.uint16)
    return Read("%s_burst%d" % (r.name, n), r.seq + bytes(b"ACGT"[k % 4] for k in range(len(tail))), np.concatenate([r.prof, tail]))


def mixed_memo(K=K):
    """Row 1's reads whose SELF memo is off chip, for any K (row 12 runs them at K = 25 and K = 101)."""
    return [motif_read("teeth62_to3", 1, K, tooth=62, end=TO_3), motif_read("teeth63", 2, K, tooth=63),
            motif_read("teeth63_otooth15", 3, K, tooth=63, o_tooth=15)]


@functools.lru_cache(maxsize=None)
def reads():
    R = [motif_read("teeth62", 4, tooth=62), motif_read("teeth10", 5, tooth=10)]
    R += mixed_memo()
    R += [motif_read("teeth5_otooth14", 6, tooth=5, o_tooth=14), motif_read("teeth5_otooth14_oplat", 7, tooth=5, o_tooth=14, o_plat=1),
          motif_read("teeth5_otooth15", 8, tooth=5, o_tooth=15), motif_read("teeth65_otooth16", 9, tooth=65, o_tooth=16)]
    # off-list SELF walls: 1..7, the full list, the bail
    R += [motif_read("teeth10_enddrop", 10, tooth=10, end=END_DROP), _adv(1, 0), _adv(1, 160), _adv(5, 162), _adv(2, 174, 193),
          _adv(2, 174, 254), _adv(2, 174, 258), _adv(2, 174)]
    # off-list SELF walls that the multi-error search pairs with an O-only wall (an interval is lost if one of them is
    # forgotten: found by doing just that in a copy of the harness; no read above has one): on chip (cf_wall_mult's
    # walk over the list), and first in the list of a read that bails (the list's copy to the arrays)
    R += [_adv(7, 228), _adv(10, 85), _adv_bursts(10, 85, 8), _adv_bursts(10, 85, 10)]
    # flags never on chip, memo on chip
    R += [motif_read("nc3", 11, tooth=1, end=TO_H), motif_read("nc4", 12, tooth=2),
          motif_read("nc213", 13, tooth=50, plateau=56, end=TO_H), motif_read("nc214", 14, tooth=50, plateau=57)]
    # the one-lane replay and the copy-in
    R += [motif_read("teeth63_enddrop", 15, tooth=63, end=END_DROP), _adv(3, 156), _adv(5, 228),
          motif_read("teeth63_plateau45", 16, tooth=63, plateau=45), motif_read("teeth62_to3_plateau46", 17, tooth=62, plateau=46, end=TO_3)]
    # the list in HBM from the start; list lengths 64 | 65
    R += [motif_read("teeth64", 18, tooth=64), motif_read("teeth65", 19, tooth=65), motif_read("teeth70", 20, tooth=70),
          zigzag(84), zigzag(85), zigzag(86),
          motif_read("teeth32_dip32", 21, tooth=32, dip=32), motif_read("teeth32_dip33", 22, tooth=32, dip=33),
          motif_read("teeth30_dip35", 23, tooth=30, dip=35), motif_read("teeth20_pair22", 24, periodic=True, tooth=20, pair=22),
          motif_read("teeth6_pair2", 25, periodic=True, tooth=6, pair=2), motif_read("teeth6_low3", 26, tooth=6, low3=3)]
    # components
    R += [motif_read("nc61", 27, tooth=30, end=TO_H), motif_read("nc62", 28, tooth=31),
          motif_read("nc319", 29, tooth=50, plateau=109, end=TO_H), motif_read("nc320", 30, tooth=50, plateau=110)]
    R += [long_comb("plen65535", 65535, 31), long_comb("plen65536", 65536, 32)]
    # the reference aborts on these
    R += [zigzag(3), zigzag(4), zigzag(5), zigzag(8)]
    # (a) to (d)
    R += [Read("short5", b"CCGCCGCGGTGTCCTAGGTGGCGACACATCTACAGATCAAGAAC", np.array([40, 1, 40, 3, 40], np.uint16)),
          Read("short7", b"GGCGCGCAATGGTCCCGGCGCAACGCCTGCGACCCAGATTGCCGGC", np.array([38, 1, 41, 1, 20, 40, 3], np.uint16))]
    R += [motif_read("burst33", 33, burst=33), motif_read("burst42", 34, burst=42), motif_read("burst26", 35, burst=26),
          motif_read("teeth63_start39_end39", 36, periodic=True, tooth=63, start=START_39, end=END_39),
          motif_read("pair32", 37, periodic=True, pair=32)]
    names = [r.name for r in R]
    assert len(set(names)) == len(names)
    return tuple(R)


@functools.lru_cache(maxsize=None)
def reads_other_k(k):
    return tuple(mixed_memo(k))


@functools.lru_cache(maxsize=None)
def expected(k=K):
    """Per read of reads() / reads_other_k(k), the oracle's dict(wall, rel, lab) -- or None where the reference aborts."""
    from oracle.oracle import Oracle
    O = Oracle(k, READ_LEN, HCOV, DCOV)
    out = []
    for r in (reads() if k == K else reads_other_k(k)):
        l, rc = O.seq_context(r.seq)
        try:
            iv = O.find_wall(r.prof, l, rc)
        except RuntimeError:
            out.append(None)
            continue
        out.append(dict(wall=iv, rel=O.find_rel_intvl(iv, r.prof, l, rc), lab=O.classify_read(r.seq, r.prof)))
    return tuple(out)


# ---- the reach table: (row, what, minimum number of reads, predicate on (account, paths, plen)) ----
def _v(key, val):
    return lambda a, p, n: (a[key] if key in a else p[key]) == val


ROWS = [
    ("1", "use_lds = 3", 2, _v("use_lds", 3)), ("1", "use_lds = 1", 2, _v("use_lds", 1)),
    ("1", "use_lds = 2", 2, _v("use_lds", 2)), ("1", "use_lds = 0", 2, _v("use_lds", 0)),
    ("1", "n_live0 = 124", 1, _v("n_live0", 124)), ("1", "n_live0 = 125", 1, _v("n_live0", 125)),
    ("1", "OTHERS tasks = 28", 1, _v("others", 28)), ("1", "OTHERS tasks = 29", 1, _v("others", 29)),
    ("2", "flags on chip to the end, x = 0", 2, lambda a, p, n: p["onchip"] and a["x"] == 0),
    ("2", "... x in 1..7", 2, lambda a, p, n: p["onchip"] and 1 <= a["x"] <= 7),
    ("2", "... x = 8", 1, lambda a, p, n: p["onchip"] and a["x"] == FW_XCAP),
    ("3", "bail, x = 9", 1, lambda a, p, n: p["bail"] and a["x"] == FW_XCAP + 1),
    ("3", "bail, x >= 10", 1, lambda a, p, n: p["bail"] and a["x"] >= FW_XCAP + 2),
    ("4", "lane replay on the arrays", 2, lambda a, p, n: p["lane_replay"] and not p["onchip0"]),
    ("4", "... n_c = 3 (ecap < FW_EVL)", 1, lambda a, p, n: p["lane_replay"] and not p["onchip0"] and a["n_c"] == 3),
    ("4", "n_c = 4, on chip", 1, lambda a, p, n: p["onchip0"] and a["n_c"] == 4),
    ("4", "n_c = 213, on chip", 1, lambda a, p, n: p["onchip0"] and a["n_c"] == 213 and a["n_live0"] <= 124),
    ("4", "n_c = 214, lane replay on the arrays", 1,
     lambda a, p, n: p["lane_replay"] and not p["onchip0"] and a["n_c"] == 214 and a["n_live0"] <= 124),
    ("5", "one-lane replay, copy-in", 2, lambda a, p, n: not p["lane_replay"] and p["copy_in"]),
    ("5", "one-lane replay, copy-in refused by a miss", 2, lambda a, p, n: not p["lane_replay"] and p["eligible"] and a["x"] > 0),
    ("5", "one-lane replay, not eligible (n_c > 213)", 2, lambda a, p, n: not p["lane_replay"] and not p["big0"] and a["n_c"] > 213),
    ("6", "n_live0 = 128, list in LDS", 1, lambda a, p, n: a["n_live0"] == 128 and not p["big0"]),
    ("6", "n_live0 >= 129, list in HBM", 2, lambda a, p, n: a["n_live0"] >= 129 and p["big0"]),
    ("7", "NSw = 64, un-wall by the wave form", 1, lambda a, p, n: a["NSw"] == 64 and p["unwall"] == "wave"),
    ("7", "NSw = 65, cf, list in LDS", 1, lambda a, p, n: a["NSw"] == 65 and p["unwall"] == "cf" and not p["big0"]),
    ("7", "64 before the merge, list in LDS", 1, lambda a, p, n: p["ns_merge"] == 64 and p["merge"] != "one_lane"),
    ("7", "65 before the merge", 1, lambda a, p, n: p["ns_merge"] == 65),
    ("7", "NSm = 64, lane per interval", 1, lambda a, p, n: a["NSm"] == 64 and p["comps"] == "lanes"),
    ("7", "NSm = 65", 1, lambda a, p, n: a["NSm"] == 65 and a["n_c"] >= 62),
    ("7", "exactly one of the three beyond 64", 1,
     lambda a, p, n: (a["NSw"] > 64) + (p["ns_merge"] > 64) + (a["NSm"] > 64) == 1),
    ("7", "NSw <= 64 < midx", 1, lambda a, p, n: a["NSw"] <= 64 < a["midx"]),
    ("8", "lane-parallel merge, m1 >= 1", 2, lambda a, p, n: p["merge"] == "lanes" and a["m1"] >= 1),
    ("8", "lane-parallel merge, m1 = 0", 2, lambda a, p, n: p["merge"] == "lanes" and a["m1"] == 0),
    ("8", "one-lane scan, NS > 64", 2, lambda a, p, n: p["merge"] == "one_lane" and p["ns_merge"] > 64),
    ("9", "n_c = 61 (ccap < 64), NS <= 64", 1, lambda a, p, n: a["n_c"] == 61 and a["NSm"] <= 64 and p["comps"] == "one_lane"),
    ("9", "n_c = 62, NS <= 64", 1, lambda a, p, n: a["n_c"] == 62 and a["NSm"] <= 64 and p["comps"] == "lanes"),
    ("9", "C = 64", 1, lambda a, p, n: a["C"] == 64 and p["smallc"]),
    ("9", "C = 65", 1, lambda a, p, n: a["C"] == 65 and not p["smallc"]),
    ("9", "n_c = 319 (on16)", 1, lambda a, p, n: a["n_c"] == 319 and p["on16"]),
    ("9", "n_c = 320", 1, lambda a, p, n: a["n_c"] == 320 and not p["on16"]),
    ("10", "plen = 65535, on chip", 1, lambda a, p, n: n == 65535 and p["onchip"] and a["n_c"] >= 20),
    ("10", "plen = 65536", 1, lambda a, p, n: n == 65536 and p["aos_long"] and not p["on16"] and a["n_c"] >= 20),
    ("11", "the reference aborts, not on chip", 2, lambda a, p, n: a["overflow"] != 0 and p["cleanup"] == "whole"),
    ("11", "the reference aborts, on chip", 1, lambda a, p, n: a["overflow"] != 0 and p["onchip"]),
    ("a", "list leaves LDS in the multi-error search", 0, lambda a, p, n: p["moves_in_mult"]),
    ("b", "list leaves LDS in the merge", 0, lambda a, p, n: p["moves_in_merge"]),
    ("c", "cf with C > SCOMP", 0, lambda a, p, n: p["cf"] and a["C"] > SCOMP),
    ("d", "lane-parallel merge refused, NS <= 64", 0, lambda a, p, n: p["merge"] == "refused" and a["overflow"] == 0),
]


def reach_table(accounts, plens, k=K):
    """[(row, what, minimum, names of the reads that reach it)] for accounts {name: account}."""
    out = []
    for row, what, need, pred in ROWS:
        hit = [nm for nm, a in accounts.items() if pred(a, wall_paths(a, plens[nm], k), plens[nm])]
        out.append((row, what, need, hit))
    return out

"""Inputs of tests/test_wall_load_inputs.py and tests/test_gpu_wall_loads.py: small reads at the edges of what k_wall_tasks
(classpro_amd/csrc/kernels.hip) keeps on chip and of the load groups of cp_wall_candidate_live (cp_wall.h).

  * the lists on chip: a read of at most FW_LISTS = 255 candidates keeps positions, info words, count pairs and task codes
    in LDS; the steps of phases 1a / 1b take 64 candidates / tasks each.  Counted by the harness's account
    (wall_path_inputs.account: n_c, n_t);
  * the wide count load: the eight counts from lo8 = j0-2 (partners to the right, j0 = i+K-1) or j0-6 (to the left,
    j0 = i-K+1) hold the counts of the six high-complexity partners and of a low-complexity partner at offset
    d = n-m in -1 .. 5 from j0; any other d, and every partner of a candidate whose eight counts do not lie inside the
    read, is loaded on its own.  What a live task does there is restated below (`live_tasks`) from the ORACLE's
    context arrays and tables -- nothing of the code under test.

The motifs are those of wall_path_inputs (a tooth: two candidates, two SELF tasks; a plateau: two candidates, no task;
to_h: a candidate; to_3: a candidate and a SELF task).  A `run` puts a homopolymer or a dinucleotide run under the bases
of a tooth's DROP, which moves its low-complexity partner: d = n-m with m = (t+1)*l the capped run before the DROP's
last base and n how far the run goes on behind it.
"""
import functools

import numpy as np

import wall_path_inputs as W
from wall_path_inputs import Read, K, READ_LEN, HCOV, DCOV, motif_read, TO_H, TO_3

FW_LISTS = 255                                             # kernels.hip
WAVE = 64
CP_MAX_N_HC = 5
CP_SELF, CP_OTHERS, CP_DROP, CP_GAIN = 0, 1, 0, 1
CP_MAX_CNT_CHANGE = 5
SKEL_CDMAX = {1: 1 * 512 - 1, 1024: 1024 * 512 - 1}       # capi.hip: cdmax = MB*2^20/8/256-1


class Tables:
    """What the restatement needs of the model: the oracle's tables (oracle/, the reference's arithmetic)."""

    def __init__(self, k=K):
        from oracle.oracle import Oracle
        self.O = Oracle(k, READ_LEN, HCOV, DCOV)
        self.K = k
        self.cthres, self.pe, self.lmax = self.O.cthres(), self.O.pe(), self.O.lmax()
        self.cov, _, self.cmax, _ = self.O.scalars()


@functools.lru_cache(maxsize=None)
def tables(k=K):
    return Tables(k)


def live_tasks(T, r):
    """The live (candidate, pass) pairs of read r, in the walk's order, each a dict: i, e, right, t, l, n, d = n-m,
    lc (none | boundary | inside), j, wide, lc_in_wide, hc_out (high-complexity partners beyond the read's end),
    far (products cov*|j-i| of the OTHERS pass's partners with cin <= cout)."""
    lctx, rctx = T.O.seq_context(r.seq)
    p = r.prof.astype(np.int64)
    plen, Kk = len(p), T.K
    REPEAT, HAPLO = T.cov[1], T.cov[2]

    def ctx(w, i):                                         # ClassPro.c:138-142
        return lctx[i + Kk - 2] if w == CP_DROP else rctx[i]

    out = []
    for i in range(1, plen):
        a, b = int(p[i - 1]), int(p[i])
        if min(a, b) >= REPEAT or abs(a - b) < 3:
            continue
        w = CP_DROP if a > b else CP_GAIN
        cin, cout, cng = min(a, b), max(a, b), abs(a - b)
        maxpe, t, l = -np.inf, -1, -1                      # wall.c:624-634
        for tt in range(3):
            ll = min(int(ctx(w, i)[tt]), int(T.lmax[tt]))
            if maxpe < T.pe[tt][ll]:
                maxpe, t, l = T.pe[tt][ll], tt, ll
        for e in (CP_SELF, CP_OTHERS):
            live = True                                    # cp_wall_candidate_filter, wall.c:643-653, 672-676
            if cout < T.cmax:
                ct_i, ct_f = int(T.cthres[t][l][cout][0][e]), int(T.cthres[t][l][cout][1][e])
                if not (cng > CP_MAX_CNT_CHANGE or cin < max(ct_i, 3)):
                    live = False
            if live and e == CP_SELF:
                if cout < T.cmax and cin >= ct_f:
                    live = False
            elif live and (cng >= HAPLO or (cout < T.cmax and cin < ct_f)):
                live = False                               # a wall by the count change alone
            if not live:
                continue
            right = w == CP_DROP
            ulen, m, n = t + 1, (t + 1) * l, 0
            while True:                                    # wall.c:345-352 / 432-439
                idx = i + ulen * (n + 1) if right else i - ulen * (n + 1)
                if (idx >= plen) if right else (idx <= 0):
                    break
                if int(ctx(w, idx)[t]) != m + n + 1:
                    break
                n += 1
            d = n - m
            j0 = i + Kk - 1 if right else i - Kk + 1
            j = j0 + d if right else j0 - d
            lo8 = j0 - 2 if right else j0 - (CP_MAX_N_HC + 1)
            wide = lo8 >= 0 and lo8 + 8 <= plen
            if (j <= i) if right else (j >= i):
                lc = "none"
            elif (j >= plen) if right else (j <= 0):
                lc = "boundary"
            else:
                lc = "inside"
            hc = [j0 + q if right else j0 - q for q in range(CP_MAX_N_HC + 1)]
            hc_in = [x for x in hc if (x < plen if right else x > 0)]
            far = []
            if e == CP_OTHERS and lc != "none":
                for x in ([j] if lc == "inside" else []) + hc_in:
                    ci, co = (int(p[x - 1]), int(p[x])) if right else (int(p[x]), int(p[x - 1]))
                    if ci <= co:
                        cv = max(a, int(p[x])) if right else max(int(p[x - 1]), b)
                        far.append(cv * abs(x - i))
            out.append(dict(i=i, e=e, right=right, t=t, l=l, n=n, d=d, lc=lc, j=j, wide=wide, lo8=lo8,
                            lc_in_wide=lc == "inside" and wide and -1 <= d <= CP_MAX_N_HC,
                            hc_out=len(hc) - len(hc_in) if lc != "none" else 0, far=far))
    return out


# ---- the reads ----
def _bases(seed, n):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, n)


def _mk(name, counts, bases):
    c = np.asarray(counts, np.uint16)
    assert len(bases) == len(c) + K - 1
    return Read(name, bytes(b"ACGT"[v] for v in bases), c)


def run_read(name, seed, right, unit, before, after, low=1):
    """One tooth in a flat diploid read over random bases without a run of their own near it, with a run of `unit`
    (1: homopolymer, 2: dinucleotide) laid under the tooth's first wall (right: its DROP, whose contexts end at base
    i+K-2) or its last (its GAIN, whose contexts begin at base i): `before` bases of the run up to and including that
    base, `after` bases behind it in the walk's direction."""
    plen = 400
    c = np.full(plen, DCOV)
    i0 = 150
    c[i0:i0 + K] = low
    i = i0 if right else i0 + K
    x = _bases(seed, plen + K - 1)
    for q in range(1, len(x)):                             # no homopolymer, dinucleotide or trinucleotide run by chance
        while x[q] == x[q - 1] or (q >= 2 and x[q] == x[q - 2]) or (q >= 3 and x[q] == x[q - 3]):
            x[q] = (x[q] + 1) % 4
    pat = [0] if unit == 1 else [0, 1]
    if right:
        last = i + K - 2
        lo, hi = last - before + 1, last + after
    else:
        lo, hi = i - after, i + before - 1
    for q in range(lo, hi + 1):
        x[q] = pat[(q - lo) % len(pat)]
    for q in (lo - 1, hi + 1):                             # the run ends where it should
        while x[q] in (x[q + 1] if q < lo else x[q - 1], x[q + 2] if q < lo else x[q - 2], 0, 1):
            x[q] = (x[q] + 1) % 4
    return _mk(name, c, x)


def end_read(name, seed, first, last):
    """A read of 120 k-mers with a tooth `first` positions after its start and one that ends `last` positions before its end."""
    plen = 120 + first + last
    c = np.full(plen, DCOV)
    c[first:first + K] = 1
    c[plen - last - K:plen - last] = 1
    return _mk(name, c, _bases(seed, plen + K - 1))


def edge_read(name, seed, head, tail):
    """A read that begins with `head` positions at 1 and ends with `tail`: a GAIN whose partners run into the read's start
    and a DROP whose partners run into its end (head = tail = K+5: the eight counts of the wide load begin at the read's
    first count / end at its last)."""
    plen = 300
    c = np.full(plen, DCOV)
    c[:head] = 1
    c[plen - tail:] = 1
    return _mk(name, c, _bases(seed, plen + K - 1))


def far_read(name, seed):
    """OTHERS tasks next to counts of 30000: cov*|j-i| of their partners lies beyond the default Skellam table."""
    plen = 600
    c = np.full(plen, DCOV)
    for s in (100, 300):
        c[s:s + K] = 36                                    # o_tooth: a DROP and a GAIN of 4, OTHERS tasks
    c[141:151] = 30000                                     # among the partners right of the first DROP (j0 = 139) ...
    c[290:299] = 30000                                     # ... and left of the second GAIN (j0 = 301)
    return _mk(name, c, _bases(seed, plen + K - 1))


def long_read(name, plen, seed):
    """A handful of candidates in a read beyond 65535 k-mers, the last of them beyond position 65535."""
    c = np.full(plen, DCOV)
    for s in (500, 40000, plen - 200):
        c[s:s + K] = 1
    return _mk(name, c, _bases(seed, plen + K - 1))


@functools.lru_cache(maxsize=None)
def reads():
    R = [motif_read("flat", 101), motif_read("nc1", 102, end=TO_H), motif_read("nt1", 103, end=TO_3),
         motif_read("nc63", 104, tooth=31, end=TO_H), motif_read("nc64", 105, tooth=32), motif_read("nc65", 106, tooth=32, end=TO_3),
         motif_read("nt128", 107, tooth=64), motif_read("nt129", 108, tooth=64, end=TO_3),
         motif_read("nc255", 109, tooth=50, plateau=77, end=TO_H), motif_read("nc256", 110, tooth=50, plateau=78),
         motif_read("nc257", 111, tooth=50, plateau=78, end=TO_H),
         motif_read("nc255_nt130", 112, tooth=65, plateau=62, end=TO_H), motif_read("nc300_nt200", 113, tooth=100, plateau=50)]
    # the low-complexity partner around the wide load: d = after-before, homopolymers and dinucleotide runs, both sides
    for right in (True, False):
        side = "r" if right else "l"
        for unit, before, after in ((1, 1, 0), (1, 2, 0), (1, 3, 1), (1, 2, 2), (1, 1, 6), (1, 1, 7), (1, 2, 8), (2, 2, 1), (2, 4, 2)):
            R.append(run_read("run_%s_u%d_b%d_a%d" % (side, unit, before, after), 200 + 10 * before + after + 100 * unit, right, unit, before, after))
    R += [end_read("ends_%d_%d" % (f, l), 300 + 10 * f + l, f, l) for f, l in ((1, 1), (2, 3), (4, 5), (6, 7), (8, 8), (9, 9))]
    R += [edge_read("edge_%d_%d" % (h, t), 350 + h + t, h, t) for h, t in ((20, 20), (K + 2, K + 2), (K + 5, K + 5), (K + 4, K + 6))]
    R += [far_read("far", 400), long_read("plen70000", 70000, 401)]
    names = [r.name for r in R]
    assert len(set(names)) == len(names)
    return tuple(R)


@functools.lru_cache(maxsize=None)
def expected():
    """Per read of reads(), the oracle's dict(wall, rel, lab) as wall_path_inputs.expected() (None: the reference aborts)."""
    O = tables().O
    out = []
    for r in reads():
        l, rc = O.seq_context(r.seq)
        try:
            iv = O.find_wall(r.prof, l, rc)
        except RuntimeError:
            out.append(None)
            continue
        out.append(dict(wall=iv, rel=O.find_rel_intvl(iv, r.prof, l, rc), lab=O.classify_read(r.seq, r.prof)))
    return tuple(out)

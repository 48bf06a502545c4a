"""The commit of k_classify_unrel_grp with four lanes per slot and K = 8 or 16 slots equals the serial loop.  CPU.

`serial` and `closed_form` are those of test_unrel_commit_rule.py.  With four lanes per slot a read holds more slots than
a slot has lanes, so "lane `role` of a slot looks at slot `role`" became "lane `role` looks at the slots role, role+4, ...
below its own", and the per-byte masks of the ballots became per-nibble ones.  `lane_form` restates that lane by lane,
with the kernel's masks as 64-bit integers: ballots over the read's L = 4K lanes, the any-bit-in-nibble fold, the first
stop, the second sweep's stop, then every `need` clear before every `need` set and the set change last.  All three forms
run on random rounds of small N and must leave the same classes, `need` bits, reliable sets and next position.
"""
import numpy as np

from test_unrel_commit_rule import D, H, closed_form, serial, set_change

LPS = 4
M64 = (1 << 64) - 1


def ffs(x):
    return (x & -x).bit_length()                           # 1-based, 0 for 0 -- __ffsll


def lane_form(st, N, slots, cover, sweep2, seen=None):
    K = len(slots)
    L = K * LPS
    glm = (1 << L) - 1
    LEADS = 0x1111111111111111 & glm
    LOWS = 0x7777777777777777
    idx = [slots[q // LPS][0] for q in range(L)]           # per lane, as the kernel holds them
    snew = [slots[q // LPS][2] for q in range(L)]
    mypos = [slots[q // LPS][1] for q in range(L)]
    sub = [q // LPS for q in range(L)]
    role = [q % LPS for q in range(L)]
    lead = [role[q] == 0 for q in range(L)]
    upd = [snew[q] >= 0 for q in range(L)]
    old, hd, setc = [0] * L, [False] * L, [False] * L
    for q in range(L):
        if lead[q] and upd[q]:
            old[q] = int(st["asgn"][idx[q]])
            ohd, nhd = old[q] in (H, D), snew[q] in (H, D)
            hd[q] = old[q] != snew[q] and (ohd or nhd)
            setc[q] = hd[q] and bool(st["isrel"][idx[q]])
    ballot = lambda v: sum(1 << q for q in range(L) if v[q])
    m_hd, m_setc = ballot(hd), ballot(setc)
    cl, late = [False] * L, [False] * L
    for q in range(L):
        for c in range((K + LPS - 1) // LPS):
            o = role[q] + c * LPS
            osl = LPS * (o & (K - 1))
            oidx = idx[osl]
            hit = o < sub[q] and bool(((m_setc >> osl) & 1) or (((m_hd >> osl) & 1) and oidx in (idx[q] - 1, idx[q] + 1)))
            cl[q] |= hit
            late[q] |= hit and o == sub[q] - LPS           # slot j against slot j+4: a lane's second look
    clm = ballot(cl) & glm
    cb = ((clm | (((clm & LOWS) + LOWS) & M64)) >> (LPS - 1)) & LEADS
    ub = ballot([lead[q] and upd[q] for q in range(L)]) & glm
    stop = (~ub & LEADS) | cb
    js = ffs(stop) - 1 if stop else L                      # in lanes
    hb = (m_hd & glm) & ((1 << js) - 1)
    hstop = sweep2 and hb != 0
    jh = ffs(hb) - 1 if hstop else 0
    cstop = (not hstop) and js < L and bool((ub >> js) & 1)
    spos = mypos[jh if hstop else js if cstop else 0]
    newit = spos + 1 if hstop else spos if cstop else cover
    cm = [lead[q] and upd[q] and q < (jh + 1 if hstop else js) for q in range(L)]
    if seen is not None and cstop:
        n_cl = sum(cl[js:js + LPS])
        seen["late"] += any(late[js:js + LPS])
        seen["late_only"] += n_cl == 1 and any(late[js:js + LPS])
    for q in range(L):                                     # one LDS instruction of the wave: every clear ...
        if cm[q]:
            st["need"][idx[q]] = False
    for q in range(L):                                     # ... before the sets
        if cm[q] and hd[q]:
            if idx[q] > 0:
                st["need"][idx[q] - 1] = True
            if idx[q] + 1 < N:
                st["need"][idx[q] + 1] = True
    for q in range(L):
        if cm[q] and old[q] != snew[q]:
            st["asgn"][idx[q]] = snew[q]
    nset = 0
    for q in range(L):
        if cm[q] and setc[q]:
            assert not any(cm[q + 1:]), "a set change is the round's last commit"
            set_change(st, N, idx[q], old[q], snew[q])
            nset += 1
    assert nset <= 1
    return newit


def test_lane_form_equals_serial_commit():
    rng = np.random.default_rng(29)
    seen = {K: dict(clash=0, setc=0, hstop=0, idle=0, full=0, late=0, late_only=0) for K in (8, 16)}
    for trial in range(24000):
        K = 8 if trial % 2 == 0 else 16
        N = int(rng.integers(K, K + 20))
        st = dict(asgn=rng.integers(-1, 4, N).astype(np.int64), isrel=rng.random(N) < 0.15, need=rng.random(N) < 0.5,
                  rel=[np.zeros(N, bool), np.zeros(N, bool)])
        for q, sq in ((0, H), (1, D)):
            st["rel"][q][:] = st["isrel"] & (st["asgn"] == sq)
        idxs = rng.permutation(N)[:K]
        nact = int(rng.integers(0, K + 1)) if rng.random() < 0.3 else K
        p0 = int(rng.integers(0, 50))
        pos = p0 + np.cumsum(rng.integers(1, 4, K))
        # mostly "no change", so that rounds reach their later slots (a clash between slot j and slot j+4 needs four
        # slots in front of it that neither clash nor change a set)
        slots = [(int(idxs[j]), int(pos[j]),
                  (int(st["asgn"][idxs[j]]) if rng.random() < 0.75 and st["asgn"][idxs[j]] >= 0 else int(rng.integers(0, 4))) if j < nact else -1)
                 for j in range(K)]
        cover = int(pos[-1]) + 1
        sweep2 = bool(rng.integers(0, 2))
        cp = lambda: {k: ([x.copy() for x in v] if isinstance(v, list) else v.copy()) for k, v in st.items()}
        a, b, c = cp(), cp(), cp()
        na, nb = serial(a, N, slots, cover, sweep2), closed_form(b, N, slots, cover, sweep2)
        nc = lane_form(c, N, slots, cover, sweep2, seen[K])
        assert na == nb == nc, (trial, slots, sweep2, na, nb, nc)
        for k in ("asgn", "need"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (trial, k, slots, sweep2)
        for q in (0, 1):
            assert np.array_equal(a["rel"][q], b["rel"][q]) and np.array_equal(a["rel"][q], c["rel"][q]), (trial, q, slots, sweep2)
        s = seen[K]
        s["idle"] += nact < K
        s["full"] += na == cover and nact == K
        s["clash"] += na != cover and not (sweep2 and any(na == x[1] + 1 for x in slots))
        s["setc"] += any(not np.array_equal(st["rel"][q], a["rel"][q]) for q in (0, 1))
        s["hstop"] += sweep2 and na != cover and any(na == x[1] + 1 for x in slots)
    print(seen)
    for K in (8, 16):
        s = seen[K]
        assert min(s[k] for k in ("clash", "setc", "hstop", "idle", "full")) >= 500, seen
        # clashes between slot j and slot j+4, and those among them that only the lane's second look sees
        assert s["late"] >= 1 and s["late_only"] >= 1, seen

"""The closed form of k_classify_unrel_grp's commit equals the serial loop it replaces.  CPU.

A speculation round evaluates K slots (distinct intervals) on the state before the round and then commits them in order:
a slot is committed unless an earlier slot of the round changed the H-or-D-ness of an index neighbour or a reliable set;
the round stops at the first slot without an update, at the first clash, or (second sweep) behind the first committed
change to or from H / D.  The kernel computes, from the slots' own (idx, old class, new class, reliable) alone, where the
round stops, then lets the committed slots write at once: every `need` clear before every `need` set.  Both forms are
run here as plain Python on random rounds -- small N, so that neighbours, set changes and repeats are frequent -- and
must leave the same classes, `need` bits, reliable sets and next position.
"""
import numpy as np

H, D = 2, 3


def near(bits, idx, step, N):
    j = idx + step
    while 0 <= j < N:
        if bits[j]:
            return j
        j += step
    return -1


def set_change(st, N, ij, old, sj):
    """ij leaves / joins the reliable-H or the reliable-D set: mark what lies between its nearest members."""
    for q, sq in ((0, H), (1, D)):
        if old != sq and sj != sq:
            continue
        lo, hi = near(st["rel"][q], ij, -1, N), near(st["rel"][q], ij, 1, N)
        lo = 0 if lo < 0 else lo
        hi = N - 1 if hi < 0 else hi
        st["need"][lo:hi + 1] = True
        st["rel"][q][ij] = sj == sq


def serial(st, N, slots, cover, sweep2):
    newit, sets_changed, changed = cover, False, []
    for ij, pos, sj in slots:
        if sj < 0:
            break
        if sets_changed or any(c in (ij - 1, ij + 1) for c in changed):
            newit = pos
            break
        old = st["asgn"][ij]
        st["need"][ij] = False
        if old != sj:
            hd = old in (H, D) or sj in (H, D)
            if hd:
                if ij > 0:
                    st["need"][ij - 1] = True
                if ij + 1 < N:
                    st["need"][ij + 1] = True
            if st["isrel"][ij] and hd:
                set_change(st, N, ij, old, sj)
                sets_changed = True
            st["asgn"][ij] = sj
            if hd:
                changed.append(ij)
            if sweep2 and hd:
                newit = pos + 1
                break
    return newit


def closed_form(st, N, slots, cover, sweep2):
    K = len(slots)
    old = [int(st["asgn"][ij]) for ij, _, _ in slots]
    upd = [sj >= 0 for _, _, sj in slots]
    hd = [upd[j] and old[j] != slots[j][2] and (old[j] in (H, D) or slots[j][2] in (H, D)) for j in range(K)]
    setc = [hd[j] and bool(st["isrel"][slots[j][0]]) for j in range(K)]
    clash = [any(setc[m] or (hd[m] and abs(slots[m][0] - slots[j][0]) == 1) for m in range(j)) for j in range(K)]
    js = next((j for j in range(K) if not upd[j] or clash[j]), K)
    jh = next((j for j in range(js) if hd[j]), -1) if sweep2 else -1
    if jh >= 0:
        newit, ncommit = slots[jh][1] + 1, jh + 1
    else:
        newit, ncommit = (slots[js][1] if js < K and upd[js] else cover), js
    for j in range(ncommit):                               # all clears ...
        st["need"][slots[j][0]] = False
    for j in range(ncommit):                               # ... before all sets
        ij, _, sj = slots[j]
        if hd[j]:
            if ij > 0:
                st["need"][ij - 1] = True
            if ij + 1 < N:
                st["need"][ij + 1] = True
        st["asgn"][ij] = sj
    for j in range(ncommit):
        if setc[j]:
            assert j == ncommit - 1                        # a set change is the round's last commit
            set_change(st, N, slots[j][0], old[j], slots[j][2])
    return newit


def test_closed_form_equals_serial_commit():
    rng = np.random.default_rng(17)
    seen = dict(clash=0, setc=0, hstop=0, idle=0, full=0)
    for trial in range(20000):
        K = int(rng.choice([4, 8]))
        N = int(rng.integers(K, 24))
        st = dict(asgn=rng.integers(-1, 4, N).astype(np.int64), isrel=rng.random(N) < 0.3, need=rng.random(N) < 0.5,
                  rel=[np.zeros(N, bool), np.zeros(N, bool)])
        for q, sq in ((0, H), (1, D)):
            st["rel"][q][:] = st["isrel"] & (st["asgn"] == sq)
        idxs = rng.permutation(N)[:K]
        nact = int(rng.integers(0, K + 1)) if rng.random() < 0.3 else K
        p0 = int(rng.integers(0, 50))
        pos = p0 + np.cumsum(rng.integers(1, 4, K))
        # mostly "no change": a round of the product commits all of its slots more often than not
        slots = [(int(idxs[j]), int(pos[j]),
                  (int(st["asgn"][idxs[j]]) if rng.random() < 0.5 and st["asgn"][idxs[j]] >= 0 else int(rng.integers(0, 4))) if j < nact else -1)
                 for j in range(K)]
        cover = int(pos[-1]) + 1
        sweep2 = bool(rng.integers(0, 2))
        a = {k: ([x.copy() for x in v] if isinstance(v, list) else v.copy()) for k, v in st.items()}
        b = {k: ([x.copy() for x in v] if isinstance(v, list) else v.copy()) for k, v in st.items()}
        na, nb = serial(a, N, slots, cover, sweep2), closed_form(b, N, slots, cover, sweep2)
        assert na == nb, (trial, slots, sweep2)
        for k in ("asgn", "need"):
            assert np.array_equal(a[k], b[k]), (trial, k, slots, sweep2)
        for q in (0, 1):
            assert np.array_equal(a["rel"][q], b["rel"][q]), (trial, q, slots, sweep2)
        seen["idle"] += nact < K
        seen["full"] += na == cover and nact == K
        seen["clash"] += na != cover and not (sweep2 and any(na == s[1] + 1 for s in slots))
        seen["setc"] += any(not np.array_equal(st["rel"][q], a["rel"][q]) for q in (0, 1))
        seen["hstop"] += sweep2 and na != cover and any(na == s[1] + 1 for s in slots)
    assert min(seen.values()) > 500, seen

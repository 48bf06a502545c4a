"""Brute-force restatement of the sorted snapshot of a label table, one consensus class per call, and of its per-class
histogram (include/classpro_amd.h, "Sorted k-mers of a label table"), on top of the label table of tests/cns_oracle.py
({key: [E, H, D, R]}), its consensus rule and the .ktab layout of tests/ktab_oracle.py.  Test helper; nothing of the
product is imported."""
import numpy as np

import cns_oracle as C

MAXC = 32767
LABELS = C.LABELS


def select(t, label=None, min_total=1, min_pct=0):
    """[(key, total)] ascending by key: the keys of class `label` ("E" "H" "D" "R"; None: every key) whose total is at
    least min_total and whose largest count c has 100 * c >= min_pct * total."""
    out = []
    for k, c in t.items():
        tot, mx = sum(c), max(c)
        if label is not None and LABELS[C.consensus_label(c)] != label:
            continue
        if tot >= min_total and 100 * mx >= min_pct * tot:
            out.append((k, tot))
    return sorted(out)


def class_hist(t):
    """(hist int64 [4, 32767], ilowcnt [4], ihighcnt [4]): kprof_oracle.hist per consensus class, total for count."""
    h, ihigh = np.zeros((4, MAXC), np.int64), np.zeros(4, np.int64)
    for c in t.values():
        l, tot = C.consensus_label(c), sum(c)
        h[l, min(tot, MAXC) - 1] += 1
        if tot >= MAXC:
            ihigh[l] += tot
    return h, h[:, 0].copy(), ihigh


def hist_bytes(K, h, ilow, ihigh):
    """A FASTK .hist file of one class: int32 K, low = 1, high = 32767, int64 ilowcnt, ihighcnt, then the cells."""
    import struct
    return struct.pack("<iiiqq", K, 1, MAXC, int(ilow), int(ihigh)) + np.asarray(h, "<i8").tobytes()

"""Brute-force restatement of the k-mer count table (include/classpro_amd.h, "K-mer count table"): a Counter over the
canonical k-mers of all reads, per-read profiles min(count, 32767) with 0 for a k-mer holding a byte outside ACGT, and the
FASTK histogram with its two hidden cells.  Test helper; nothing of the product is imported."""
from collections import Counter

import numpy as np

MAXC = 32767
_RC = bytes.maketrans(b"ACGT", b"TGCA")
_OK = frozenset(b"ACGT")


def canon(km):
    rc = km.translate(_RC)[::-1]
    return rc if rc < km else km


def kmers(seq, K):
    """Per k-mer position of one read: the canonical k-mer, or None when it holds a byte other than A C G T."""
    seq = bytes(seq)
    bad = [i for i, c in enumerate(seq) if c not in _OK]
    out = []
    for i in range(len(seq) - K + 1):
        out.append(None if any(i <= b < i + K for b in bad) else canon(seq[i:i + K]))
    return out


def count(seqs, K):
    """(Counter of canonical k-mers, per-read k-mer lists, skipped positions)."""
    per = [kmers(s, K) for s in seqs]
    cnt = Counter(k for p in per for k in p if k is not None)
    return cnt, per, sum(1 for p in per for k in p if k is None)


def profiles(cnt, per):
    return [np.array([0 if k is None else min(cnt[k], MAXC) for k in p], np.uint16) for p in per]


def hist(cnt):
    """(1, 32767, ilowcnt, ihighcnt, int64[32767]) as fastk.write_fastk and hist_covs take it."""
    h = np.zeros(MAXC, np.int64)
    ihigh = 0
    for c in cnt.values():
        h[min(c, MAXC) - 1] += 1
        if c >= MAXC:
            ihigh += c
    return 1, MAXC, int(h[0]), ihigh, h


def stats(cnt, skipped):
    return dict(n_kmers=sum(cnt.values()), n_skipped=skipped, n_distinct=len(cnt))


def run(seqs, K):
    """Everything at once: dict(profiles, hist, stats)."""
    cnt, per, skipped = count(seqs, K)
    return dict(profiles=profiles(cnt, per), hist=hist(cnt), stats=stats(cnt, skipped), counter=cnt)

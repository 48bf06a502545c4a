"""Brute-force restatement of the lookups in a sorted k-mer table (include/classpro_amd.h, "Sorted k-mers as input"): a
dict over the entries of tests/ktab_oracle.py -- [(key, count)] ascending by key -- gives the ordinal of a key and the
per-read cells of a batch, for canonical and for forward keys.  Test helper; nothing of the product is imported."""
import numpy as np

import ktab_oracle as KO


def find(ents, keys):
    """The ordinal of each key in the table, -1 for one that is absent (Find_Kmer's return value)."""
    at = {k: i for i, (k, _) in enumerate(ents)}
    return [at.get(int(k), -1) for k in keys]


def read_keys(seq, K, canonical=True):
    """Per k-mer position of one read: the key looked up -- min(forward, reverse complement) or the forward k-mer as an
    integer of 2K bits, first base most significant -- or None for a k-mer with a byte other than A C G T."""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    mask, top = (1 << (2 * K)) - 1, 2 * (K - 1)
    fw = rc = valid = 0
    out = []
    for i, c in enumerate(bytes(seq)):
        b = code.get(c)
        if b is None:
            fw = rc = valid = 0
        else:
            fw = ((fw << 2) | b) & mask
            rc = (rc >> 2) | ((3 - b) << top)
            valid += 1
        if i >= K - 1:
            out.append(None if valid < K else min(fw, rc) if canonical else fw)
    return out


def keys_of(seqs, K, canonical=True):
    return [read_keys(s, K, canonical) for s in seqs]


def cells(ents, seqs, K, canonical=True, keys=None):
    """(per-read uint16 arrays of min(count, 32767) or 0, [cells present, absent, with other bytes]); `keys` is
    keys_of(seqs, K, canonical) when the caller has it already."""
    cnt = dict(ents)
    prof, tally = [], [0, 0, 0]
    for ks in keys_of(seqs, K, canonical) if keys is None else keys:
        for k in ks:
            tally[2 if k is None else 0 if k in cnt else 1] += 1
        prof.append(np.array([0 if k is None else min(cnt.get(k, 0), KO.MAXC) for k in ks], np.uint16))
    return prof, tally


def flat(prof):
    return np.concatenate(prof) if prof else np.zeros(0, np.uint16)

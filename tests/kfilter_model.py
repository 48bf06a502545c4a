"""Model of the singleton filter of a filtered count table (include/classpro_amd.h, "Filtered count table"; the hash is
kf_hash / kf_bits of classpro_amd/csrc/kmer_counts.hip, restated in numpy): a key owns one 64-bit word of the filter and up
to four bits in it, and is "seen before" when all of them were set already.  `simulate` runs the filter sequentially, in
the order of the occurrences.  Test helper; nothing of the product is imported."""
import numpy as np

M63 = (1 << 63) - 1
SALT = 0xd6e8feb86659fd93
_CODE = bytes.maketrans(b"ACGT", b"0123")


def key_of(kmer):
    """A canonical k-mer of A C G T (bytes) as the integer key: 2 bits per base, the first base highest."""
    return int(kmer.translate(_CODE), 4)


def mix(x):
    """kt_mix on a uint64 array (the multiplications wrap)."""
    x = x.copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return x


def word_and_mask(keys, filter_bits):
    """(word index, 64-bit mask) of every key (python ints below 2^126) as two uint64 arrays."""
    assert filter_bits >= 64 and filter_bits & (filter_bits - 1) == 0
    hi = np.array([k >> 63 for k in keys], np.uint64)
    lo = np.array([k & M63 for k in keys], np.uint64)
    h = mix(lo ^ mix(hi ^ np.uint64(SALT)))
    one, m = np.uint64(1), np.zeros(len(keys), np.uint64)
    for f in range(4):
        m |= one << ((h >> np.uint64(6 * f)) & np.uint64(63))
    return (h >> np.uint64(24)) & np.uint64(filter_bits // 64 - 1), m


def simulate(counter, filter_bits):
    """`counter`: a dict key -> number of occurrences whose order is the order of the FIRST occurrences (a Counter filled
    in read order).  Later occurrences of a key set no new bit, so only that order matters.  Returns dict(n_table_keys,
    n_false, n_outside) of a sequential run: a key is in the table when it occurs twice or its first occurrence found all
    its bits set; a singleton in the table is a false positive."""
    keys = list(counter)
    w, m = word_and_mask(keys, filter_bits)
    state = {}
    n_table = n_false = 0
    for k, wi, mi in zip(keys, w.tolist(), m.tolist()):
        old = state.get(wi, 0)
        seen = old & mi == mi
        state[wi] = old | mi
        if counter[k] >= 2:
            n_table += 1
        elif seen:
            n_table += 1
            n_false += 1
    return dict(n_table_keys=n_table, n_false=n_false, n_outside=len(keys) - n_table)

"""Brute-force restatement of the sorted k-mer table and of the FASTK .ktab layout as libfastk.c reads it (Open_Kmer_Stream,
Load_Kmer_Table, Find_Kmer), from the canonical counts of tests/kprof_oracle.py.  Written from the layout, not from
classpro_amd/fastk.py; nothing of the product is imported.

  key      the k-mer as an integer of 2K bits: first base most significant, A C G T = 0 1 2 3
  record   kbyte = (K+3)>>2 bytes hold the key left-aligned (first base in bits 7..6 of byte 0, unused low bits 0); the
           first ibyte of them (3 for K >= 13, 2 for K in 9..12, 1 for K in 5..8) are the prefix, the record is the
           other hbyte bytes and min(count, 32767) as a little-endian uint16
  index    index[p] = number of entries whose prefix, read big-endian, is <= p
  stub     int32 K, nparts, minval, ibyte; int64 index[1 << 8*ibyte]
  part     int32 K; int64 nels; the records; part p holds the entries [n*p/nparts, n*(p+1)/nparts)"""
import struct

import numpy as np

import kprof_oracle as O

MAXC = 32767
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}
M63 = (1 << 63) - 1


def key_of(kmer):
    v = 0
    for c in kmer:
        v = v * 4 + _CODE[c]
    return v


def text_of(key, K):
    return "".join("acgt"[(key >> (2 * (K - 1 - i))) & 3] for i in range(K))


def ibyte_of(K):
    return 3 if K >= 13 else 2 if K >= 9 else 1 if K >= 5 else 0


def entries(cnt, min_count=1):
    """The sorted table of a Counter of canonical k-mers: [(key, exact count)] ascending by key."""
    return sorted((key_of(k), c) for k, c in cnt.items() if c >= min_count)


def table(seqs, K, min_count=1):
    return entries(O.count(seqs, K)[0], min_count)


def hi_lo_cnt(ents):
    return [k >> 63 for k, _ in ents], [k & M63 for k, _ in ents], [c for _, c in ents]


def record(key, c, K):
    kbyte, ib = (K + 3) >> 2, ibyte_of(K)
    out = []
    for i in range(ib * 4, kbyte * 4, 4):                  # four bases per byte, the bases past K are 0 bits
        b = 0
        for j in range(i, i + 4):
            b = b * 4 + ((key >> (2 * (K - 1 - j))) & 3 if j < K else 0)
        out.append(b)
    c = min(c, MAXC)
    return bytes(out + [c & 255, c >> 8])


def prefix(key, K):
    p = 0
    for j in range(4 * ibyte_of(K)):
        p = p * 4 + ((key >> (2 * (K - 1 - j))) & 3 if j < K else 0)
    return p


def records(ents, K):
    return b"".join(record(k, c, K) for k, c in ents)


def records_fast(ents, K):
    """records() for millions of entries: the same bytes through int.to_bytes (test_ktab_host.py holds the two equal)."""
    kbyte, ib = (K + 3) >> 2, ibyte_of(K)
    pad = 8 * kbyte - 2 * K
    return b"".join((k << pad).to_bytes(kbyte, "big")[ib:] + struct.pack("<H", min(c, MAXC)) for k, c in ents)


def index(ents, K):
    per = np.zeros(1 << (8 * ibyte_of(K)), np.int64)       # an int64 array: up to 2^24 prefixes
    for k, _ in ents:
        per[prefix(k, K)] += 1
    return np.cumsum(per)


# ---- the same in numpy, for K <= 31 (a key fits 62 bits) and millions of k-mers of upper-case A C G T; held equal to
# the functions above on small inputs by tests/test_ktab_host.py ----

def table_np(seqs, K, min_count=1):
    """(keys uint64 ascending, counts int64) of the canonical k-mers of reads that hold nothing but A C G T."""
    code = np.full(256, 255, np.uint8)
    code[[65, 67, 71, 84]] = [0, 1, 2, 3]
    keys = []
    for s in seqs:
        b = code[np.frombuffer(s, np.uint8)].astype(np.uint64)
        assert (b < 4).all()
        n = len(b) - K + 1
        if n <= 0:
            continue
        fw, rc = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for j in range(K):
            x = b[j:j + n]
            fw = fw * np.uint64(4) + x
            rc = rc + ((np.uint64(3) - x) << np.uint64(2 * j))
        keys.append(np.minimum(fw, rc))
    k, c = np.unique(np.concatenate(keys), return_counts=True)
    keep = c >= min_count
    return k[keep], c[keep].astype(np.int64)


def records_np(keys, counts, K):
    kbyte, ib = (K + 3) >> 2, ibyte_of(K)
    left = keys << np.uint64(8 * kbyte - 2 * K)
    out = np.zeros((len(keys), kbyte - ib + 2), np.uint8)
    for b in range(ib, kbyte):
        out[:, b - ib] = (left >> np.uint64(8 * (kbyte - 1 - b))) & np.uint64(255)
    c = np.minimum(counts, MAXC)
    out[:, kbyte - ib] = c & 255
    out[:, kbyte - ib + 1] = c >> 8
    return out.tobytes()


def index_np(keys, K):
    ib = ibyte_of(K)
    return np.cumsum(np.bincount((keys >> np.uint64(2 * K - 8 * ib)).astype(np.int64), minlength=1 << (8 * ib)))


def files(ents, K, min_count, nparts):
    """{file name suffix: bytes}: "" is the stub `<root>.ktab`, p >= 1 the part `.<root>.ktab.p`."""
    idx = index(ents, K)
    out = {"": struct.pack("<iiii", K, nparts, min_count, ibyte_of(K)) + idx.astype("<i8").tobytes()}
    n = len(ents)
    for p in range(nparts):
        part = ents[n * p // nparts:n * (p + 1) // nparts]
        out[p + 1] = struct.pack("<i", K) + struct.pack("<q", len(part)) + records(part, K)
    return out


def read_files(d, root, nparts):
    import os
    out = {"": open(os.path.join(d, root + ".ktab"), "rb").read()}
    for p in range(nparts):
        out[p + 1] = open(os.path.join(d, ".%s.ktab.%d" % (root, p + 1)), "rb").read()
    return out


# ---- the reference's own readers (oracle/_ref/libclasspro_ref.so compiles libfastk.c whole) through ctypes ----

def ref_lib():
    """The library, or None when oracle/_ref is not built."""
    import ctypes as C
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                        "libclasspro_ref.so")
    if not os.path.exists(path):
        return None
    L = C.CDLL(path)
    L.Open_Kmer_Stream.restype = C.c_void_p
    L.Open_Kmer_Stream.argtypes = [C.c_char_p]
    for f in ("First_Kmer_Entry", "Next_Kmer_Entry", "Free_Kmer_Stream", "Free_Kmer_Table"):
        getattr(L, f).restype = None
        getattr(L, f).argtypes = [C.c_void_p]
    L.Current_Kmer.restype = C.c_void_p
    L.Current_Kmer.argtypes = [C.c_void_p, C.c_char_p]
    L.Load_Kmer_Table.restype = C.c_void_p
    L.Load_Kmer_Table.argtypes = [C.c_char_p, C.c_int]
    L.Fetch_Kmer.restype = C.c_void_p
    L.Fetch_Kmer.argtypes = [C.c_void_p, C.c_int64, C.c_char_p]
    L.Find_Kmer.restype = C.c_int64
    L.Find_Kmer.argtypes = [C.c_void_p, C.c_void_p]
    return L


def _stream_struct():
    import ctypes as C

    class KmerStream(C.Structure):                         # the public part of Kmer_Stream (libfastk.h)
        _fields_ = [("kmer", C.c_int), ("minval", C.c_int), ("nels", C.c_int64), ("cidx", C.c_int64),
                    ("csuf", C.POINTER(C.c_uint8)), ("cpre", C.c_int), ("ibyte", C.c_int), ("kbyte", C.c_int),
                    ("tbyte", C.c_int), ("hbyte", C.c_int), ("pbyte", C.c_int)]
    return KmerStream


def ref_stream(L, path):
    """(K, minval, [(k-mer text, count)]) as Open_Kmer_Stream / Next_Kmer_Entry / Current_Kmer walk the table.  The
    count is read through the stream's csuf pointer and hbyte field, which is what the inline Current_Count does."""
    import ctypes as C
    S = L.Open_Kmer_Stream(path.encode())
    assert S, "Open_Kmer_Stream(%s) failed" % path
    st = C.cast(S, C.POINTER(_stream_struct())).contents
    buf = C.create_string_buffer(st.kmer + 8)
    out = []
    L.First_Kmer_Entry(S)
    while bool(st.csuf):
        L.Current_Kmer(S, buf)
        out.append((buf.value.decode(), st.csuf[st.hbyte] | (st.csuf[st.hbyte + 1] << 8)))
        L.Next_Kmer_Entry(S)
    head = (st.kmer, st.minval, st.nels)
    L.Free_Kmer_Stream(S)
    assert head[2] == len(out)
    return head[0], head[1], out


class RefTable:
    """Load_Kmer_Table / Find_Kmer / Fetch_Kmer."""

    def __init__(self, L, path, cut_off=0):
        import ctypes as C
        self.L = L
        self.T = L.Load_Kmer_Table(path.encode(), cut_off)
        assert self.T, "Load_Kmer_Table(%s) failed" % path
        head = (C.c_int * 2).from_address(self.T)
        self.K, self.minval = head[0], head[1]
        self.nels = C.c_int64.from_address(self.T + 8).value
        self.buf = C.create_string_buffer(self.K + 16)     # Find_Kmer writes up to 3 bytes before and after the k-mer

    def find(self, text):
        import ctypes as C
        C.memmove(C.addressof(self.buf) + 4, text.encode(), self.K)
        return self.L.Find_Kmer(self.T, C.addressof(self.buf) + 4)

    def fetch(self, i):
        import ctypes as C
        out = C.create_string_buffer(self.K + 8)
        self.L.Fetch_Kmer(self.T, i, out)
        return out.value.decode()

    def close(self):
        self.L.Free_Kmer_Table(self.T)

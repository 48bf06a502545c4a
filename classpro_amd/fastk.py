"""FASTK on-disk formats that ClassPro consumes (`<root>.hist`, `<root>.prof`, `.<root>.pidx.N`,
`.<root>.prof.N`) -- Python writer/reader used to build test and benchmark inputs.

Format as read by the reference (all little-endian):
  .hist    int kmer, int low, int high, int64 ilowcnt, int64 ihighcnt, int64 hist[high-low+1]   (libfastk.c:72-83)
  .prof    int kmer, int nparts                                                              (libfastk.c:1291-1292)
  .pidx.N  int kmer, int64 first, int64 n, int64 endoff[n]  (cumulative byte ends in .prof.N) (libfastk.c:1305-1333)
  .prof.N  per read: first count 1 byte (<128) or 2 bytes (0x80|hi, lo); then
           00rrrrrr run of r equal counts, 01sxxxxx 6-bit signed delta, 1sxxxxxx yyyyyyyy 15-bit delta
                                                                                             (libfastk.c:1467-1534)
  .ktab    int kmer, int nparts, int minval, int ibyte, int64 index[1 << 8*ibyte]: index[p] = entries whose first
           ibyte key bytes, read big-endian, are <= p                          (libfastk.c:816-841, 994)
  .ktab.N  int kmer, int64 nels, nels records of (kmer+3)/4 - ibyte key bytes and a uint16 count
                                                                                             (libfastk.c:854-855, 1037-1047)
The production host path (C++ CLI, classpro_amd/csrc/host) has its own readers; this module is tooling.
"""
import gzip
import os
import struct
import numpy as np


def encode_profile(c):
    """Inverse of Fetch_Profile's decoder for one read (counts <= 32767)."""
    out = bytearray()
    n = len(c)
    if n == 0:
        return bytes(out)
    c = [int(x) for x in c]
    d = c[0]
    if d < 128:
        out.append(d)
    else:
        out.append(0x80 | (d >> 8))
        out.append(d & 0xFF)
    i = 1
    while i < n:
        if c[i] == d:
            run = 1
            while i + run < n and c[i + run] == d and run < 63:
                run += 1
            out.append(run)
            i += run
        else:
            dl = c[i] - d
            if 1 <= dl <= 31:
                out.append(0x40 | dl)
            elif -32 <= dl <= -1:
                out.append(0x60 | (dl + 32))
            else:
                x = dl & 0x7FFF
                out.append(0x80 | (x >> 8))
                out.append(x & 0xFF)
            d = c[i]
            i += 1
    return bytes(out)


def decode_profile(code):
    """Pure-Python decoder (tooling / cross-check of the encoder)."""
    code = bytes(code)
    if not code:
        return np.zeros(0, np.uint16)
    out = []
    p = 0
    x = code[p]; p += 1
    if x & 0x80:
        d = ((x & 0x7F) << 8) | code[p]; p += 1
    else:
        d = x
    out.append(d)
    while p < len(code):
        x = code[p]; p += 1
        if (x & 0xC0) == 0:
            out.extend([d] * x)
        else:
            if x & 0x80:
                v = ((x << 8) & 0xFFFF) if (x & 0x40) else ((x << 8) & 0x7FFF)
                v |= code[p]; p += 1
                d = (d + v) & 0x7FFF
            else:
                if x & 0x20:
                    d = (d + ((x & 0x1F) | 0xFFE0)) & 0xFFFF
                else:
                    d = (d + (x & 0x1F)) & 0xFFFF
            out.append(d)
    return np.array(out, dtype=np.uint16)


def write_fastk(dirpath, root, K, profiles, hist, nparts=1):
    """hist = (low, high, ilowcnt, ihighcnt, int64 array[high-low+1])."""
    os.makedirs(dirpath, exist_ok=True)
    low, high, ilow, ihigh, h = hist
    with open(os.path.join(dirpath, root + ".hist"), "wb") as f:
        f.write(struct.pack("<iii", K, low, high))
        f.write(struct.pack("<qq", ilow, ihigh))
        f.write(np.asarray(h, dtype="<i8").tobytes())
    with open(os.path.join(dirpath, root + ".prof"), "wb") as f:
        f.write(struct.pack("<ii", K, nparts))
    n = len(profiles)
    per = (n + nparts - 1) // nparts if nparts else n
    first = 0
    for part in range(nparts):
        chunk = profiles[part * per:(part + 1) * per]
        codes = [encode_profile(c) for c in chunk]
        ends = np.cumsum([len(c) for c in codes], dtype=np.int64) if codes else np.zeros(0, np.int64)
        with open(os.path.join(dirpath, ".%s.pidx.%d" % (root, part + 1)), "wb") as f:
            f.write(struct.pack("<i", K))
            f.write(struct.pack("<qq", first, len(chunk)))
            f.write(ends.astype("<i8").tobytes())
        with open(os.path.join(dirpath, ".%s.prof.%d" % (root, part + 1)), "wb") as f:
            f.write(b"".join(codes))
        first += len(chunk)


def read_fastk_hist(path):
    with open(path, "rb") as f:
        K, low, high = struct.unpack("<iii", f.read(12))
        ilow, ihigh = struct.unpack("<qq", f.read(16))
        h = np.frombuffer(f.read(8 * (high - low + 1)), dtype="<i8").copy()
    return K, low, high, ilow, ihigh, h


def read_fastk_codes(dirpath, root):
    """Returns (K, [code bytes per read]) without decoding."""
    with open(os.path.join(dirpath, root + ".prof"), "rb") as f:
        K, nparts = struct.unpack("<ii", f.read(8))
    codes = []
    for part in range(nparts):
        with open(os.path.join(dirpath, ".%s.pidx.%d" % (root, part + 1)), "rb") as f:
            _k = struct.unpack("<i", f.read(4))[0]
            _first, n = struct.unpack("<qq", f.read(16))
            ends = np.frombuffer(f.read(8 * n), dtype="<i8")
        with open(os.path.join(dirpath, ".%s.prof.%d" % (root, part + 1)), "rb") as f:
            blob = f.read()
        o = 0
        for e in ends:
            codes.append(blob[o:int(e)])
            o = int(e)
    return K, codes


def ktab_ibyte(K):
    """Prefix bytes of a .ktab for this K (cp_ktab_ibyte): 3, 2, 1, or 0 for "no .ktab for this K"."""
    return 3 if K >= 13 else 2 if K >= 9 else 1 if K >= 5 else 0


def write_fastk_ktab(dirpath, root, K, min_count, keys, counts, nparts=1):
    """Writes `<root>.ktab` and `.<root>.ktab.1..nparts`.  keys: Python ints, the 2K-bit k-mers (first base most
    significant, A C G T = 0 1 2 3), distinct and ascending; counts: their counts, clamped to 32767 in the records.
    Part p holds the entries [n*p/nparts, n*(p+1)/nparts)."""
    ibyte = ktab_ibyte(K)
    if ibyte == 0:
        raise ValueError("there is no .ktab for K < 5")
    keys = [int(k) for k in keys]
    if any(a >= b for a, b in zip(keys, keys[1:])):
        raise ValueError("keys must be distinct and ascending")
    if len(counts) != len(keys) or nparts < 1:
        raise ValueError("bad counts or nparts")
    kbyte = (K + 3) >> 2
    hbyte = kbyte - ibyte
    n = len(keys)
    index = np.zeros(1 << (8 * ibyte), np.int64)
    recs = []
    for k, c in zip(keys, counts):
        b = (k << (8 * kbyte - 2 * K)).to_bytes(kbyte, "big")
        index[int.from_bytes(b[:ibyte], "big")] += 1
        recs.append(b[ibyte:] + struct.pack("<H", min(int(c), 32767)))
    os.makedirs(dirpath, exist_ok=True)
    with open(os.path.join(dirpath, root + ".ktab"), "wb") as f:
        f.write(struct.pack("<iiii", K, nparts, min_count, ibyte))
        f.write(np.cumsum(index).astype("<i8").tobytes())
    for p in range(nparts):
        lo, hi = n * p // nparts, n * (p + 1) // nparts
        with open(os.path.join(dirpath, ".%s.ktab.%d" % (root, p + 1)), "wb") as f:
            f.write(struct.pack("<iq", K, hi - lo))
            f.write(b"".join(recs[lo:hi]))


def read_fastk_ktab(dirpath, root):
    """Returns (K, min_count, ibyte, keys, counts): keys as Python ints in file order (see write_fastk_ktab), counts a
    uint16 array.  The prefix of an entry comes from the index, as in libfastk.c."""
    with open(os.path.join(dirpath, root + ".ktab"), "rb") as f:
        K, nparts, min_count, ibyte = struct.unpack("<iiii", f.read(16))
        index = np.frombuffer(f.read(8 << (8 * ibyte)), dtype="<i8")
    kbyte = (K + 3) >> 2
    hbyte = kbyte - ibyte
    pbyte = hbyte + 2
    blob = b""
    for p in range(nparts):
        with open(os.path.join(dirpath, ".%s.ktab.%d" % (root, p + 1)), "rb") as f:
            pk, n = struct.unpack("<iq", f.read(12))
            if pk != K:
                raise ValueError("part %d has another K than the stub" % (p + 1))
            part = f.read()
            if len(part) != n * pbyte:
                raise ValueError("part %d does not hold %d records" % (p + 1, n))
            blob += part
    n = len(blob) // pbyte
    if len(index) and int(index[-1]) != n:
        raise ValueError("the index ends at %d, the parts hold %d entries" % (int(index[-1]), n))
    prefix = np.searchsorted(index, np.arange(n), side="right")
    keys, counts = [], np.zeros(n, np.uint16)
    for i in range(n):
        r = blob[i * pbyte:(i + 1) * pbyte]
        b = int(prefix[i]).to_bytes(ibyte, "big") + r[:hbyte]
        keys.append(int.from_bytes(b, "big") >> (8 * kbyte - 2 * K))
        counts[i] = r[hbyte] | (r[hbyte + 1] << 8)
    return K, min_count, ibyte, keys, counts


def read_fastk_ktab_raw(dirpath, root):
    """Returns (K, min_count, ibyte, index, records): the stub's prefix index as an int64 array of 1 << 8*ibyte and the
    records of all parts, in file order, as one uint8 array -- the payload as it is on disk, no key decoded (what
    `SortedKmers.from_records` takes).  The checks are those of read_fastk_ktab."""
    with open(os.path.join(dirpath, root + ".ktab"), "rb") as f:
        K, nparts, min_count, ibyte = struct.unpack("<iiii", f.read(16))
        index = np.frombuffer(f.read(8 << (8 * ibyte)), dtype="<i8").astype(np.int64)
    if len(index) != 1 << (8 * ibyte):
        raise ValueError("the stub is truncated")
    pbyte = ((K + 3) >> 2) - ibyte + 2
    parts = []
    for p in range(nparts):
        with open(os.path.join(dirpath, ".%s.ktab.%d" % (root, p + 1)), "rb") as f:
            pk, n = struct.unpack("<iq", f.read(12))
            if pk != K:
                raise ValueError("part %d has another K than the stub" % (p + 1))
            part = np.frombuffer(f.read(), np.uint8)
            if len(part) != n * pbyte:
                raise ValueError("part %d does not hold %d records" % (p + 1, n))
            parts.append(part)
    records = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    if int(index[-1]) * pbyte != len(records):
        raise ValueError("the index ends at %d, the parts hold %d entries" % (int(index[-1]), len(records) // pbyte))
    return K, min_count, ibyte, index, records


def write_fasta(path, names, seqs, gz=None, comments=None):
    gz = path.endswith(".gz") if gz is None else gz
    op = gzip.open if gz else open
    with op(path, "wb") as f:
        for i, (n, s) in enumerate(zip(names, seqs)):
            hdr = n if not comments else "%s %s" % (n, comments[i])
            f.write(b">" + hdr.encode() + b"\n" + s + b"\n")

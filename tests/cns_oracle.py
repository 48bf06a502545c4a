"""A Python restatement of the reference's k-mer consensus pipeline (scripts/naive_consensus.sh), the oracle of the
class2cns / KmerTable tests:

  * dump       src/class2cns.c:62-68: "KMER L\\n" for every position i in [K-1, rlen) of every record;
  * sort_uniq  `LC_ALL=C sort | uniq -c` on those lines ("%7d %s\\n", byte order);
  * table      per distinct k-mer the four label counts (order E, H, D, R), forward or canonical keys;
  * stats      agg2cons.py:calc_mcf over the table, the consistency as include/classpro_amd.h defines it (64.64 fixed
               point, correctly rounded), the tie rule R > D > H > E of the consensus label.
"""
import gzip
from fractions import Fraction

LABELS = "EHDR"
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def read_class(path):
    """Records of a .class file (FASTQ-like, one line each): list of (header line without '@', seq bytes, labels)."""
    op = gzip.open if path.endswith(".gz") else open
    lines = op(path, "rb").read().split(b"\n")
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]


def dump(records, K):
    out = []
    for _h, s, q in records:
        for i in range(K - 1, len(s)):
            out.append(s[i - K + 1:i + 1] + b" " + q[i:i + 1] + b"\n")
    return b"".join(out)


def sort_uniq(text):
    lines = text.split(b"\n")[:-1] if text else []
    lines.sort()
    out, i = [], 0
    while i < len(lines):
        j = i
        while j < len(lines) and lines[j] == lines[i]:
            j += 1
        out.append(b"%7d %s\n" % (j - i, lines[i]))
        i = j
    return b"".join(out)


def key_of(kmer):
    k = 0
    for c in kmer:
        k = (k << 2) | _CODE[c]
    return k


def kmer_of(key, K):
    return bytes(b"ACGT"[(key >> (2 * (K - 1 - i))) & 3] for i in range(K))


def valid(kmer):
    return all(c in _CODE for c in kmer)


def table(records, K, canonical=False):
    """{key: [E, H, D, R]} and the number of skipped positions."""
    t, skipped = {}, 0
    for _h, s, q in records:
        for i in range(K - 1, len(s)):
            km = s[i - K + 1:i + 1]
            if not valid(km):
                skipped += 1
                continue
            if canonical:
                km = min(km, km.translate(_COMP)[::-1])
            k = key_of(km)
            c = t.setdefault(k, [0, 0, 0, 0])
            c[LABELS.index(chr(q[i]))] += 1
    return t, skipped


def consensus_label(c):
    best = 0
    for l in range(1, 4):
        if c[l] >= c[best]:
            best = l
    return best


def s_fixed(counts):
    """S = sum of floor(total * 2^64 / max) over the entries (each a list of four counts)."""
    return sum((sum(c) << 64) // max(c) for c in counts)


def consistency(n, s):
    """The correctly rounded double of n * 2^64 / S (Python's int / int is correctly rounded)."""
    return (n << 64) / s if n else float("nan")


def consistency_exact(counts):
    """n / sum(total/max) as a Fraction: what the fixed-point figure approximates."""
    counts = list(counts)
    return Fraction(len(counts)) / sum(Fraction(sum(c), max(c)) for c in counts)


def stats(t, skipped):
    cs = list(t.values())
    label_total = [sum(c[l] for c in cs) for l in range(4)]
    cns_total = [0, 0, 0, 0]
    for c in cs:
        cns_total[consensus_label(c)] += sum(c)
    s = s_fixed(cs)
    return dict(n_kmers=sum(label_total), n_skipped=skipped, n_distinct=len(cs),
                n_unanimous=sum(1 for c in cs if sum(c) == max(c)), label_total=label_total, cns_total=cns_total,
                s_fixed=s, consistency=consistency(len(cs), s))


def consensus_records(records, K, t, canonical=False):
    """The records with every counted position relabelled by its k-mer's consensus label."""
    out = []
    for h, s, q in records:
        q = bytearray(q)
        for i in range(K - 1, len(s)):
            km = s[i - K + 1:i + 1]
            if not valid(km):
                continue
            if canonical:
                km = min(km, km.translate(_COMP)[::-1])
            q[i] = ord(LABELS[consensus_label(t[key_of(km)])])
        out.append((h, s, bytes(q)))
    return out


def uniq_table(t, K):
    """What class2cns -u prints: "%7d KMER L" per (k-mer, label) with a count > 0, key order, then D < E < H < R."""
    out = []
    for k in sorted(t):
        km = kmer_of(k, K)
        for l in (2, 0, 1, 3):
            if t[k][l]:
                out.append(b"%7d %s %s\n" % (t[k][l], km, LABELS[l].encode()))
    return b"".join(out)

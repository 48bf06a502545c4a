"""Brute-force restatement of the ground truth genome2class gives (include/classpro_amd.h, "Relative labels"): the count
of each read k-mer in a Counter over the canonical k-mers of the genome (its a c g t folded to upper case, the reads left
as they are), the labels prof2class makes of those counts, the .class text, and a small diploid case that holds plenty of
every label.  Test helper built on tests/kprof_oracle.py; nothing of the product is imported except file writers."""
import random

import numpy as np

import kprof_oracle as O

_FOLD = bytes.maketrans(b"acgt", b"ACGT")
_RC = bytes.maketrans(b"ACGT", b"TGCA")


def fold(seq):
    """The genome-only case fold: a c g t count as A C G T, every other byte stays."""
    return bytes(seq).translate(_FOLD)


def genome_counter(genome_seqs, K):
    return O.count([fold(g) for g in genome_seqs], K)[0]


def rel_profiles(genome_seqs, read_seqs, K, counter=None):
    """Per read: min(count in the genome, 32767) of every k-mer, 0 for one that is absent or holds a byte other than
    upper-case A C G T."""
    cnt = genome_counter(genome_seqs, K) if counter is None else counter
    return [np.array([0 if k is None else min(cnt.get(k, 0), O.MAXC) for k in O.kmers(s, K)], np.uint16)
            for s in read_seqs]


def labels(rel, rlen, K):
    """prof2class.c:203-254: K-1 'N' (rlen 'N' for a read shorter than K), then 0 -> E, 1 -> H, 2 -> D, >= 3 -> R."""
    if rlen <= K - 1:
        return b"N" * rlen
    assert len(rel) == rlen - (K - 1)
    return b"N" * (K - 1) + bytes(b"EHDR"[min(int(c), 3)] for c in rel)


def label_counts(labs):
    """[E, H, D, R] over a list of label strings."""
    x = b"".join(labs)
    return [x.count(c) for c in b"EHDR"]


def class_text(names, seqs, labs, headers=None):
    """The .class file: "@name (null)" is what the reference prints for a FASTX read without a comment; `headers`
    (complete lines, "@..." included) replaces that for database sources."""
    headers = headers or ["@%s (null)" % n for n in names]
    return b"".join(h.encode() + b"\n" + bytes(s) + b"\n+\n" + l + b"\n" for h, s, l in zip(headers, seqs, labs))


def _rnd(rng, n):
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def make_case(seed, K=40):
    """A small diploid case: dict(genome_names, genome (4 contigs: haplotype A's two, then B's), names, seqs).
    Haplotype A: about 40 kbp in two contigs, a 2-kbp segment at three places, a microsatellite.  B: A with SNPs outside
    one SNP-free block.  Contig 2 holds a run of N (the reads see random bases there); contig 1 holds a soft-masked
    lower-case stretch that reads cover.  Reads: about 25x, 3-8 kbp, both strands, substitutions and 1-base indels;
    then one read shorter than K, one of exactly K-1 bases and one holding an N."""
    rng = random.Random(seed)
    a1, a2 = _rnd(rng, 22000), _rnd(rng, 18000)
    rep = _rnd(rng, 2000)
    a1[2000:4000] = rep
    a1[15000:17000] = rep
    a2[9000:11000] = rep
    a2[3000:3300] = b"AC" * 150
    hap = []
    for a, free in ((a1, (6000, 12000)), (a2, (0, 0))):
        b = bytearray(a)
        for p in range(0, len(b)):
            if not free[0] <= p < free[1] and rng.random() < 1 / 70:
                b[p] = rng.choice(bytes(set(b"ACGT") - {b[p]}))
        hap.append(b)
    b1, b2 = hap
    gap = (13000, 13060)                                           # the assembly's N run in contig 2 of both haplotypes
    mask = (18000, 18900)                                          # soft-masked in contig 1 of both
    genome = []
    for c1, c2 in ((a1, a2), (b1, b2)):
        g1 = bytes(c1[:mask[0]]) + bytes(c1[mask[0]:mask[1]]).lower() + bytes(c1[mask[1]:])
        g2 = bytes(c2[:gap[0]]) + b"N" * (gap[1] - gap[0]) + bytes(c2[gap[1]:])
        genome += [g1, g2]
    true = [bytes(x) for x in (a1, a2, b1, b2)]
    seqs = []
    target = 25 * 40000
    while sum(len(s) for s in seqs) < target:
        src = true[rng.randrange(4)]
        n = rng.randint(3000, 8000)
        s0 = rng.randrange(0, len(src) - n)
        out = bytearray()
        for c in src[s0:s0 + n]:
            u = rng.random()
            if u < 0.004:
                out.append(rng.choice(bytes(set(b"ACGT") - {c})))
            elif u < 0.006:
                continue                                           # deletion
            elif u < 0.008:
                out.append(c)
                out.append(rng.choice(b"ACGT"))                   # insertion
            else:
                out.append(c)
        s = bytes(out)
        seqs.append(s.translate(_RC)[::-1] if rng.random() < 0.5 else s)
    seqs.insert(3, bytes(true[0][500:510]))                       # shorter than K
    seqs.insert(9, bytes(true[1][700:700 + K - 1]))               # exactly K-1 bases: an empty profile
    s = bytes(true[2][5000:8000])
    seqs.insert(14, s[:1500] + b"N" + s[1501:])
    names = ["read%d" % i for i in range(len(seqs))]
    return dict(genome_names=["hapA_1", "hapA_2", "hapB_1", "hapB_2"], genome=genome, names=names, seqs=seqs)


def cut(seq, b, K):
    """A contig in pieces of at most b + K-1 bases that overlap by K-1: every k-mer lies in exactly one."""
    return [seq[s:s + b + K - 1] for s in range(0, max(len(seq) - (K - 1), 0), b)]

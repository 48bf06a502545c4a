"""Inputs of the pruning tests (tests/test_prune_host.py, tests/test_gpu_prune.py): graphs built by hand whose expected marks
follow from how they are built, and the read sets of the first-principles case.  Nothing of the product is imported.

A hand case is (name, sequences, K, limits, expect): `expect` maps the sequence of a unitig that has to go -- in either
orientation -- to its mark; every other unitig stays."""
import random

import unitig_oracle as UO
from test_unitig_host import clean, rcs, rnd, simple

SEEDS = (1, 2, 3, 4, 5, 6)                                 # of the first-principles case: kept fixed


def other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def expected_why(utgs, expect):
    """The marks of the unitigs of unitig_oracle.unitigs() under a hand case's `expect`; every key of it must be met."""
    why = [expect.get(u[1], expect.get(rcs(u[1]), 0)) for u in utgs]
    assert sum(w != 0 for w in why) == len(expect), (expect, [u[1] for u in utgs])
    return why


def fork(seed, K, la, lb):
    """A stem of 6K bases that ends in two dead-end branches of la and lb nodes: (stem, a, b), the branches from the K-1 bases
    they share with the stem on."""
    rng = random.Random(seed)
    while True:
        stem = rnd(rng, 6 * K)
        c = rng.choice("ACGT")
        a, b = stem[-(K - 1):] + c + rnd(rng, la - 1), stem[-(K - 1):] + other(c) + rnd(rng, lb - 1)
        if clean([stem, a, b], K, (6 * K - K + 2) + la + lb):
            return stem, a, b


def snp(seed, K, arms=2, flank=None):
    """`arms` haplotypes that differ at one base between two flanks of `flank` bases."""
    rng = random.Random(seed)
    flank = 2 * K - 2 if flank is None else flank
    while True:
        left, right = rnd(rng, flank), rnd(rng, flank)
        c = rng.choice("ACGT")
        hs = [left + other(c, k) + right for k in range(arms)]
        if clean(hs, K, 2 * (flank - K + 2) + arms * (K - 1)):
            return hs


def hand_cases():
    K = 9
    T = 2 * K
    cases = []
    # a tip on a path: four nodes hang off the middle of a long path
    rng = random.Random(7)
    while True:
        main = simple(rng, 80, K)
        tip = main[40 - K + 1:40] + other(main[40]) + rnd(rng, 3)
        if clean([main, tip], K, 80 - K + 2 + 4):
            break
    cases.append(("tip on a path", [main, tip], K, (0, T, 0), {tip: 2}))
    # two tip candidates at one junction
    stem, a, b = fork(11, K, 5, 3)
    cases.append(("the longer tip stays", [stem, a, b], K, (0, T, 0), {b: 2}))
    stem, a, b = fork(12, K, 4, 4)
    cases.append(("equal nodes: the heavier tip stays", [stem, a, b, b], K, (0, T, 0), {a: 2}))
    stem, a, b = fork(13, K, 4, 4)
    first = min(a, b, key=lambda s: min(UO.canon(UO.key_of(s[:K]), K), UO.canon(UO.key_of(s[-K:]), K)))
    cases.append(("all equal: the smaller ordinal stays", [stem, a, b], K, (0, T, 0), {a if first == b else b: 2}))
    # a lone dead end: a short stem before a fork of two long branches has no competitor
    rng = random.Random(17)
    while True:
        stem = rnd(rng, K + 3)
        c = rng.choice("ACGT")
        a, b = stem[-(K - 1):] + c + rnd(rng, 40), stem[-(K - 1):] + other(c) + rnd(rng, 40)
        if clean([stem, a, b], K, 5 + 41 + 41):
            break
    cases.append(("a lone dead end stays", [stem, a, b], K, (0, T, 0), {}))
    # bubbles: the arms of a SNP have K nodes and 2K-1 bases
    h = snp(3, K)
    cases.append(("bubble, unequal counts", [h[0], h[0], h[1]], K, (0, 0, 2 * K - 1), {h[1][2 * K - 2 - (K - 1):2 * K - 2 + K]: 3}))
    arm = lambda s: s[K - 1:3 * K - 2]                     # the arm of a haplotype of snp(): its K k-mers over the site
    arms = sorted((arm(x) for x in h), key=lambda s: min(UO.canon(UO.key_of(s[:K]), K), UO.canon(UO.key_of(s[-K:]), K)))
    cases.append(("bubble, equal counts", h, K, (0, 0, 2 * K - 1), {arms[1]: 3}))
    cases.append(("bubble, arms one base over the limit", [h[0], h[0], h[1]], K, (0, 0, 2 * K - 2), {}))
    h = snp(5, K, 3)
    cases.append(("three arms, unequal", [h[0]] * 3 + [h[1]] * 2 + [h[2]], K, (0, 0, 2 * K - 1), {arm(h[1]): 3, arm(h[2]): 3}))
    arms = sorted((arm(x) for x in h), key=lambda s: min(UO.canon(UO.key_of(s[:K]), K), UO.canon(UO.key_of(s[-K:]), K)))
    cases.append(("three arms, equal", h, K, (0, 0, 2 * K - 1), {arms[1]: 3, arms[2]: 3}))
    # islands at and above the limit
    rng = random.Random(23)
    while True:
        at, above, far = rnd(rng, 14), rnd(rng, 15), rnd(rng, 60)
        if clean([at, above, far], K, (14 - K + 2) + (15 - K + 2) + (60 - K + 2)):
            break
    cases.append(("islands at and above the limit", [at, above, far], K, (14, 0, 0), {at: 1}))
    return cases


def closed_table(rng, n, K):
    """The table of a closed sequence of n bases whose n k-mers form one closed chain."""
    while True:
        s = rnd(rng, n)
        c = (s * ((n + K - 1) // n + 1))[:n + K - 1]
        if clean([c[:n + K - 2]], K, n):
            return UO.table([c], K)


def quiet_cases():
    """Graphs with self arcs, arcs onto the other strand and palindromic nodes: every rule is on with wide limits, nothing
    goes and nothing is raised.  (name, ents, K)"""
    return [("closed", closed_table(random.Random(5), 40, 7), 7), ("homopolymer", UO.table(["A" * 60], 21), 21),
            ("hairpin", UO.table(["AT" * 30], 21), 21), ("palindrome", UO.table(["AT" * 30], 20), 20)]


def limit_case():
    """An island, a tip and a bubble in one graph: (sequences, K, {rule index: expect})."""
    K = 9
    rng = random.Random(31)
    h = snp(33, K, 2, 6 * K)
    while True:
        isl = rnd(rng, K + 2)
        p = 3 * K
        tip = h[0][p - K + 1:p] + other(h[0][p]) + rnd(rng, 2)
        seqs = [h[0], h[0], h[1], isl, tip]
        if clean(seqs, K, 2 * (6 * K - K + 2) + 2 * (K - 1) + 4 + 3):
            break
    return seqs, K, {0: {isl: 1}, 1: {tip: 2}, 2: {h[1][6 * K - (K - 1):6 * K + K]: 3}}


# ---- the first-principles case ----

def genome(rng, K, n=1500):
    """n random bases with no repeated canonical (K-1)-mer."""
    while True:
        g = rnd(rng, n)
        if clean([g], K, n - K + 2):
            return g


def reads(rng, g, K, spaced, rlen=200, cov=8, rate=0.5):
    """Reads of rlen bases off g at `cov`x with substitutions; reads within 3K of the genome's ends carry none.
    spaced: a substitution falls only on a genome position that is 0 mod 4K and lies in the read's last K-1 bases (a tip), or
    is 2K mod 4K and lies at least K from both ends of the read (a bubble), each with probability `rate`.
    not spaced: two substitutions per read at uniform positions."""
    out = []
    for _ in range(len(g) * cov // rlen):
        s = rng.randrange(len(g) - rlen + 1)
        r = list(g[s:s + rlen])
        if s >= 3 * K and s + rlen <= len(g) - 3 * K:
            if spaced:
                for p in range(s, s + rlen):
                    q = p - s
                    site = (p % (4 * K) == 0 and q >= rlen - (K - 1)) or (p % (4 * K) == 2 * K and K <= q < rlen - K)
                    if site and rng.random() < rate:
                        r[q] = other(r[q], rng.randrange(1, 4))
            else:
                for q in rng.sample(range(rlen), 2):
                    r[q] = other(r[q], rng.randrange(1, 4))
        out.append("".join(r))
    return out


def read_set(seed, K, spaced):
    """(genome, the sequences the table is made of: the genome three times and the reads)."""
    rng = random.Random(1000 * K + seed)
    g = genome(rng, K)
    return g, [g] * 3 + reads(rng, g, K, spaced)

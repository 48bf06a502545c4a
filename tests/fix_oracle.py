"""Brute-force restatement of "Fixing reads from a k-mer table" (include/classpro_amd.h) by plain loops: the gaps of a
read, the candidate edits of a closed gap in their fixed order, acceptance, the status of a gap, the clash rule and the pass
that applies the fixes; a genome with homopolymers and tandem repeats and reads over it with spaced errors of every kind
the rule undoes; and the line and files `tabfix` leaves.  Test helper; nothing of the product is imported."""
import random

import readhits_oracle as RO
import tabprof_oracle as TO

NONE, ONE, MANY, OPEN, NOCAND, CLASH = range(6)
STATUS = ("none", "one", "many", "open", "nocand", "clash")
ACGT = b"ACGT"


def marks_of(seq, K, present, canonical=True):
    """Per k-mer position 'A' (present), '.' (absent) or 'o' (a byte other than A C G T)."""
    return RO.markers(seq, K, present, set(), canonical)


def gaps_of(marks):
    """[(i, j, closed)]: the maximal runs of '.', closed when both neighbouring positions exist and are present."""
    out, P, p = [], len(marks), 0
    while p < P:
        if marks[p] != ".":
            p += 1
            continue
        q = p
        while q + 1 < P and marks[q + 1] == ".":
            q += 1
        out.append((p, q, p >= 1 and q <= P - 2 and marks[p - 1] == "A" and marks[q + 1] == "A"))
        p = q + 1
    return out


def candidates(s, K, i, j, D):
    """[(del, ins)] of the closed gap [i, j] of s in the fixed order of the rule; those with e + del > len(s) left out."""
    e = i + K - 1
    g = (j - i + 1) - K + 1
    t = -g
    out = []
    if g >= 1:
        out += [(d, b"") for d in range(g, D + 1)]
        if g == 1:
            out += [(1, bytes([c])) for c in ACGT if c != s[e]]
    else:
        out += [(d, b"") for d in range(1, D + 1)]
        if D >= 1:
            out += [(0, bytes([c])) for c in ACGT]
        out += [(0, bytes(s[e - d:e])) for d in range(2, min(D, t) + 1)]
    return [(d, ins) for d, ins in out if e + d <= len(s)]


def edited(s, e, d, ins):
    return bytes(s[:e]) + ins + bytes(s[e + d:])


def accepted(s, K, i, d, ins, present, canonical=True):
    e = i + K - 1
    c = edited(s, e, d, ins)
    lo, hi = max(i, 0), min(e + len(ins) - 1 if ins else e - 1, len(c) - K)
    if hi < lo:
        return False
    return all(k is not None and k in present for k in TO.read_keys(c[lo:hi + K], K, canonical))


def fixes_of(s, K, D, present, canonical=True):
    """[[first, last, status, del, nins, nacc, ins]] of one read, the clash rule applied."""
    recs = []
    for i, j, closed in gaps_of(marks_of(s, K, present, canonical)):
        if not closed:
            recs.append([i, j, OPEN, 0, 0, 0, b""])
            continue
        cand = candidates(s, K, i, j, D)
        acc = [c for c in cand if accepted(s, K, i, c[0], c[1], present, canonical)]
        if not cand:
            recs.append([i, j, NOCAND, 0, 0, 0, b""])
        elif len(acc) == 1:
            recs.append([i, j, ONE, acc[0][0], len(acc[0][1]), 1, acc[0][1]])
        else:
            recs.append([i, j, MANY if acc else NONE, 0, 0, len(acc), b""])
    before = [r[2] for r in recs]
    for k, r in enumerate(recs):
        if before[k] != ONE:
            continue
        e = r[0] + K - 1
        if k > 0 and before[k - 1] == ONE and e < recs[k - 1][0] + K - 1 + recs[k - 1][3]:
            r[2] = CLASH
        if k + 1 < len(recs) and before[k + 1] == ONE and e + r[3] > recs[k + 1][0] + K - 1:
            r[2] = CLASH
    return recs


def read_fixes(ents, seqs, K, D=1, canonical=True, count_range=None):
    """(fix_off, [(first, last, read, status, del, nins, nacc, ins padded to 8 bytes)], tally by status) of a batch."""
    present = RO.present(ents, count_range)
    off, out, tally = [0], [], [0] * 6
    for r, s in enumerate(seqs):
        for first, last, status, d, nins, nacc, ins in fixes_of(s, K, D, present, canonical):
            out.append((first, last, r, status, d, nins, nacc, ins + bytes(8 - len(ins))))
            tally[status] += 1
        off.append(len(out))
    return off, out, tally


def apply_one(s, recs, K):
    """The read with its ONE records applied; recs are (first, last, read, status, del, nins, nacc, ins)."""
    out, at = b"", 0
    for first, _last, _r, status, d, nins, _n, ins in recs:
        if status != ONE:
            continue
        e = first + K - 1
        assert e >= at                                     # disjoint and ascending
        out += bytes(s[at:e]) + ins[:nins]
        at = e + d
    return out + bytes(s[at:])


def apply(seqs, fix_off, recs, K):
    return [apply_one(s, recs[fix_off[r]:fix_off[r + 1]], K) for r, s in enumerate(seqs)]


def none_count(seqs, K, present, canonical=True):
    return sum(marks_of(s, K, present, canonical).count(".") for s in seqs)


# ---- a genome and reads with spaced errors ----

def genome(seed, n=30000):
    """Random bases with homopolymers of 2 to 9 bases and tandem repeats of 2 to 3 bases times 2 to 5 copies sprinkled in."""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        x = rng.random()
        if x < 0.03:
            out += bytes([rng.choice(ACGT)]) * rng.randint(2, 9)
        elif x < 0.05:
            out += bytes(rng.choice(ACGT) for _ in range(rng.randint(2, 3))) * rng.randint(2, 5)
        else:
            out.append(rng.choice(ACGT))
    return bytes(out[:n])


KINDS1 = ("sub", "ins", "del", "hp+", "hp-")               # what D = 1 undoes
KINDS3 = ("sub", "ins", "del", "tandem+", "tandem-")       # D = 2 and 3: insertions of 1..D bases, whole repeat units


def run_at(t, p):
    """(start, length) of the homopolymer run of t that holds p."""
    a = b = p
    while a > 0 and t[a - 1] == t[p]:
        a -= 1
    while b + 1 < len(t) and t[b + 1] == t[p]:
        b += 1
    return a, b - a + 1


def tandem_at(t, p, D):
    """(unit, copies) of a tandem repeat of unit 2..D that begins at p, the longest unit first; None without one."""
    for u in range(min(D, 3), 1, -1):
        unit = t[p:p + u]
        if len(unit) < u or len(set(unit)) == 1:
            continue
        c = 1
        while t[p + c * u:p + (c + 1) * u] == unit:
            c += 1
        if c >= 2:
            return u, c
    return None


def spoil(rng, t, K, D, kinds, space=None):
    """t with one error every `space` (3K) bases, the kinds in turn; [(kind, position in t)] beside it.  An error the
    site does not allow (no run, no repeat) becomes a substitution."""
    space = 3 * K if space is None else space
    out, at, log, n = bytearray(), 0, [], 0
    for p in range(space, len(t) - space, space):
        kind = kinds[n % len(kinds)]
        n += 1
        out += t[at:p]
        at = p
        if kind == "hp+" or kind == "hp-":
            a, h = run_at(t, p)
            if kind == "hp+" and a + h <= p + 1:
                out += t[p:p + 1] * 2
                at = p + 1
            elif kind == "hp-" and h >= 2 and a == p:
                at = p + 1
            else:
                kind = "sub"
        elif kind == "tandem+" or kind == "tandem-":
            rep = tandem_at(t, p, D)
            if rep and kind == "tandem+":
                out += t[p:p + rep[0]]
            elif rep and rep[1] > D:
                at = p + rep[0]
            else:
                kind = "sub"
        if kind == "ins":
            out += bytes(rng.choice(ACGT) for _ in range(rng.randint(1, D)))
        elif kind == "del":
            at = p + 1
        elif kind == "sub":
            out.append(rng.choice([c for c in ACGT if c != t[p]]))
            at = p + 1
        log.append((kind, p))
    return bytes(out + t[at:]), log


def read_set(seed, K, D, kinds, nreads=40, rlen=None, glen=30000, space=None):
    """(genome, true pieces, the pieces with spaced errors, the kinds that were made)."""
    rng = random.Random(seed * 7919 + K)
    g = genome(seed, glen)
    rlen = 40 * K if rlen is None else rlen
    truth, reads, made = [], [], set()
    for _ in range(nreads):
        a = rng.randrange(0, len(g) - rlen)
        t = g[a:a + rlen]
        s, log = spoil(rng, t, K, D, kinds[rng.randrange(len(kinds)):] + kinds, space)
        truth.append(t)
        reads.append(s)
        made |= {k for k, _ in log}
    return g, truth, reads, made


def table(seqs, K, canonical=True):
    """[(key, count)] ascending: the k-mers of upper-case A C G T of seqs."""
    cnt = {}
    for s in seqs:
        for k in TO.read_keys(s, K, canonical):
            if k is not None:
                cnt[k] = cnt.get(k, 0) + 1
    return sorted(cnt.items())


# ---- the command ----

def tabfix(ents, names, seqs, K, D=1, count_range=None):
    """(the summary line, the bytes of <out_root>.fixed.fasta, the bytes of <out_root>.fixes.tsv) of `tabfix -d<D>` over
    reads named `names` in a FASTA without comments: the header of such a read is "<name> (null)"."""
    off, recs, tally = read_fixes(ents, seqs, K, D, True, count_range)
    fixed = apply(seqs, off, recs, K)
    fasta, tsv, kinds = b"", b"", [0, 0, 0]
    for r, (name, s) in enumerate(zip(names, seqs)):
        fasta += b">" + ("%s (null)" % name).encode() + b"\n" + fixed[r] + b"\n"
        for first, _l, _r, status, d, nins, _n, ins in recs[off[r]:off[r + 1]]:
            if status != ONE:
                continue
            e = first + K - 1
            kinds[0 if d == nins else 1 if d > nins else 2] += 1
            tsv += ("%s\t%d\t" % (name, e)).encode() + bytes(s[e:e + d]) + b"\t" + ins[:nins] + b"\n"
    line = ("tabfix: %d sequences, %d gaps, %d fixed (%d substitutions, %d insertions removed, %d deletions filled), "
            "%d ambiguous, %d unfixed, %d open, %d without candidate, %d clashes\n"
            % (len(seqs), sum(tally), tally[ONE], kinds[0], kinds[1], kinds[2], tally[MANY], tally[NONE], tally[OPEN],
               tally[NOCAND], tally[CLASH]))
    return line, fasta, tsv

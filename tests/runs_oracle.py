"""Brute-force restatement of "Runs of k-mer states along reads" (include/classpro_amd.h) over the marker strings of
tests/readhits_oracle.py: the runs of a read by a plain loop, the blocks of a read's runs, the block N50, and the lines
and files `tabtrack` leaves in both modes.  Test helper; nothing of the product is imported."""
import math

import readhits_oracle as RO

NONE, A, B, BOTH, OTHER = range(5)
STATE = {".": NONE, "A": A, "B": B, "2": BOTH, "o": OTHER}
ALL = 0x1f
PHASE_SKIP, PHASE_EMIT = 1 << NONE | 1 << BOTH | 1 << OTHER, 1 << A | 1 << B


def runs(marks, skip=0, emit=None):
    """[(state, first, last, n)] of one read's marker string; `skip` and `emit` are masks of 1 << state."""
    emit = ALL & ~skip if emit is None else emit
    out, cur = [], None
    for i, m in enumerate(marks):
        s = STATE[m]
        if skip >> s & 1:
            continue
        if cur is not None and cur[0] == s:
            cur[2], cur[3] = i, cur[3] + 1
        else:
            cur = [s, i, i, 1]
            out.append(cur)
    return [tuple(r) for r in out if emit >> r[0] & 1]


def blocks(rs, min_n=1):
    """(blocks, dropped) of the runs of one read: those with n < min_n dropped, equal neighbours of the rest merged."""
    out, dropped = [], 0
    for s, first, last, n in rs:
        if n < min_n:
            dropped += 1
        elif out and out[-1][0] == s:
            out[-1][2], out[-1][3] = last, out[-1][3] + n
        else:
            out.append([s, first, last, n])
    return [tuple(b) for b in out], dropped


def n50(spans):
    """The largest s such that the spans >= s sum to at least half of the sum of all; 0 without spans."""
    total = sum(spans)
    for s in sorted(set(spans), reverse=True):
        if 2 * sum(x for x in spans if x >= s) >= total:
            return s
    return 0


def qv_text(K, missing, valid):
    if valid <= 0:
        return "-"
    if missing == 0:
        return "inf"
    return "%.4f" % (-10.0 * math.log10(1.0 - math.pow(1.0 - missing / valid, 1.0 / K)))


def marks_of(a, b, seqs, K, canonical=True, a_range=None, b_range=None, keys=None):
    in_a, in_b = RO.present(a, a_range), RO.present(b, b_range) if b is not None else set()
    keys = [None] * len(seqs) if keys is None else keys
    return [RO.markers(s, K, in_a, in_b, canonical, ks) for s, ks in zip(seqs, keys)]


def read_runs(a, b, seqs, K, skip=0, emit=None, canonical=True, a_range=None, b_range=None, keys=None):
    """(run_off, [(first, last, n, read, state)]) of a batch, as SortedKmers.read_runs returns them."""
    off, out = [0], []
    for r, m in enumerate(marks_of(a, b, seqs, K, canonical, a_range, b_range, keys)):
        out += [(first, last, n, r, s) for s, first, last, n in runs(m, skip, emit)]
        off.append(len(out))
    return off, out


def headers_of(names):
    """The .class headers, without their '@', of reads named `names` in a FASTA without comments."""
    return ["%s (null)" % name for name in names]


def absence(a, headers, seqs, K, a_range=None):
    """(stdout, the summary line of stderr, the bytes of <out_root>.missing.bed) of `tabtrack <A> <source>` over reads
    with the given .class headers (without '@'); the name in the BED file is the header up to its first blank."""
    out, bed, tot = [], [], [0, 0, 0]
    for i, (header, s, m) in enumerate(zip(headers, seqs, marks_of(a, None, seqs, K, True, a_range))):
        name = header.split(" ")[0]
        rs = runs(m)
        valid = sum(n for st, _, _, n in rs if st != OTHER)
        miss = [r for r in rs if r[0] == NONE]
        missing = sum(r[3] for r in miss)
        bed += ["%s\t%d\t%d\t%d\n" % (name, first, last + K, n) for _, first, last, n in miss]
        out.append("%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % (i + 1, len(s), valid, missing, len(miss), qv_text(K, missing, valid), header))
        tot = [tot[0] + valid, tot[1] + missing, tot[2] + len(miss)]
    summary = "tabtrack: %d sequences, %d k-mers, %d missing in %d runs, QV %s\n" % (len(seqs), tot[0], tot[1], tot[2],
                                                                                   qv_text(K, tot[1], tot[0]))
    return "".join(out), summary, "".join(bed).encode()


def phase(a, b, headers, seqs, K, a_range=None, b_range=None, min_n=1):
    """The same of `tabtrack [-m<min_n>] <A> <B> <source>`, the file being <out_root>.blocks.bed."""
    out, bed, spans, tot = [], [], [], [0] * 5
    for i, (header, s, m) in enumerate(zip(headers, seqs, marks_of(a, b, seqs, K, True, a_range, b_range))):
        name = header.split(" ")[0]
        rs = runs(m, PHASE_SKIP, PHASE_EMIT)
        bl, dropped = blocks(rs, min_n)
        na, nb = (sum(n for st, _, _, n in rs if st == side) for side in (A, B))
        mine = [last + K - first for _, first, last, _ in bl]
        bed += ["%s\t%d\t%d\t%s\t%d\n" % (name, first, last + K, "AB"[st - 1], n) for st, first, last, n in bl]
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (i + 1, len(s), na, nb, len(rs), dropped, len(bl), sum(mine), header))
        spans += mine
        tot = [x + y for x, y in zip(tot, (na, nb, len(rs), dropped, len(bl)))]
    summary = ("tabtrack: %d sequences, %d A and %d B markers, %d runs, %d dropped, %d blocks, block N50 %d\n"
               % ((len(seqs),) + tuple(tot) + (n50(spans),)))
    return "".join(out), summary, "".join(bed).encode()

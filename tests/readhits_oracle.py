"""Brute-force restatement of "Read hits in two sorted k-mer sets" (include/classpro_amd.h) over dicts: two tables as
[(key, count)] lists, a marker per k-mer position of a read, the row of a read by a plain loop, the call of a row, and
the lines and files `tabbin` leaves.  Test helper; nothing of the product is imported."""
import tabprof_oracle as TO

BIG = (1 << 63) - 1


def present(ents, rng):
    """The keys of a table whose count lies in the range (lo, hi), either end None for open."""
    lo, hi = (None, None) if rng is None else rng
    lo, hi = 1 if lo is None else lo, BIG if hi is None else hi
    return {k for k, c in ents if lo <= c <= hi}


def markers(seq, K, in_a, in_b, canonical=True, keys=None):
    """Per k-mer position: 'A', 'B', '2' (both), 'o' (another byte) or '.' (no marker); `keys` is
    TO.read_keys(seq, K, canonical) when the caller has it already."""
    out = []
    for key in TO.read_keys(seq, K, canonical) if keys is None else keys:
        if key is None:
            out.append("o")
        elif key in in_a:
            out.append("2" if key in in_b else "A")
        else:
            out.append("B" if key in in_b else ".")
    return "".join(out)


def row_of(marks):
    """[nA, nB, nBoth, nOther, switches] of one read's marker string."""
    switches, last = 0, None
    for m in marks:
        if m in "AB":
            if last is not None and last != m:
                switches += 1
            last = m
    return [marks.count("A"), marks.count("B"), marks.count("2"), marks.count("o"), switches]


def rows(a, b, seqs, K, canonical=True, a_range=None, b_range=None, keys=None):
    """The rows of a batch; `keys` is TO.keys_of(seqs, K, canonical) when the caller has it already."""
    in_a, in_b = present(a, a_range), present(b, b_range)
    keys = [None] * len(seqs) if keys is None else keys
    return [row_of(markers(s, K, in_a, in_b, canonical, ks)) for s, ks in zip(seqs, keys)]


def only(a, b, a_range=None, b_range=None):
    """(keys only in A, keys only in B) after the ranges: the sizes of the two marker sets."""
    in_a, in_b = present(a, a_range), present(b, b_range)
    return len(in_a - in_b), len(in_b - in_a)


def call(row, only_a, only_b, min_markers=1, normalise=True):
    na, nb = row[0], row[1]
    if na + nb < min_markers:
        return "U"
    wa, wb = (only_a, only_b) if normalise and only_a > 0 and only_b > 0 else (1, 1)
    return "A" if na * wb > nb * wa else "B" if nb * wa > na * wb else "U"


def tabbin(a, b, names, seqs, K, a_range=None, b_range=None, min_markers=1, normalise=True):
    """(stdout, the summary line of stderr, {bin: bytes of its FASTA}) of `tabbin` over reads named `names` in a FASTA
    without comments: the .class header of such a read is "@<name> (null)"."""
    oa, ob = only(a, b, a_range, b_range)
    out, fasta, n = [], {"A": b"", "B": b"", "U": b""}, {"A": 0, "B": 0, "U": 0}
    switched = 0
    for i, (name, s, row) in enumerate(zip(names, seqs, rows(a, b, seqs, K, True, a_range, b_range))):
        c = call(row, oa, ob, min_markers, normalise)
        header = "%s (null)" % name
        out.append("\t".join([str(i + 1), str(len(s))] + [str(x) for x in row] + [c, header]) + "\n")
        fasta[c] += b">" + header.encode() + b"\n" + bytes(s) + b"\n"
        n[c] += 1
        switched += row[4] > 0
    summary = "tabbin: %d reads, %d A, %d B, %d U, %d reads with switches\n" % (len(seqs), n["A"], n["B"], n["U"], switched)
    return "".join(out), summary, fasta

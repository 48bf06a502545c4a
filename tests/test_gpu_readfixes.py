"""cp_kmer_sorted_read_fixes and cp_apply_fixes (SortedKmers.read_fixes, .apply_fixes) on a real MI355X (`-m gpu`), against
the plain loops of tests/fix_oracle.py: reads with spaced and with crowded errors over a genome with homopolymers and tandem
repeats for K = 5, 21, 31, 32 and 63 and max_indel = 0, 1, 2 and 4 (K = 63 with 4 has windows of 66 k-mers, the second
round of a wave), a sequence of 50 000 bases with an edit at every edge of a lane's 64 bases, gaps at the ends of reads,
reads shorter than K, empty reads and batches, an empty table, a count range, a forward table, capacity and overflow of
both calls, batching, the tally, the identity with `read_runs`, that table and batch are only read, the argument errors,
and records spoilt by hand.  Everything is integers and bytes: the tolerance is zero."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import fix_oracle as FO
import readhits_oracle as RO
from test_gpu_ktab import flat
from test_gpu_tabprof import load

pytestmark = pytest.mark.gpu
EINVAL, EOVERFLOW = -1, -5
KS = [5, 21, 31, 32, 63]
DS = [0, 1, 2, 4]


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def crowd(rng, t, K, n):
    """t with n errors anywhere: substitutions, insertions and deletions of 1 to 4 bases."""
    s = bytearray(t)
    for _ in range(n):
        p = rng.randrange(len(s))
        kind, m = rng.randrange(3), rng.randint(1, 4)
        if kind == 0:
            s[p] = rng.choice([c for c in FO.ACGT if c != s[p]])
        elif kind == 1:
            s[p:p] = bytes(rng.choice(FO.ACGT) for _ in range(m))
        else:
            del s[p:p + m]
    return bytes(s)


@functools.lru_cache(maxsize=None)
def case(K):
    """(entries of the genome's table, reads): a few hundred reads of at most 400 bases -- spaced errors of every kind,
    crowded errors, errors in the first and last K bases, an N, reads of K-1, K and K+1 bases and empty ones."""
    rng = random.Random(K)
    glen, rlen = (260, 150) if K == 5 else (30000, 400)
    g = FO.genome(K, glen)
    reads = []
    for D, kinds in ((1, FO.KINDS1), (3, FO.KINDS3), (4, FO.KINDS3)):
        reads += FO.read_set(K + D, K, D, kinds, nreads=50, rlen=rlen - 30, glen=glen, space=max(3 * K, 24))[2]
    for _ in range(60):
        a = rng.randrange(len(g) - rlen)
        reads.append(crowd(rng, g[a:a + rlen], K, rng.randint(1, 6))[:400])
    for _ in range(30):                                    # errors that the ends of the read clip or leave open
        a = rng.randrange(len(g) - rlen)
        t = bytearray(g[a:a + rng.randint(K + 2, 3 * K)])
        p = rng.choice([rng.randrange(0, 3), len(t) - 1 - rng.randrange(0, 3), rng.randrange(len(t))])
        t[p] = rng.choice([c for c in FO.ACGT if c != t[p]])
        if rng.random() < 0.5:
            q = rng.randrange(len(t))
            t[q:q] = bytes(rng.choice(FO.ACGT) for _ in range(rng.randint(1, 4)))
        reads.append(bytes(t))
    a = rng.randrange(len(g) - rlen)
    n_read = bytearray(crowd(rng, g[a:a + rlen], K, 2)[:400])
    n_read[len(n_read) // 2] = ord("N")
    reads += [bytes(n_read), g[:K - 1], g[3:3 + K], g[5:6 + K], b"", b"", g[:K][:-1] + b"N"]
    rng.shuffle(reads)
    assert max(len(s) for s in reads) <= 400
    return FO.table([g], K), reads


def records(f):
    cols = [f[k].cpu().tolist() for k in ("first", "last", "read", "status", "del", "nins", "nacc")]
    ins = [bytes(x) for x in f["ins"].cpu().numpy()]
    return list(zip(*cols, ins))


def split(torch, seq, off):
    s, o = seq.cpu().numpy().tobytes(), off.cpu().tolist()
    return [s[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def got(torch, S, seqs, D, **kw):
    """((fix_off, records, tally), corrected reads) of the device."""
    batch = flat(torch, seqs)
    off, f, tally = S.read_fixes(batch, max_indel=D, **kw)
    assert off.dtype == torch.int64 and f["first"].dtype == f["last"].dtype == torch.int64 and f["read"].dtype == torch.int32
    assert all(f[k].dtype == torch.uint8 for k in ("status", "del", "nins", "nacc", "ins"))
    out, out_off = S.apply_fixes(batch, off, f)
    assert out.dtype == torch.uint8 and out_off.dtype == torch.int64 and int(out_off[-1]) == out.numel()
    return (off.cpu().tolist(), records(f), [tally[k] for k in S.FIX_TALLY]), split(torch, out, out_off)


def check(torch, S, ents, seqs, K, D, **kw):
    want = FO.read_fixes(ents, seqs, K, D, **kw)
    have, fixed = got(torch, S, seqs, D, **kw)
    assert have[0] == want[0] and have[2] == want[2], (K, D, kw)
    assert have[1] == want[1], (K, D, kw, next(x for x in zip(have[1], want[1]) if x[0] != x[1]))
    assert fixed == FO.apply(seqs, want[0], want[1], K), (K, D, kw)
    return want


# ---- 1. every K and D ----

@pytest.mark.parametrize("K", KS)
def test_against_the_oracle(torch_dev, K):
    torch = torch_dev
    ents, seqs = case(K)
    S = load(torch, ents, K)
    seen = set()
    for D in DS:
        off, recs, tally = check(torch, S, ents, seqs, K, D)
        seen |= {r[3] for r in recs}
        assert tally[FO.ONE] > 10 and tally[FO.OPEN] > 10
        if D == 0:
            assert all(r[4:6] == (1, 1) for r in recs if r[3] == FO.ONE) and tally[FO.NOCAND] > 50
        if D == 4:
            assert {(r[4] > 0, r[5] > 0) for r in recs if r[3] == FO.ONE} == {(True, True), (True, False), (False, True)}
            assert max(r[4] for r in recs) >= 3 and max(r[5] for r in recs) >= 2
    assert {FO.NONE, FO.ONE, FO.OPEN, FO.NOCAND} <= seen and (K != 5 or FO.MANY in seen)
    S.close()


def test_statuses_written_out(torch_dev):
    """The hand cases of tests/test_fix_host.py on the device: every status, the clash with D = 3."""
    torch = torch_dev
    import test_fix_host as H
    for name, K, D, table_seqs, s, want in H.HAND:
        ents = FO.table(table_seqs, K)
        S = load(torch, ents, K)
        (off, recs, tally), fixed = got(torch, S, [s], D)
        assert [(r[0], r[1], r[3], r[4], r[6], r[7].rstrip(b"\0")) for r in recs] == want, name
        assert fixed == FO.apply([s], *FO.read_fixes(ents, [s], K, D)[:2], K), name
        S.close()


# ---- 2. a long sequence: the copy kernel and the scan across lanes and blocks ----

def long_case(K, D, n=50000):
    """(truth, a sequence with one error at every multiple of 64 of its OWN coordinates, six kinds in turn by m = position / 64:
    a substitution of base 64m, two bases inserted before 64m-2, two inserted before 64m-1, a base lost before 64m, two
    inserted before 64m, a base lost before 64m-1).  A fix has its e where the error is, so as the FIRST read of a batch the
    sequence has fixes that begin on a lane's first base, fixes on a lane's last two bases whose removed bases end at or
    reach over the edge into the next lane's chunk, and at the block edges 16384, 32768 and 49152 (m = 256, 512, 768) an
    insertion on the block's first base, a removal that reaches over the edge, and a substitution of the first base."""
    rng = random.Random(n + K)
    g = FO.genome(7, n + 2000)
    where = (0, -2, -1, 0, 0, -1)
    out, at, m = bytearray(), 0, 1
    while len(out) < n:
        kind = m % 6
        step = 64 * m + where[kind] - len(out)
        out += g[at:at + step]
        at += step
        if kind == 0:
            out.append(rng.choice([c for c in FO.ACGT if c != g[at]]))
            at += 1
        elif kind in (1, 2, 4):
            out += bytes(rng.choice(FO.ACGT) for _ in range(2))
        else:
            at += 1
        m += 1
    out += g[at:at + 3 * K]
    return g[:at + 3 * K], bytes(out)


def test_a_long_sequence(torch_dev):
    """The copy kernel and the offset scan across lanes and blocks: a lane owns 64 bases of the BATCH, so the places below
    are taken in batch coordinates, seq_off[read] + e."""
    torch = torch_dev
    K, D = 21, 2
    truth, s = long_case(K, D)
    assert len(s) >= 50000
    ents = FO.table([truth], K)
    S = load(torch, ents, K)
    seqs = [s, b"ACGTACGTAC", b"", s[:20000]]              # the second copy begins 10 bases behind a lane's edge
    off, recs, tally = check(torch, S, ents, seqs, K, D)
    start = [0]
    for x in seqs:
        start.append(start[-1] + len(x))
    assert start[1] > 3 * 16384 and start[3] % 64 == 10
    one = [(start[r[2]] + r[0] + K - 1, r[4], r[5]) for r in recs if r[3] == FO.ONE]   # (e in the batch, del, nins)
    assert tally[FO.ONE] > 0.9 * sum(tally) and len(one) > 900
    first = [x for x in one if x[0] % 64 == 0]             # the edit begins on a lane's first base
    assert sum(d > 0 for _, d, _ in first) > 100 and sum(ni > 0 and d == 0 for _, d, ni in first) > 50
    over = [x for x in one if x[1] >= 2 and x[0] % 64 == 63]                            # removed bases reach into the next lane's chunk
    upto = [x for x in one if x[1] >= 2 and x[0] % 64 == 62]                            # removed bases end at the edge
    assert len(over) > 50 and len(upto) > 50
    assert sum(x[0] % 64 == 63 and x[1] == 0 for x in one) > 50                         # an insertion before a lane's last base
    block = {(x[0] // 16384, x[0] % 16384): x for x in one if x[0] % 16384 in (0, 16383)}
    assert block[(1, 0)][1] == 2 and block[(1, 16383)][1] == 2 and block[(3, 0)][1:] == (1, 1)   # at the block edges too
    S.close()


# ---- 3. the presence rule ----

def test_count_range_and_forward_table(torch_dev):
    torch = torch_dev
    K = 21
    _, seqs = case(K)
    ents = FO.table(seqs, K)                               # the reads' own table: errors are the rare k-mers
    S = load(torch, ents, K)
    a = check(torch, S, ents, seqs, K, 1)
    b = check(torch, S, ents, seqs, K, 1, count_range=(3, None))
    c = check(torch, S, ents, seqs, K, 2, count_range=(2, 40))
    assert a[2][FO.ONE] < b[2][FO.ONE] and a != b and b != c
    S.close()
    fents = FO.table([FO.genome(K, 30000)], K, canonical=False)
    F = load(torch, fents, K)
    d = check(torch, F, fents, seqs, K, 2, canonical=False)
    e = check(torch, F, fents, seqs, K, 2, canonical=True)
    assert d != e and d[2][FO.ONE] > 50
    F.close()


def test_empty_things(torch_dev):
    torch = torch_dev
    K = 21
    ents, seqs = case(K)
    S, E = load(torch, ents, K), load(torch, [], K)
    off, recs, tally = check(torch, E, [], seqs, K, 2)     # an empty table: every read with a k-mer is one open gap
    assert tally[FO.OPEN] == len(recs) > 100 and sum(tally) == len(recs)
    for T in (S, E):
        off, f, tally = T.read_fixes(flat(torch, []))      # nreads == 0
        assert off.cpu().tolist() == [0] and f["first"].numel() == 0 and f["ins"].shape == (0, 8) and not any(tally.values())
        out, out_off = T.apply_fixes(flat(torch, []), off, f)
        assert out.numel() == 0 and out_off.cpu().tolist() == [0]
        few = [b"", b"ACG", b"", b"ACGTACGTACGTACGTACGT"]   # no k-mer position at all
        (o, r, t), fixed = got(torch, T, few, 1)
        assert (o, r, t, fixed) == ([0] * 5, [], [0] * 6, few)
    S.close()
    E.close()


# ---- 4. capacity ----

def raw_fixes(torch, L, S, seq, off, n, total, D, cap, tally=None, rng=None, poison=-7):
    buf = torch.full((max(cap, 0) + 3, 4), poison, dtype=torch.int64, device="cuda:0")
    foff = torch.full((n + 1,), poison, dtype=torch.int64, device="cuda:0")
    count = C.c_int64(-1)
    rc = L.cp_kmer_sorted_read_fixes(S.s, 1, rng, D, seq.data_ptr(), off.data_ptr(), n, total, buf.data_ptr() if cap > 0 else None,
                                     cap, foff.data_ptr(), C.byref(count), tally.data_ptr() if tally is not None else None, None)
    torch.cuda.synchronize()
    return rc, count.value, foff.cpu().tolist(), buf


def rows_of(recs):
    """The records as the four int64 words of a cp_kmer_fix."""
    out = []
    for first, last, read, status, d, nins, nacc, ins in recs:
        out.append([first, last, read | status << 32 | d << 40 | nins << 48 | nacc << 56, int.from_bytes(ins, "little")])
    return out


def test_capacity_and_tally(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K, D = 21, 2
    ents, seqs = case(K)
    S = load(torch, ents, K)
    seq, off = flat(torch, seqs)
    n, total = len(seqs), int(off[-1])
    want_off, want, want_tally = FO.read_fixes(ents, seqs, K, D)
    t, rows = len(want), rows_of(want)
    assert t > 300
    tally = torch.tensor([5, 0, 7, 0, 0, 1], dtype=torch.int64, device="cuda:0")
    rc, count, foff, buf = raw_fixes(torch, L, S, seq, off, n, total, D, 0, tally)      # the counting call
    assert (rc, count, foff) == (EOVERFLOW, t, want_off) and tally.cpu().tolist() == [5, 0, 7, 0, 0, 1]
    rc, count, foff, buf = raw_fixes(torch, L, S, seq, off, n, total, D, t, tally)      # the exact call
    assert (rc, count, foff) == (0, t, want_off)
    assert buf[:t].cpu().tolist() == rows and bool((buf[t:] == -7).all())
    assert tally.cpu().tolist() == [x + y for x, y in zip([5, 0, 7, 0, 0, 1], want_tally)]     # added to
    for cap in (t - 1, t // 2):                            # too small: exact offsets and total, no record, nothing added
        rc, count, foff, buf = raw_fixes(torch, L, S, seq, off, n, total, D, cap, tally)
        assert (rc, count, foff) == (EOVERFLOW, t, want_off) and bool((buf == -7).all())
    assert tally.cpu().tolist() == [x + y for x, y in zip([5, 0, 7, 0, 0, 1], want_tally)]
    _, f, _ = S.read_fixes((seq, off), max_indel=D, capacity=3)                         # the wrapper asks again
    assert records(f) == want
    # cp_apply_fixes: exact capacity, one short
    rec = torch.tensor(rows, dtype=torch.int64, device="cuda:0")
    fo = torch.tensor(want_off, dtype=torch.int64, device="cuda:0")
    fixed = FO.apply(seqs, want_off, want, K)
    new_off = [0]
    for x in fixed:
        new_off.append(new_off[-1] + len(x))
    m = new_off[-1]
    assert m != total
    for cap in (m, m - 1):
        out = torch.full((m + 64,), 35, dtype=torch.uint8, device="cuda:0")
        ooff = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
        count = C.c_int64(-1)
        rc = L.cp_apply_fixes(seq.data_ptr(), off.data_ptr(), n, total, K, rec.data_ptr(), fo.data_ptr(), out.data_ptr(), cap,
                              ooff.data_ptr(), C.byref(count), None)
        torch.cuda.synchronize()
        assert (rc, count.value, ooff.cpu().tolist()) == (0 if cap == m else EOVERFLOW, m, new_off)
        o = out.cpu().numpy().tobytes()
        assert o == (b"".join(fixed) if cap == m else b"#" * m) + b"#" * 64
    S.close()


# ---- 5. batching ----

def test_batching_and_order(torch_dev):
    torch = torch_dev
    K, D = 31, 2
    ents, seqs = case(K)
    S = load(torch, ents, K)
    (off, whole, tally), fixed = got(torch, S, seqs, D)
    per = [[x[:2] + x[3:] for x in whole[off[i]:off[i + 1]]] for i in range(len(seqs))]
    parts, at = [], 0
    for size in (1, 7, 100, 3, len(seqs)):
        piece = seqs[at:at + size]
        at += size
        if piece:
            (o, r, t), fx = got(torch, S, piece, D)
            parts.append(([[x[:2] + x[3:] for x in r[o[i]:o[i + 1]]] for i in range(len(piece))], t, fx))
    assert [x for p in parts for x in p[0]] == per and [x for p in parts for x in p[2]] == fixed
    assert [sum(p[1][k] for p in parts) for k in range(6)] == tally
    (o, r, t), fx = got(torch, S, seqs[::-1], D)
    assert [[x[:2] + x[3:] for x in r[o[i]:o[i + 1]]] for i in range(len(seqs))] == per[::-1] and fx == fixed[::-1] and t == tally
    S.close()


# ---- 6. against code that exists; the inputs are only read ----

def test_against_read_runs_and_only_read(torch_dev):
    torch = torch_dev
    K = 32
    ents, seqs = case(K)
    S = load(torch, ents, K)
    seq, off = flat(torch, seqs)
    before = [x.clone() for x in S.ktab()] + [seq.clone(), off.clone()]
    for kw in ({}, dict(count_range=(1, 1)), dict(canonical=False)):
        roff, runs = S.read_runs(None, (seq, off), skip=0, emit=1 << 0, canonical=kw.get("canonical", True), a_range=kw.get("count_range"))
        foff, f, _ = S.read_fixes((seq, off), max_indel=4, **kw)
        assert torch.equal(roff, foff) and all(torch.equal(runs[k], f[k]) for k in ("first", "last", "read"))
        assert bool((runs["n"] == f["last"] - f["first"] + 1).all()) and f["first"].numel() > 100
        S.apply_fixes((seq, off), foff, f)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, list(S.ktab()) + [seq, off]))
    S.close()


# ---- 7. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import ClassProError, lib
    import ktab_oracle as KO
    L = lib()
    K = 21
    ents, seqs = case(K)
    S = load(torch, ents, K)
    seq, off = flat(torch, seqs)
    n, total = len(seqs), int(off[-1])
    cap = 1 << 12
    buf = torch.full((cap, 4), -7, dtype=torch.int64, device="cuda:0")
    foff = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    tally = torch.full((6,), -7, dtype=torch.int64, device="cuda:0")
    count = C.c_int64(-7)
    Q, O, R, F, T = seq.data_ptr(), off.data_ptr(), buf.data_ptr(), foff.data_ptr(), tally.data_ptr()
    go = lambda s, rng, D, q, o, nr, tb, r, c, f, t=C.byref(count): L.cp_kmer_sorted_read_fixes(s, 1, rng, D, q, o, nr, tb, r, c, f, t, T, None)
    r2 = lambda *v: (C.c_int64 * 2)(*v)
    h = C.c_void_p()                                       # a snapshot that is still being loaded
    assert L.cp_kmer_sorted_load_begin(K, KO.index(ents, K).ctypes.data, C.byref(h)) == 0
    bad = [(None, None, 1, Q, O, n, total, R, cap, F), (h, None, 1, Q, O, n, total, R, cap, F),
           (S.s, None, -1, Q, O, n, total, R, cap, F), (S.s, None, 5, Q, O, n, total, R, cap, F),
           (S.s, r2(0, 5), 1, Q, O, n, total, R, cap, F), (S.s, r2(3, 2), 1, Q, O, n, total, R, cap, F),
           (S.s, None, 1, Q, O, -1, total, R, cap, F), (S.s, None, 1, Q, O, n, -1, R, cap, F), (S.s, None, 1, Q, O, n, total, R, -1, F),
           (S.s, None, 1, None, O, n, total, R, cap, F), (S.s, None, 1, Q, None, n, total, R, cap, F),
           (S.s, None, 1, Q, O, n, total, None, cap, F), (S.s, None, 1, Q, O, n, total, R, cap, None),
           (S.s, None, 1, Q, O, n, total, R, cap, F, None)]
    for args in bad:
        assert go(*args) == EINVAL, args
        assert b"cp_kmer_sorted_read_fixes" in L.cp_last_error()
    L.cp_kmer_sorted_destroy(h)
    out = torch.full((total + 4 * cap,), 35, dtype=torch.uint8, device="cuda:0")
    ooff = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    ap = lambda q, o, nr, tb, k, r, f, d, c, oo, t=C.byref(count): L.cp_apply_fixes(q, o, nr, tb, k, r, f, d, c, oo, t, None)
    D_, OO = out.data_ptr(), ooff.data_ptr()
    zoff = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
    Z = zoff.data_ptr()
    for args in ((Q, O, -1, total, K, R, Z, D_, total, OO), (Q, O, n, -1, K, R, Z, D_, total, OO), (Q, O, n, total, 4, R, Z, D_, total, OO),
                 (Q, O, n, total, 64, R, Z, D_, total, OO), (Q, O, n, total, K, R, Z, D_, -1, OO), (None, O, n, total, K, R, Z, D_, total, OO),
                 (Q, None, n, total, K, R, Z, D_, total, OO), (Q, O, n, total, K, R, None, D_, total, OO),
                 (Q, O, n, total, K, R, Z, None, total, OO), (Q, O, n, total, K, R, Z, D_, total, None),
                 (Q, O, n, total, K, R, Z, D_, total, OO, None)):
        assert ap(*args) == EINVAL, args
        assert b"cp_apply_fixes" in L.cp_last_error()
    torch.cuda.synchronize()
    assert all(bool((x == -7).all()) for x in (buf, foff, tally, ooff)) and bool((out == 35).all()) and count.value == -7
    assert go(S.s, None, 1, None, None, 0, 0, None, 0, None) == 0 and count.value == 0  # no reads: no work, no error
    assert go(S.s, r2(1, 1), 4, Q, O, n, total, R, cap, F) == 0
    want_off, want, _ = FO.read_fixes(ents, seqs, K, 4, count_range=(1, 1))
    assert foff.cpu().tolist() == want_off and buf[:len(want)].cpu().tolist() == rows_of(want)
    with pytest.raises(ClassProError):
        S.read_fixes((seq, off), max_indel=5)
    from test_gpu_ktab import table_of
    T4 = table_of(torch, [b"ACGTTGCAAGGCTTAACC"], 4)       # a snapshot of 4-mers: a candidate needs the five bases s[e-4 .. e]
    S4 = T4.sorted()
    assert go(S4.s, None, 1, Q, O, n, total, R, cap, F) == EINVAL and b"K must lie in [5, 63]" in L.cp_last_error()
    with pytest.raises(ClassProError):
        S4.read_fixes((seq, off))
    S4.close()
    T4.close()
    with pytest.raises(ClassProError):
        S.read_fixes((seq, off), count_range=(0, None))
    fo, f, _ = S.read_fixes((seq, off))
    with pytest.raises(ValueError):
        S.apply_fixes((seq, off), fo[:-1], f)
    with pytest.raises(ValueError):
        S.apply_fixes((seq, off), fo, f["records"][:3])
    with pytest.raises(ValueError):
        S.apply_fixes((seq, off), fo, f["first"])
    S.close()
    with pytest.raises(ValueError):
        S.read_fixes((seq, off))
    with pytest.raises(ValueError):
        S.apply_fixes((seq, off), fo, f)


# ---- 8. records that cannot be ----

def test_spoilt_records_change_nothing(torch_dev):
    """By the clamping contract any content of the records is a legal input: what is no edit is treated as none."""
    torch = torch_dev
    K, D = 21, 4
    ents, seqs = case(K)
    S = load(torch, ents, K)
    seq, off = flat(torch, seqs)
    fo, f, tally = S.read_fixes((seq, off), max_indel=D)
    good = f["records"].clone()
    one = f["status"] == FO.ONE
    assert int(one.sum()) > 100
    total = int(off[-1])
    guard = 64

    def apply(rec):
        n = len(seqs)
        cap = total + 4 * rec.shape[0]
        out = torch.full((cap + guard,), 35, dtype=torch.uint8, device="cuda:0")
        ooff = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        count = C.c_int64()
        rc = S.L.cp_apply_fixes(seq.data_ptr(), off.data_ptr(), n, total, K, rec.data_ptr(), fo.data_ptr(), out.data_ptr(), cap,
                                ooff.data_ptr(), C.byref(count), None)
        torch.cuda.synchronize()
        assert rc == 0 and bool((out[count.value:] == 35).all())   # nothing behind the new total: not the spare room, not the guard
        return split(torch, out[:count.value], ooff)

    want = FO.apply(seqs, *FO.read_fixes(ents, seqs, K, D)[:2], K)
    assert apply(good) == want != seqs
    for which, value in ((20, 9), (20, FO.CLASH), (20, FO.MANY), (21, 200), (21, 5), (22, 200), (22, 5)):   # status, del, nins
        rec = good.clone()
        rec.view(torch.uint8)[:, which][one] = value
        assert apply(rec) == seqs, (which, value)
    for first in (1 << 40, -3, (1 << 63) - 1, -(1 << 63)):                         # first beyond the read
        rec = good.clone()
        rec[:, 0][one] = first
        assert apply(rec) == seqs, first
    rec = good.clone()
    rec.view(torch.int32)[:, 4][one] += 1                                          # the record names another read
    assert apply(rec) == seqs
    rec = good.clone()
    ends = (off[1:] - off[:-1])[f["read"].long()] - (K - 1) - 1                    # e on the read's last base, del one too many
    rec[:, 0][one] = ends[one]
    rec.view(torch.uint8)[:, 21][one] = 2
    assert apply(rec) == seqs
    S.close()

"""cp_kmer_sorted_read_runs (SortedKmers.read_runs) on a real MI355X (`-m gpu`), against the plain loops of
tests/runs_oracle.py: the reads of tests/test_gpu_readhits.py whose markers are written out, reads packed into the chunks
of single lanes, runs that cross whole blocks of skipped positions, random read sets for every kind of lookup, the
identities with `read_hits` and `profiles`, capacity and overflow, batching, that the tables are only read, and the
argument errors.  Everything is integers: the tolerance is zero."""
import ctypes as C
import random

import numpy as np
import pytest

import ktab_oracle as KO
import readhits_oracle as RO
import runs_oracle as UO
import tabprof_oracle as TO
from test_gpu_ktab import flat, mixed_reads, table_of
from test_gpu_readhits import BLOCK, RANGES, block_case, hand_case, lane_case, prefix_of, random_case, rnd, tables_for
from test_gpu_tabprof import load

pytestmark = pytest.mark.gpu
EINVAL, EOVERFLOW = -1, -5
MASKS = ((UO.PHASE_SKIP, UO.PHASE_EMIT), (0, 1 << UO.NONE), (0, UO.ALL))      # phase, absence, everything


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def got(torch, A, B, batch, **kw):
    """(run_off, [(first, last, n, read, state)]) as lists."""
    off, r = A.read_runs(B, batch if not isinstance(batch, list) else flat(torch, batch), **kw)
    assert off.dtype == torch.int64 and r["first"].dtype == r["last"].dtype == r["n"].dtype == torch.int64
    assert r["read"].dtype == r["state"].dtype == torch.int32
    cols = [r[k].cpu().tolist() for k in ("first", "last", "n", "read", "state")]
    return off.cpu().tolist(), list(zip(*cols))


def check(torch, A, B, a, b, seqs, K, masks=MASKS, **kw):
    seen = []
    kw.setdefault("keys", TO.keys_of(seqs, K, kw.get("canonical", True)))
    for skip, emit in masks:
        want = UO.read_runs(a, b, seqs, K, skip, emit, **kw)
        assert got(torch, A, B, seqs, skip=skip, emit=emit, **{k: v for k, v in kw.items() if k != "keys"}) == want, (skip, emit, kw)
        seen.append(want)
    return seen


# ---- 1. reads whose markers are written out ----

def test_hand_made(torch_dev):
    torch = torch_dev
    K, seqs, marks, _ = hand_case()
    a, b = tables_for(seqs, K, marks)
    A, B, E = load(torch, a, K), load(torch, b, K), load(torch, [], K)
    masks = MASKS + ((0, 1 << UO.A),)
    seen = check(torch, A, B, a, b, seqs, K, masks)
    assert [r[:3] + r[4:] for r in seen[0][1][:3]] == [(0, 1, 2, UO.A), (3, 5, 2, UO.B), (6, 6, 1, UO.A)]
    assert seen[1][1][0] == (2, 2, 1, 0, UO.NONE)
    assert [r for r in seen[2][1] if r[3] == 4] == [(0, 0, 1, 4, UO.A), (1, 1, 1, 4, UO.NONE), (2, 6, 5, 4, UO.OTHER),
                                                   (7, 7, 1, 4, UO.NONE), (8, 8, 1, 4, UO.B)]
    assert seen[0][0] == [0, 3, 4, 4, 4, 6, 6, 6, 6, 12, 12]
    check(torch, B, A, b, a, seqs, K, masks)                                           # A and B swapped
    one = check(torch, A, None, a, None, seqs, K, masks)                               # no second table
    assert {r[4] for r in one[2][1]} == {UO.NONE, UO.A, UO.OTHER}
    check(torch, E, B, [], b, seqs, K, masks)                                          # an empty A
    check(torch, E, None, [], None, seqs, K, masks)
    both = check(torch, A, A, a, a, seqs, K, masks)                                    # a is b
    assert {r[4] for r in both[2][1]} == {UO.NONE, UO.BOTH, UO.OTHER} and both[0][1] == []
    check(torch, A, B, a, b, seqs + seqs, K, masks)                                    # the same reads twice in one batch
    off, r = A.read_runs(B, flat(torch, []))                                           # an empty batch
    assert off.cpu().tolist() == [0] and off.dtype == torch.int64
    assert all(r[k].numel() == 0 and r[k].dtype == torch.int64 for k in ("first", "last", "n"))
    assert all(r[k].numel() == 0 and r[k].dtype == torch.int32 for k in ("read", "state"))
    assert got(torch, A, B, [b"", b"ACG", b""]) == ([0, 0, 0, 0], [])
    for s in (A, B, E):
        s.close()


# ---- 2. many reads inside one lane's chunk ----

@pytest.mark.parametrize("K", [5, 21])
def test_reads_of_exactly_k_bases_in_a_row(torch_dev, K):
    torch = torch_dev
    reads, a, b = lane_case(K)
    A, B = load(torch, a, K), load(torch, b, K)
    seen = check(torch, A, B, a, b, reads, K)
    assert seen[0][1] == [(0, 0, 1, i, (UO.A, UO.B)[i % 2]) for i in range(len(reads))]
    one = b"".join(reads)
    seen = check(torch, A, B, a, b, [one], K)
    if K == 21:                                                                        # 100 runs of one marker: 99 switches
        assert [(r[2], r[4]) for r in seen[0][1]] == [(1, (UO.A, UO.B)[i % 2]) for i in range(100)]
        assert [r[0] for r in seen[0][1]] == [K * i for i in range(100)]
    check(torch, A, B, a, b, reads[:70] + [one] + reads[70:] + [b"", one[:K - 1], one[3:]], K)
    A.close()
    B.close()


# ---- 3. runs over whole blocks ----

@pytest.mark.parametrize("nblocks,last", [(5, 4), (7, 6)])
def test_block_edges(torch_dev, nblocks, last):
    """The read of block_case: marker groups round its bases BLOCK and last * BLOCK, nothing between.  In phase mode with
    `same` the run that spans the gap begins in one block and ends three or five blocks later, across whole blocks of
    skipped positions, and its n is the sum over both sides; otherwise it is two runs.  In absence mode the NONE run
    between the groups covers whole blocks.  The read's last run is closed by the read's end."""
    torch = torch_dev
    rng = random.Random(nblocks)
    for same in (False, True):
        K, read, a, b, _ = block_case(nblocks, last, same)
        A, B = load(torch, a, K), load(torch, b, K)
        m = UO.marks_of(a, b, [read], K)[0]
        phase, absent = UO.runs(m, UO.PHASE_SKIP, UO.PHASE_EMIT), UO.runs(m, 0, 1 << UO.NONE)
        n = 2 * (K + 70) + 1
        span = [r for r in phase if r[2] - r[1] > BLOCK]
        assert len(phase) == (2 * n - 1 if same else 2 * n) and (len(span), sum(r[3] for r in span)) == ((1, 2) if same else (0, 0))
        gap = absent[1]
        assert len(absent) == 3 and gap[3] == gap[2] - gap[1] + 1 == (last - 1) * BLOCK - n and absent[2][2] == len(m) - 1
        for total in (0, 37, 16379):
            pre = prefix_of(rng, total, K)
            seqs = pre + [read, rnd(rng, 30)]
            seen = check(torch, A, B, a, b, seqs, K)
            mine = [r for r in seen[0][1] if r[3] == len(pre)]
            assert [(r[4], r[0], r[1], r[2]) for r in mine] == phase
            assert [(r[4], r[0], r[1], r[2]) for r in seen[1][1] if r[3] == len(pre)] == absent
        A.close()
        B.close()


# ---- 4. random reads, every kind of lookup ----

@pytest.mark.parametrize("K", [5, 12, 21, 31, 32, 40, 44, 63])
def test_random_reads(torch_dev, K):
    torch = torch_dev
    a, b, seqs = random_case(K)
    A, B = load(torch, a, K, piece=999), load(torch, b, K)
    batch = flat(torch, seqs)
    seen, states = set(), set()
    for canonical in (True, False):
        keys = TO.keys_of(seqs, K, canonical)
        for ar in RANGES:
            for br in RANGES:
                for skip, emit in MASKS:
                    want = UO.read_runs(a, b, seqs, K, skip, emit, canonical, ar, br, keys)
                    assert got(torch, A, B, batch, skip=skip, emit=emit, canonical=canonical, a_range=ar, b_range=br) == want, \
                        (canonical, ar, br, skip, emit)
                    seen.add((skip, tuple(want[1])))
                    states |= {r[4] for r in want[1]}
    assert {UO.NONE, UO.A, UO.B, UO.OTHER} <= states and (K != 5 or UO.BOTH in states)
    assert len(seen) > 16                                  # the ranges, the strand and the masks change the runs
    A.close()
    B.close()


# ---- 5. against code that exists ----

@pytest.mark.parametrize("K", [21, 40])
def test_against_read_hits_and_profiles(torch_dev, K):
    """Snapshots sorted here (exact counts), not loaded ones."""
    torch = torch_dev
    ra, rb = mixed_reads(K, 5), mixed_reads(K, 7)
    _, _, seqs = random_case(K)
    TA, TB = table_of(torch, ra + seqs[3:5], K), table_of(torch, rb + seqs[3:4], K)
    A, B = TA.sorted(), TB.sorted()
    seq, off = flat(torch, seqs)
    n, switches = len(seqs), 0
    for ar, br in ((None, None), (None, (2, None)), ((2, 3), (None, 1))):
        hits = A.read_hits(B, (seq, off), a_range=ar, b_range=br).cpu().tolist()
        roff, r = got(torch, A, B, (seq, off), skip=UO.PHASE_SKIP, emit=UO.PHASE_EMIT, a_range=ar, b_range=br)
        assert [max(roff[i + 1] - roff[i] - 1, 0) for i in range(n)] == [h[4] for h in hits]
        switches += sum(h[4] for h in hits)
        _, r = got(torch, A, B, (seq, off), a_range=ar, b_range=br)
        for col, state in ((0, UO.A), (1, UO.B), (2, UO.BOTH), (3, UO.OTHER)):
            assert [sum(x[2] for x in r if x[3] == i and x[4] == state) for i in range(n)] == [h[col] for h in hits], (ar, br, col)
    assert switches > 0
    tally = torch.zeros(3, dtype=torch.int64, device="cuda:0")
    A.profiles((seq, off), tally=tally)
    _, r = got(torch, A, None, (seq, off), emit=1 << UO.NONE)
    assert sum(x[2] for x in r) == int(tally[1]) > 0
    for s in (A, B, TA, TB):
        s.close()


# ---- 6. capacity ----

def raw_call(torch, L, A, B, seq, off, n, total, skip, emit, cap, poison=-7):
    buf = torch.full((max(cap, 0) + 3, 4), poison, dtype=torch.int64, device="cuda:0")
    roff = torch.full((n + 1,), poison, dtype=torch.int64, device="cuda:0")
    count = C.c_int64(-1)
    rc = L.cp_kmer_sorted_read_runs(A.s, B.s if B is not None else None, 1, None, skip, emit, seq.data_ptr(), off.data_ptr(), n, total,
                                    buf.data_ptr() if cap > 0 else None, cap, roff.data_ptr(), C.byref(count), None)
    torch.cuda.synchronize()
    return rc, count.value, roff.cpu().tolist(), buf.cpu().tolist()


def test_capacity(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import lib
    L = lib()
    K = 21
    reads, a, b = lane_case(K)
    seqs = reads[:40] + [b"".join(reads), b"", reads[3][1:]] + reads[40:]               # about three hundred runs
    A, B = load(torch, a, K), load(torch, b, K)
    seq, off = flat(torch, seqs)
    n, total = len(seqs), int(off[-1])
    want_off, want = UO.read_runs(a, b, seqs, K)
    rows = [[f, l, m, (st << 32) | r] for f, l, m, r, st in want]
    t = len(want)
    assert t > 100
    rc, count, roff, _ = raw_call(torch, L, A, B, seq, off, n, total, 0, UO.ALL, 0)   # the counting call
    assert (rc, count, roff) == (EOVERFLOW, t, want_off)
    rc, count, roff, buf = raw_call(torch, L, A, B, seq, off, n, total, 0, UO.ALL, t)  # the exact call
    assert (rc, count, roff) == (0, t, want_off) and buf[:t] == rows and buf[t:] == [[-7] * 4] * 3
    for cap in (t - 1, t // 2):
        rc, count, roff, buf = raw_call(torch, L, A, B, seq, off, n, total, 0, UO.ALL, cap)
        assert (rc, count, roff) == (EOVERFLOW, t, want_off)
        assert buf[:cap] == rows[:cap] and buf[cap:] == [[-7] * 4] * 3                 # nothing beyond the capacity is touched
    A.close()
    B.close()


# ---- 7. batching ----

def test_batching(torch_dev):
    torch = torch_dev
    from classpro_amd.api import Batch
    K = 21
    a, b, seqs = random_case(K)
    long_k, long_read, la, lb, _ = block_case(5, 4, True)
    a, b = sorted({**dict(la), **dict(a)}.items()), sorted({**dict(lb), **dict(b)}.items())
    seqs = seqs[:6] + [long_read] + seqs[6:]
    A, B = load(torch, a, K), load(torch, b, K)
    for skip, emit in MASKS:
        off, whole = got(torch, A, B, seqs, skip=skip, emit=emit)
        assert (off, whole) == UO.read_runs(a, b, seqs, K, skip, emit)
        per = [[x[:3] + x[4:] for x in whole[off[i]:off[i + 1]]] for i in range(len(seqs))]
        alone = [got(torch, A, B, [s], skip=skip, emit=emit) for s in seqs]            # each read alone
        assert [[x[:3] + x[4:] for x in r] for _, r in alone] == per and all(o == [0, len(r)] and all(x[3] == 0 for x in r) for o, r in alone)
        roff, rev = got(torch, A, B, seqs[::-1], skip=skip, emit=emit)                 # reversed order
        assert [[x[:3] + x[4:] for x in rev[roff[i]:roff[i + 1]]] for i in range(len(seqs))] == per[::-1]
        assert got(torch, A, B, Batch.from_seqs(seqs, K), skip=skip, emit=emit) == (off, whole)
    A.close()
    B.close()


# ---- 8. the tables are only read ----

def test_tables_are_only_read(torch_dev):
    torch = torch_dev
    K = 40
    a, b, seqs = random_case(K)
    TA = table_of(torch, mixed_reads(K, 5), K)
    for A, B in ((load(torch, a, K), load(torch, b, K)), (TA.sorted(), load(torch, b, K))):
        before = [[x.clone() for x in s.ktab()] for s in (A, B)]
        A.read_runs(B, flat(torch, seqs))
        A.read_runs(B, flat(torch, seqs), skip=UO.PHASE_SKIP, canonical=False, a_range=(2, None), b_range=(None, 2))
        B.read_runs(None, flat(torch, seqs[::-1]), emit=1)
        A.read_runs(A, flat(torch, seqs))
        torch.cuda.synchronize()
        after = [s.ktab() for s in (A, B)]
        assert all(torch.equal(x, y) for s0, s1 in zip(before, after) for x, y in zip(s0, s1))
        A.close()
        B.close()
    TA.close()


# ---- 9. arguments ----

def test_arguments(torch_dev):
    torch = torch_dev
    from classpro_amd._lib import ClassProError, lib
    L = lib()
    K = 21
    a, b, seqs = random_case(K)
    A, B, B12 = load(torch, a, K), load(torch, b, K), load(torch, KO.table(mixed_reads(12), 12), 12)
    seq, off = flat(torch, seqs)
    n, total = len(seqs), int(off[-1])
    cap = 1 << 16
    buf = torch.full((cap, 4), -7, dtype=torch.int64, device="cuda:0")
    roff = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda:0")
    count = C.c_int64(-7)
    S, O, R, F = seq.data_ptr(), off.data_ptr(), buf.data_ptr(), roff.data_ptr()
    go = lambda x, y, rng, skip, emit, s, o, nr, tb, r, c, f, t=C.byref(count): \
        L.cp_kmer_sorted_read_runs(x, y, 1, rng, skip, emit, s, o, nr, tb, r, c, f, t, None)
    r4 = lambda *v: (C.c_int64 * 4)(*v)
    h, index = C.c_void_p(), KO.index(a, K)                # a snapshot that is still being loaded
    assert L.cp_kmer_sorted_load_begin(K, index.ctypes.data, C.byref(h)) == 0
    bad = [(None, B.s, None, 0, 31, S, O, n, total, R, cap, F), (A.s, B12.s, None, 0, 31, S, O, n, total, R, cap, F),
           (h, B.s, None, 0, 31, S, O, n, total, R, cap, F), (A.s, h, None, 0, 31, S, O, n, total, R, cap, F),
           (h, None, None, 0, 31, S, O, n, total, R, cap, F),
           (A.s, B.s, None, 0, 0, S, O, n, total, R, cap, F), (A.s, B.s, None, 3, 6, S, O, n, total, R, cap, F),
           (A.s, B.s, None, 32, 1, S, O, n, total, R, cap, F), (A.s, B.s, None, 0, 63, S, O, n, total, R, cap, F),
           (A.s, B.s, None, 0, 31, S, O, -1, total, R, cap, F), (A.s, B.s, None, 0, 31, S, O, n, -1, R, cap, F),
           (A.s, B.s, None, 0, 31, S, O, n, total, R, -1, F), (A.s, B.s, None, 0, 31, None, O, n, total, R, cap, F),
           (A.s, B.s, None, 0, 31, S, None, n, total, R, cap, F), (A.s, B.s, None, 0, 31, S, O, n, total, None, cap, F),
           (A.s, B.s, None, 0, 31, S, O, n, total, R, cap, None), (A.s, B.s, None, 0, 31, S, O, n, total, R, cap, F, None)]
    bad += [(A.s, B.s, rng, 0, 31, S, O, n, total, R, cap, F)
            for rng in (r4(0, 5, 1, 5), r4(3, 2, 1, 5), r4(1, 5, 0, 5), r4(1, 5, 4, 3), r4(-1, -1, 1, 1))]
    for args in bad:
        assert go(*args) == EINVAL, args
    assert go(A.s, B12.s, None, 0, 31, S, O, n, total, R, cap, F) == EINVAL and b"21-mers and 12-mers" in L.cp_last_error()
    L.cp_kmer_sorted_destroy(h)
    torch.cuda.synchronize()
    assert bool((buf == -7).all()) and bool((roff == -7).all()) and count.value == -7   # no call above launched anything
    assert go(A.s, B.s, None, 0, 31, None, None, 0, 0, None, 0, None) == 0 and count.value == 0   # no reads: no work, no error
    assert go(A.s, B.s, r4(1, 1, 1, 1), 0, 31, S, O, n, total, R, cap, F) == 0
    want_off, want = UO.read_runs(a, b, seqs, K, a_range=(1, 1), b_range=(1, 1))
    assert roff.cpu().tolist() == want_off and count.value == len(want)
    assert buf[:len(want)].cpu().tolist() == [[f, l, m, (st << 32) | r] for f, l, m, r, st in want]
    with pytest.raises(ValueError):
        A.read_runs(B12, (seq, off))
    with pytest.raises(ValueError):
        A.read_runs("B", (seq, off))
    with pytest.raises(ClassProError):
        A.read_runs(B, (seq, off), a_range=(0, None))
    with pytest.raises(ClassProError):
        A.read_runs(B, (seq, off), skip=1, emit=1)
    B.close()
    with pytest.raises(ValueError):
        A.read_runs(B, (seq, off))
    A.close()
    B12.close()

"""Every call family once on a LATE side stream (tests/stream_harness.py), on a real MI355X (`-m gpu`).

The rest of the suite issues every call on the default stream, where work a call does outside its `stream` argument -- a
blocking copy, a fill or a launch on the null stream, a read-back that does not wait for the call's kernels -- still runs
in order and passes.  Here the inputs of a call arrive ten milliseconds late on a side stream that does not block on the
null stream, the state one call leaves is late for the next (`rearm()` before every call of a chain), and every result is
compared with the oracles the suite has, never with the same code on the default stream.  The control of the harness
holds in every block: a clone queued on the default stream right after arming still saw the poison, so an escape would have
been seen.  Everything is integers and bytes: the tolerance is zero.

The batch: twelve reads, about 38,000 bases, over two haplotypes of 4,000 bases that differ by SNPs -- both whole and
reverse complemented, pieces, one with an N, one with substitutions and an inserted base, one that switches haplotype, an
empty read and a read of K-1 bases -- so three blocks of 16,384 positions and tables of a few thousand k-mers; K = 21 (a key fits `lo`) and K = 40 (`hi`
is loaded).  A `Batch` carries the sizes on the host: a call made with (seq, seq_off) tensors would read seq_off[-1] back
first, wait for the stream, and find its inputs on time.  `apply_fixes` does read fix_off[-1] back, so its inputs are not
late; it runs after a delay all the same."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import cmphist_oracle as CH
import cns_oracle as CO
import cnstab_oracle as CT
import fix_oracle as FO
import hetpairs_oracle as HO
import kprof_oracle as KP
import ktab_oracle as KO
import path_oracle as PA
import phase_oracle as PH
import prune_oracle as PR
import readhits_oracle as RO
import runs_oracle as RU
import setop_oracle as SO
import stream_harness as SH
import tabprof_oracle as TO
import truth_oracle as TR
import unitig_graph_oracle as GO
import unitig_oracle as UO
from test_gpu_classgs import compare_stats, np_accuracy, np_labels
from test_gpu_kfilter import check_filtered
from test_gpu_kmer_table import check_table
from test_gpu_kprof import split
from test_gpu_ktab import check as check_sorted
from test_gpu_parity import oracle_stages
from test_gpu_readfixes import records as fix_records
from test_gpu_setop import check as check_snapshot
from test_gpu_tabprof import i64, u8

pytestmark = pytest.mark.gpu
KS = (21, 40)
GENOME = 4000
MAX_ARMINGS = 150


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    cal = SH.calibrate(torch, force=True)                  # once per module
    print("stream_harness: %s, %.0f cycles per ms, %d per arming of %.1f ms" % (cal["mode"], cal["cycles_per_ms"], cal["unit"],
                                                                               cal["unit_ms"]))
    return torch


class Case:
    """The reads of the file comment at one K, and the oracles' tables of them."""

    def __init__(self, K):
        rng = random.Random(1000 + K)
        self.K = K
        h1, h2, self.snps = PH.genome(rng, K, length=GENOME, gap=(60, 140), edge=300)
        self.haps = [h1, h2]
        rc = PH.revcomp_seq
        noisy = bytearray(h1)
        for p in range(350, GENOME - 350, 610):            # spaced further than K apart: each is a gap one edit closes
            noisy[p] = rng.choice([c for c in b"ACGT" if c != noisy[p]])
        noisy[2001:2001] = b"G" if noisy[2000] != ord("G") else b"C"
        self.reads = [h1, rc(h2), h2, rc(h1), h1[:2000] + b"N" + h1[2001:], b"", h2[:K - 1], bytes(noisy), h2[300:3700],
                      rc(h1[500:3900]), h2[150:2000] + h1[2000:], h1[1000:]]          # the last but one switches haplotype
        self.total = sum(len(r) for r in self.reads)
        assert len(self.reads) == 12 and 2 * 16384 < self.total < 3 * 16384
        self.text = [r.decode() for r in self.reads]
        self.kprof = KP.run(self.reads, K)
        self.kprof["per"] = KP.count(self.reads, K)[1]
        self.ents = KO.entries(self.kprof["counter"])      # every k-mer of the reads
        self.solid = [(x, c) for x, c in self.ents if c >= 2]
        self.a, self.b = KO.table([h1], K), KO.table([h2], K)
        assert 3000 < len(self.solid) < len(self.ents) < 10000 and self.a != self.b
        self.keys = TO.keys_of(self.reads, K)

    def batch(self, torch, **tensors):
        """A fresh `Batch` of the reads and the (dst, src) pairs of late(): seq and seq_off, then what `tensors` names
        (a Batch field and its values as a host array)."""
        from classpro_amd.api import Batch
        B = Batch.from_seqs(self.reads, self.K)
        for name, value in tensors.items():
            getattr(B, name)[:len(value)].copy_(torch.from_numpy(np.array(value)).to(B.device))
        torch.cuda.synchronize()
        names = ["seq", "seq_off"] + list(tensors)
        return B, [(getattr(B, n), getattr(B, n).clone()) for n in names]


@functools.lru_cache(maxsize=None)
def case(K):
    return Case(K)


def pair(torch, values, dtype=None):
    """(dst, src) of a host array: two device tensors, dst to be poisoned."""
    src = torch.as_tensor(np.array(values), dtype=dtype).to("cuda:0")
    return src.clone(), src


def loaded(torch, ents, K, piece=None):
    """SortedKmers.from_records of the oracle's entries, from the host."""
    from classpro_amd.api import SortedKmers
    return SortedKmers.from_records(K, KO.index(ents, K), u8(KO.records_fast(ents, K)), piece=piece)


def warm(T, K, positions, **kw):
    """The first add, mark or add_keys of a table sizes its failure bitmaps, and the first add of a LabelAccuracy its per-read
    counters; each waits for its stream to do so, and a call that has waited finds its inputs on time.  So the object first
    takes a batch of `positions` bases in reads of K-1 bases: no k-mer, nothing counted, the buffers sized."""
    from classpro_amd.api import Batch
    n = positions // (K - 1) + 1
    B = Batch.from_seqs([b"A" * (K - 1)] * n, K)
    B.labels.fill_(ord("N"))
    return B, getattr(T, kw.get("how", "add"))(B, *kw.get("args", ()))


def same_hist(got, want):
    assert got[:4] == want[:4] and np.array_equal(got[4], want[4])


# ---- the harness itself -----------------------------------------------------------------------------------------

def test_the_delay_is_measured_and_the_control_sees_the_default_stream(torch_dev):
    """The calibration gives the delay asked for, within a factor of two either way; a block whose body does nothing passes
    its control; work queued on the side stream sees the late values and work queued on the default stream the poison."""
    torch = torch_dev
    cal = SH.calibrate(torch)
    assert cal["mode"] in ("sleep", "sort") and cal["unit"] >= 1
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst, src = pair(torch, np.arange(1000, dtype=np.int64))
    with SH.late(torch, (dst, src)) as side:
        a.record(side)
        SH.rearm()
        b.record(side)
        on_side = dst.clone()                              # in the stream's order: after the copy
        with torch.cuda.stream(torch.cuda.default_stream()):
            early = dst.clone()                            # outside it: at once
    ms = a.elapsed_time(b)
    print("stream_harness: one arming took %.2f ms" % ms)
    assert SH.DELAY_MS / 2 <= ms <= SH.DELAY_MS * 2 or cal["mode"] == "sort"
    assert torch.equal(on_side, src) and (early == -1).all()
    seq, seq_src = pair(torch, np.frombuffer(b"ACGT" * 100, np.uint8))
    with SH.late(torch, (seq, seq_src)):
        with torch.cuda.stream(torch.cuda.default_stream()):
            early = seq.clone()
    assert (early == SH.POISON_BYTE).all() and torch.equal(seq, seq_src)


# ---- KmerCounts -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_kmer_counts(torch_dev, K):
    torch = torch_dev
    from classpro_amd.api import KmerCounts
    c = case(K)
    want = c.kprof
    B, pairs = c.batch(torch)
    T = KmerCounts(K)
    warm(T, K, c.total)
    with SH.late(torch, *pairs):
        T.add(B)
        SH.rearm()
        s = T.stats()
        SH.rearm()
        h = T.hist()
        SH.rearm()
        S = T.sorted(1)
    for k, v in want["stats"].items():
        assert s[k] == v, (k, s[k], v)
    same_hist(h, want["hist"])
    check_sorted(S, c.ents, K)
    S.close()
    with SH.late(torch, *pairs):
        got = T.profiles(B).cpu().numpy()                  # asynchronous: nothing has waited for the batch when it returns
    assert np.array_equal(got, np.concatenate(want["profiles"]))
    T.close()


@pytest.mark.parametrize("K", KS)
def test_filtered_counts_mark_then_add(torch_dev, K):
    torch = torch_dev
    from classpro_amd.api import KmerCounts
    c = case(K)
    B, pairs = c.batch(torch)
    T = KmerCounts(K, filter_bits=1 << 16)
    warm(T, K, c.total, how="mark")
    with SH.late(torch, *pairs):
        T.mark(B)
    with SH.late(torch, *pairs):
        T.add(B)                                           # the count pass of a filtered table reads nothing back
        SH.rearm()
        prof = T.profiles(B)
        SH.rearm()
        h = T.hist()
        SH.rearm()
        s = T.stats()
        SH.rearm()
        f = T.filter_stats()
        prof = split(prof, c.reads, K)
    check_filtered((prof, h, s), f, c.kprof)
    assert f["filter_bits"] == 1 << 16
    T.close()


@pytest.mark.parametrize("K", KS)
def test_add_keys(torch_dev, K):
    torch = torch_dev
    from classpro_amd.api import KmerCounts
    c = case(K)
    keys = [x for x, _ in c.ents] + [x for x, _ in c.ents[::3]]
    random.Random(K).shuffle(keys)
    lo, lo_src = pair(torch, np.array([x & KO.M63 for x in keys], np.int64))
    hi, hi_src = pair(torch, np.array([x >> 63 for x in keys], np.int64))
    assert (K == 40) == bool(hi_src.any())
    T = KmerCounts(K)
    warm(T, K, len(keys))
    with SH.late(torch, (lo, lo_src), (hi, hi_src)):
        T.add_keys(lo, hi if K == 40 else None)
        SH.rearm()
        S = T.sorted(1)
    check_sorted(S, [(x, 2 if i % 3 == 0 else 1) for i, (x, _) in enumerate(c.ents)], K)
    S.close()
    T.close()


@pytest.mark.parametrize("K", KS)
def test_rel_labels_of_a_late_batch(torch_dev, K):
    """The table holds the two haplotypes; the reads' own errors are absent from it (E), the SNP k-mers are there once (H)."""
    torch = torch_dev
    from classpro_amd.api import Batch, KmerCounts
    c = case(K)
    T = KmerCounts(K)
    T.add(Batch.from_seqs(c.haps, K))
    B, pairs = c.batch(torch)
    with SH.late(torch, *pairs):
        lab, prof, counts = T.rel_labels(B, profiles=True)
        lab, prof, counts = lab.cpu().numpy().tobytes(), prof.cpu().numpy(), counts.cpu().tolist()
    rel = TR.rel_profiles(c.haps, c.reads, K)
    labs = [TR.labels(r, len(s), K) for r, s in zip(rel, c.reads)]
    assert lab == b"".join(labs) and np.array_equal(prof, np.concatenate(rel)) and counts == TR.label_counts(labs)
    assert min(counts[:3]) > 0
    T.close()


# ---- KmerTable --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_kmer_table(torch_dev, K):
    torch = torch_dev
    from classpro_amd.api import KmerTable
    c = case(K)
    rng = random.Random(K)
    canonical = K == 40
    labs = [b"N" * min(len(s), K - 1) + bytes(rng.choice(b"EEHHHDDR") for _ in range(max(0, len(s) - K + 1))) for s in c.reads]
    recs = [(b"r%d" % i, s, l) for i, (s, l) in enumerate(zip(c.reads, labs))]
    t, skipped = CO.table(recs, K, canonical)
    B, pairs = c.batch(torch, labels=np.frombuffer(b"".join(labs), np.uint8))
    T = KmerTable(K, canonical=canonical)
    warm(T, K, c.total)
    snaps = {}
    with SH.late(torch, *pairs):
        T.add(B)
        SH.rearm()
        check_table(T, t, skipped)                         # entries(), then stats()
        SH.rearm()
        s = T.stats()
        SH.rearm()
        h = T.class_hist()
        for label in "EHDR":
            SH.rearm()
            snaps[label] = T.sorted(label)
    assert s["n_kmers"] == B.total_kmers - skipped and skipped > 0
    for got, want in zip(h, CT.class_hist(t)):
        assert np.array_equal(got, want)
    for label, S in snaps.items():
        ents = CT.select(t, label)
        assert len(ents) > 100
        check_sorted(S, ents, K)
        S.close()
    with SH.late(torch, *pairs):
        out = T.consensus(B).cpu().numpy().tobytes()       # asynchronous
    assert out == b"".join(r[2] for r in CO.consensus_records(recs, K, t, canonical))
    T.close()


# ---- SortedKmers ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_sorted_load_find_profiles_ktab_hist(torch_dev, K):
    torch = torch_dev
    from classpro_amd.api import SortedKmers
    c = case(K)
    ents = c.solid
    rec, rec_src = pair(torch, u8(KO.records_fast(ents, K)))
    with SH.late(torch, (rec, rec_src)):
        S = SortedKmers.from_records(K, KO.index(ents, K), rec, piece=999)      # four pieces and more
    check_snapshot(torch, S, ents, K)
    rng = random.Random(K)
    keys = [x for x, _ in rng.sample(c.ents, 2000)] + [rng.getrandbits(2 * K) for _ in range(500)]
    hi, hi_src = pair(torch, np.array([x >> 63 for x in keys], np.int64))
    lo, lo_src = pair(torch, np.array([x & KO.M63 for x in keys], np.int64))
    with SH.late(torch, (hi, hi_src), (lo, lo_src)):
        pos = S.find(hi, lo).cpu().tolist()                # asynchronous
    want = TO.find(ents, keys)
    assert pos == want and 0 < sum(p < 0 for p in want) < len(want)
    B, pairs = c.batch(torch)
    with SH.late(torch, *pairs):
        tally = torch.zeros(3, dtype=torch.int64, device="cuda:0")
        prof = S.profiles(B, tally=tally).cpu().numpy()    # asynchronous
        tally = tally.cpu().tolist()
    cells, wt = TO.cells(ents, c.reads, K, keys=c.keys)
    assert np.array_equal(prof, TO.flat(cells)) and tally == wt and min(wt) > 0
    with SH.late(torch, *pairs):
        SH.rearm()
        got_rec, got_idx = S.ktab()
        got_rec, got_idx = got_rec.cpu().numpy().tobytes(), got_idx.cpu().numpy()
        SH.rearm()
        h = S.hist()
    assert got_rec == KO.records_fast(ents, K) and np.array_equal(got_idx, KO.index(ents, K))
    same_hist(h, SO.hist(ents))
    S.close()


@pytest.mark.parametrize("K", KS)
def test_sorted_algebra_and_pairs(torch_dev, K):
    torch = torch_dev
    c = case(K)
    _, pairs = c.batch(torch)
    out, rest = {}, {}
    with SH.late(torch, *pairs):
        A, B, S = loaded(torch, c.a, K, piece=1500), loaded(torch, c.b, K, piece=1500), loaded(torch, c.solid, K)
        for op in ("and", "or", "sub", "xor"):
            SH.rearm()
            out[op] = A.combine(B, op, "sum")
        SH.rearm()
        rest["compare"] = A.compare(B)
        SH.rearm()
        rest["cmp"] = A.compare_hist(S, 4, 12, "b")
        SH.rearm()
        rest["het"] = S.het_pairs(xmax=8, ymax=8, unique=True, table=True)
        SH.rearm()
        rest["sites"] = rest["het"][2].het_sites(mates=True)
    for op, r in out.items():
        want, tally = SO.combine(c.a, c.b, op, "sum")
        assert r.tally == tally and min(tally) > 0
        check_snapshot(torch, r, want, K)
        r.close()
    assert rest["compare"] == tally[:3]
    assert np.array_equal(rest["cmp"], CH.matrix(c.a, c.solid, 4, 12, "b"))
    mat, tally, P = rest["het"]
    members = HO.members(c.solid, K, None, True)
    assert np.array_equal(mat, HO.matrix(c.solid, K, 8, 8, None, True)) and tally == HO.tally(c.solid, K, None, True)
    assert len(members) >= 2 * len(c.snps) > 20
    check_snapshot(torch, P, members, K)
    mate, mark, ns = PH.sites(members, K)
    got_mark, got_ns, st, got_mate = rest["sites"]
    assert got_mark.tolist() == mark and got_mate.tolist() == mate and got_ns == ns
    assert st == {"mated": 2 * ns, "unmated": len(members) - 2 * ns}
    for x in (A, B, S, P):
        x.close()


@pytest.mark.parametrize("K", KS)
def test_read_hits_and_runs(torch_dev, K):
    torch = torch_dev
    c = case(K)
    A, Bt = loaded(torch, c.a, K), loaded(torch, c.b, K)
    B, pairs = c.batch(torch)
    with SH.late(torch, *pairs):
        hits = A.read_hits(Bt, B).cpu().tolist()           # asynchronous
    want = RO.rows(c.a, c.b, c.reads, K, keys=c.keys)
    assert hits == want and sum(r[4] for r in want) > 0 and all(sum(r[i] for r in want) > 0 for i in range(4))
    with SH.late(torch, *pairs):
        off, r = A.read_runs(Bt, B)
        off, runs = off.cpu().tolist(), list(zip(*[r[k].cpu().tolist() for k in ("first", "last", "n", "read", "state")]))
    assert (off, runs) == RU.read_runs(c.a, c.b, c.reads, K, keys=c.keys) and len(runs) > 100
    with SH.late(torch, *pairs):
        off, r = A.read_runs(None, B, skip=A.RUN_OTHER, emit=A.RUN_NONE)      # no second table
        off, runs = off.cpu().tolist(), list(zip(*[r[k].cpu().tolist() for k in ("first", "last", "n", "read", "state")]))
    assert (off, runs) == RU.read_runs(c.a, None, c.reads, K, 1 << RU.OTHER, 1 << RU.NONE, keys=c.keys)
    A.close()
    Bt.close()


@pytest.mark.parametrize("K", KS)
def test_read_fixes_then_apply(torch_dev, K):
    torch = torch_dev
    c = case(K)
    S = loaded(torch, c.solid, K)
    B, pairs = c.batch(torch)
    with SH.late(torch, *pairs):
        off, f, tally = S.read_fixes(B, max_indel=1)
        SH.rearm()
        out, out_off = S.apply_fixes(B, off, f)
        out, out_off = out.cpu().numpy().tobytes(), out_off.cpu().tolist()
    woff, wrecs, wtally = FO.read_fixes(c.solid, c.reads, K, 1)
    assert off.cpu().tolist() == woff and fix_records(f) == wrecs and [tally[k] for k in S.FIX_TALLY] == wtally
    assert wtally[FO.ONE] >= 6
    assert [out[out_off[i]:out_off[i + 1]] for i in range(len(c.reads))] == FO.apply(c.reads, woff, wrecs, K)
    S.close()


@pytest.mark.parametrize("K", KS)
def test_unitigs_paths_counts_and_prune(torch_dev, K):
    torch = torch_dev
    from classpro_amd._lib import lib
    from classpro_amd.api import _stream_of
    c = case(K)
    ents = c.ents
    S = loaded(torch, ents, K)
    P = PA.Paths(ents, K)
    B, pairs = c.batch(torch)
    with SH.late(torch, *pairs):
        SH.rearm()
        U = S.unitigs(where=True, links=True, components=True)
    assert U.strings() == [u[1] for u in P.utgs] and (U.utg.tolist(), U.at.tolist()) == (P.utg, P.at)
    assert U.kc.tolist() == [u[3] for u in P.utgs] and U.links() == P.L.arcs and U.comp.tolist() == P.L.comp
    assert {k: U.link_tally[k] for k in GO.TALLY} == P.L.tally() and len(P.utgs) > 50 and len(P.L.arcs) > 50
    want = P.batch(c.text)
    limits = (3 * K, 3 * K, 3 * K)
    with SH.late(torch, *pairs):
        off, segs, t = S.read_paths(U, B, coverage=True, support=True)
        nz = []
        for v in (t["coverage"], t["support"]):
            SH.rearm()
            n = C.c_int64(-1)
            assert lib().cp_count_nonzero(v.data_ptr(), v.numel(), C.byref(n), _stream_of(torch.device("cuda:0"))) == 0
            nz.append(n.value)
        SH.rearm()
        kept, why, pt = S.prune(U, *limits, table=True)
    assert off.tolist() == want[0] and list(zip(*[segs[k].tolist() for k in PA.FIELDS])) == want[1]
    assert {k: t[k] for k in PA.TALLY} == want[2] and want[2]["joined"] > 50 and want[2]["other"] > 0
    assert t["coverage"].tolist() == want[3] and t["support"].tolist() == want[4]
    assert nz == [sum(x != 0 for x in want[3]), sum(x != 0 for x in want[4])] and 0 < nz[1] and 0 < nz[0] <= len(U)
    wkept, wwhy, wt = PR.prune(ents, K, None, limits, L=P.L)
    assert why.tolist() == wwhy and pt == wt and wt["removed_keys"] > 0
    check_snapshot(torch, kept, wkept, K)
    for x in (kept, U, S):
        x.close()


@pytest.mark.parametrize("K", KS)
def test_read_links_forest_and_split(torch_dev, K):
    """The chain of `SortedKmers.phase`, call by call, so that each is the first to wait after a delay."""
    torch = torch_dev
    from classpro_amd.api import KmerCounts, phase_forest
    c = case(K)
    want = PH.phase(c.ents, K, [c.reads], (2, None), 2)
    assert want["nsites"] > 20 and want["forest"]["blocks"] >= 1 and want["links"]["links"] > 100
    S = loaded(torch, c.ents, K)
    P = S.het_pairs(xmax=1, ymax=1, unique=True, count_range=(2, None), table=True)[2]
    check_snapshot(torch, P, want["P"], K)
    mark, mark_src = pair(torch, np.array(want["mark"], np.int32))
    B, pairs = c.batch(torch)
    with SH.late(torch, *pairs, (mark, mark_src)):
        links, tally = P.read_links(B, mark)
    wlinks, wt = PH.read_links(want["P"], want["mark"], c.reads, K)
    assert links.tolist() == wlinks and tally.tolist() == wt
    keys, keys_src = pair(torch, np.array(wlinks, np.int64))
    acc = KmerCounts(32)
    warm(acc, 32, len(wlinks))
    with SH.late(torch, (keys, keys_src)):
        acc.add_keys(keys)
        SH.rearm()
        edges = acc.sorted(1)
        SH.rearm()
        block, side, forest = phase_forest(edges, want["nsites"], 2)
    assert block.tolist() == want["block"] and side.tolist() == want["side"] and forest == want["forest"]
    blk, blk_src = pair(torch, np.array(want["block"], np.int64))
    sd, sd_src = pair(torch, np.array(want["side"], np.uint8))
    with SH.late(torch, (mark, mark_src), (blk, blk_src), (sd, sd_src)):
        A, Bs = P.phase_split(mark, blk, sd)
    check_snapshot(torch, A, want["A"], K)
    check_snapshot(torch, Bs, want["B"], K)
    assert want["A"] and want["B"]
    for x in (A, Bs, edges, acc, P, S):
        x.close()


# ---- threshold labels and their accuracy ------------------------------------------------------------------------

def random_truth(est, K):
    """Per read: the K-1 'N' of the estimate, then random labels."""
    rng = random.Random(K)
    return [np.concatenate([e[:K - 1], np.frombuffer(bytes(rng.choice(b"EHDR") for _ in range(max(len(e) - K + 1, 0))), np.uint8)])
            .astype(np.uint8) for e in est]


@pytest.mark.parametrize("K", KS)
def test_threshold_labels_and_accuracy(torch_dev, K):
    torch = torch_dev
    from classpro_amd.api import LabelAccuracy, threshold_labels
    c = case(K)
    profs = c.kprof["profiles"]
    rlens = [len(s) for s in c.reads]
    thres = (2, 5, 8)
    B, pairs = c.batch(torch, prof=np.concatenate(profs).view(np.int16))
    pairs += [(B.prof_off, B.prof_off.clone())]
    with SH.late(torch, *pairs):
        lab, cnt = threshold_labels(B, thres, K)           # asynchronous
        lab, cnt = lab[:B.total_bases].cpu().numpy(), cnt.cpu().tolist()
    est = np_labels(profs, rlens, thres, K)
    wl = np.concatenate(est)
    assert np.array_equal(lab, wl) and cnt == [int((wl == ord(ch)).sum()) for ch in "EHDR"] and min(cnt[:3]) > 0
    truth = random_truth(est, K)
    B, pairs = c.batch(torch, labels=wl)
    tr, tr_src = pair(torch, np.concatenate(truth + [np.zeros(8, np.uint8)]))
    A = LabelAccuracy(K)
    W = warm(A, K, 11 * (K - 1), args=(tr_src,))[0]            # twelve reads: the per-read counters
    with SH.late(torch, *pairs, (tr, tr_src)):
        A.add(B, tr)                                       # asynchronous
        SH.rearm()
        s = A.stats()
    want = np_accuracy(est, truth, K)
    want["n_reads"] += W.nreads
    compare_stats(s, want)
    assert s["ntot"] == B.total_kmers
    A.close()


# ---- the classifier ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reads_with_profiles():
    from classpro_amd import synth
    from oracle.oracle import Oracle
    ds = synth.make_dataset(genome_len=30000, cov=30, read_len=5000, seed=21)
    O = Oracle(40, 20000, 15, 30)
    packed = synth.pack_batch(ds["seqs"], ds["profiles"])
    return ds, O, packed, O.classify_batch(*packed, nthreads=4), oracle_stages(O, ds)


def test_classifier(torch_dev, reads_with_profiles):
    torch = torch_dev
    from classpro_amd.api import (Batch, Classifier, STAGE_CLASS_ALL, encode_profiles, expand_label_runs, math_eval, pack_bases)
    ds, O, (seq, so, prof, po), want, stages = reads_with_profiles
    K = 40
    clf = Classifier(K=K, read_len=20000, hcov=15, dcov=30)
    B = Batch(seq, so, prof, po)
    pairs = [(getattr(B, n), getattr(B, n).clone()) for n in ("seq", "seq_off", "prof", "prof_off")]
    with SH.late(torch, *pairs):
        got = clf.classify(B)
    assert np.array_equal(got, want)
    with SH.late(torch, *pairs):
        clf.run(B, STAGE_CLASS_ALL)
        SH.rearm()
        nc, ni, nr, off = clf.counts(B)
        SH.rearm()
        ivs = clf.intervals(B)
        SH.rearm()
        asgn = clf.rel_asgn(B)
        SH.rearm()
        bits = np.unpackbits(clf.bitmap(B).view(np.uint8), bitorder="little")[:B.total_kmers]
    for r, ((iv, _), (fw, bw), w) in enumerate(zip(ivs, asgn, stages)):
        assert ni[r] == len(iv) and np.array_equal(iv["asgn"], w["call"]["asgn"])
        assert np.array_equal(fw, w["crel"][2]) and np.array_equal(bw, w["crel"][3])
    p = prof.astype(np.int64)                              # the candidate scan, as tests/test_gpu_parity.py states it
    exp = np.zeros(B.total_kmers, np.uint8)
    exp[1:] = (np.minimum(p[1:], p[:-1]) < O.scalars()[0][1]) & (np.abs(p[1:] - p[:-1]) >= 3)
    inner = np.ones(B.total_kmers, bool)
    inner[po[:-1]] = False
    assert np.array_equal(bits[inner], exp[inner])
    with SH.late(torch, *pairs):
        runs = clf.label_runs(B)
        SH.rearm()
        clf.classify(B)                                    # the seeds are found on a labelled batch
        SH.rearm()
        seeds, reps = clf.find_seeds(B)
    for r, (ends, cls) in enumerate(runs):
        assert expand_label_runs(ends, cls, int(so[r + 1] - so[r]), K) == want[so[r]:so[r + 1]].tobytes()
    for r, (s, q) in enumerate(zip(ds["seqs"], ds["profiles"])):
        sas, rep = O.find_seeds(s, want[so[r]:so[r + 1]].tobytes(), q)
        assert np.array_equal(seeds[so[r] + K - 1:so[r + 1]], sas) and np.array_equal(reps[r].reshape(-1, 2), rep.reshape(-1, 2))
    codes, co = encode_profiles(ds["profiles"])
    packed, pk_off = pack_bases([bytes(s) for s in ds["seqs"]])
    with SH.late(torch, *pairs):
        B.prof = clf.decode_profiles(codes, co, po)        # the inputs go up on the side stream, behind the delay
        SH.rearm()
        B.seq = clf.unpack_bases(packed, pk_off, so)
        SH.rearm()
        got = clf.classify(B)
        SH.rearm()
        x = np.abs(np.random.default_rng(1).standard_normal(100000)) * 1e3
        root = math_eval(2, x)
    assert np.array_equal(got, want) and np.array_equal(root, np.sqrt(x))
    clf.close()


# ---- the calls without a stream argument, from another stream ---------------------------------------------------

@pytest.mark.parametrize("K", KS)
def test_calls_without_a_stream_wait_for_the_objects_stream(torch_dev, K):
    """The work is queued on stream A, behind the delay; the call without a stream argument is made while stream B is
    current.  The header's contract: such a call waits for the stream of the last call that queued work on the object."""
    torch = torch_dev
    from classpro_amd.api import KmerCounts, KmerTable, LabelAccuracy
    c = case(K)
    other = torch.cuda.Stream()
    B, pairs = c.batch(torch)
    T = KmerCounts(K, filter_bits=1 << 16)
    T.mark(B)
    with SH.late(torch, *pairs):
        T.add(B)                                           # A: the count pass, no read-back
        with torch.cuda.stream(other):
            s, h, f = T.stats(), T.hist(), T.filter_stats()         # B
    prof = split(T.profiles(B), c.reads, K)
    check_filtered((prof, h, s), f, c.kprof)
    T.close()
    T = KmerCounts(K)
    with SH.late(torch, *pairs):
        T.add(B)
        with torch.cuda.stream(other):
            s, h = T.stats(), T.hist()
            S = T.sorted(1)                                # cp_kmer_counts_sort waits for the table's stream, then runs on B
    assert all(s[k] == v for k, v in c.kprof["stats"].items())
    same_hist(h, c.kprof["hist"])
    check_sorted(S, c.ents, K)
    S.close()
    T.close()
    rng = random.Random(K)
    labs = [b"N" * min(len(r), K - 1) + bytes(rng.choice(b"EHDR") for _ in range(max(0, len(r) - K + 1))) for r in c.reads]
    recs = [(b"r%d" % i, r, l) for i, (r, l) in enumerate(zip(c.reads, labs))]
    B, pairs = c.batch(torch, labels=np.frombuffer(b"".join(labs), np.uint8))
    t, skipped = CO.table(recs, K, True)
    T = KmerTable(K, canonical=True)
    with SH.late(torch, *pairs):
        T.add(B)
        with torch.cuda.stream(other):
            check_table(T, t, skipped)
            h = T.class_hist()
    for got, want in zip(h, CT.class_hist(t)):
        assert np.array_equal(got, want)
    T.close()
    est = [np.frombuffer(l, np.uint8) for l in labs]
    truth = random_truth(est, K)
    tr, tr_src = pair(torch, np.concatenate(truth + [np.zeros(8, np.uint8)]))
    A = LabelAccuracy(K)
    with SH.late(torch, *pairs, (tr, tr_src)):
        A.add(B, tr)                                       # A, asynchronous
        with torch.cuda.stream(other):
            s = A.stats()                                  # B
    compare_stats(s, np_accuracy(est, truth, K))
    A.close()


def test_the_budget_of_armings(torch_dev):
    """Runs last: the whole file queued no more delays than the budget."""
    print("stream_harness: %d armings of %.1f ms in this process" % (SH.armings(), SH.DELAY_MS))
    assert 0 < SH.armings() <= MAX_ARMINGS

"""Host-side Python mirror of the reference's per-read interface, batched, over the C ABI.

Names follow the reference (ClassPro.c:229-271): calc_seq_context, find_wall, find_rel_intvl,
classify_rel, classify_unrel; `Classifier.classify` is the whole read loop body for a batch.
PyTorch is used only to own device memory and streams; every computation is a HIP kernel in
libclasspro_amd.so.  Nothing here imports oracle/.
"""
import ctypes as C
import numpy as np
import torch

from ._lib import CP_EOVERFLOW, lib, check

STAGE_SCAN, STAGE_WALL, STAGE_REL, STAGE_CLASS_REL, STAGE_CLASS_ALL, STAGE_LABELS = 1, 2, 3, 4, 5, 6

INTVL_DTYPE = np.dtype({
    "names":   ["b", "e", "cb", "ce", "ccb", "cce", "is_rel", "asgn", "pe", "peo_b", "peo_e"],
    "formats": ["<i4", "<i4", "<u2", "<u2", "<u2", "<u2", "u1", "i1", "<f8", "<f8", "<f8"],
    "offsets": [0, 4, 8, 10, 12, 14, 16, 17, 24, 32, 40],
    "itemsize": 48,
})


def hist_covs(hist, low, high, ilowcnt=0, ihighcnt=0, coverage=0):
    """process_global_hist (hist.c:28): (H,D) coverage from a FASTK histogram or from -c."""
    h = np.ascontiguousarray(hist, dtype=np.int64)
    hc, dc = C.c_int(), C.c_int()
    check(lib().cp_hist_covs(h.ctypes.data, low, high, ilowcnt, ihighcnt, coverage, C.byref(hc), C.byref(dc)))
    return hc.value, dc.value


def decode_profile(code, cap=60000):
    """Fetch_Profile's decoder (libfastk.c:1467) for one read's code string."""
    buf = np.frombuffer(bytes(code), dtype=np.uint8)
    out = np.zeros(cap, np.uint16)
    n = check(lib().cp_decode_profile(buf.ctypes.data if len(buf) else None, len(buf), out.ctypes.data, cap))
    return n, out[:min(n, cap)]


def load_error_model(path):
    """-M: pe[t][l] fitted from a HIsim error-model file (wall.c:55-115); double[3][21]."""
    pe = np.zeros((3, 21), np.float64)
    check(lib().cp_load_error_model(path.encode(), pe.ctypes.data))
    return pe


def encode_profiles(profiles):
    """FASTK code strings for a list of count arrays: (uint8 codes, int64 code_off[n+1])."""
    L = lib()
    chunks, off = [], [0]
    for p in profiles:
        p = np.ascontiguousarray(p, np.uint16)
        buf = np.empty(2 * len(p) + 2, np.uint8)
        n = check(L.cp_encode_profile(p.ctypes.data, len(p), buf.ctypes.data, len(buf)))
        chunks.append(buf[:n].copy())
        off.append(off[-1] + n)
    codes = np.concatenate(chunks) if chunks else np.zeros(0, np.uint8)
    return codes, np.array(off, np.int64)


def pack_bases(seqs):
    """2-bit packing of a list of reads (bytes) for cp_unpack_bases: (uint8 packed, int64 pack_off[n+1]) or None when a
    read holds a letter other than upper-case A, C, G, T (the batch then travels as characters)."""
    L = lib()
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([(len(x) + 3) // 4 for x in seqs], out=off[1:])
    out = np.zeros(max(int(off[-1]), 1), np.uint8)
    for i, x in enumerate(seqs):
        b = np.frombuffer(bytes(x), np.uint8)
        if len(b) and check(L.cp_pack_bases(b.ctypes.data, len(b), out[off[i]:].ctypes.data)) == 0:
            return None
    return out, off


def unpack_labels(packed, pack_off, rlens, K):
    """cp_unpack_labels for every read of a batch: the concatenated label bytes."""
    L = lib()
    packed = np.ascontiguousarray(packed, np.uint8)
    so = np.zeros(len(rlens) + 1, np.int64)
    np.cumsum(rlens, out=so[1:])
    out = np.zeros(max(int(so[-1]), 1), np.uint8)
    for i, n in enumerate(rlens):
        if n:
            check(L.cp_unpack_labels(packed[pack_off[i]:].ctypes.data, int(n), K, out[so[i]:].ctypes.data))
    return out[:so[-1]]


def math_eval(fn, x, x2=None, device="cuda:0"):
    """cp_math_eval: the device's own exp (fn 0) / log (1) / sqrt (2) / bessi (3, n = x2) / logp_skellam (4, k = x2) on an
    array of doubles; returns a host float64 array."""
    dev = torch.device(device)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev)
    x2d = torch.from_numpy(np.ascontiguousarray(x2, np.float64)).to(dev) if x2 is not None else None
    yd = torch.empty_like(xd)
    check(lib().cp_math_eval(fn, xd.data_ptr(), x2d.data_ptr() if x2d is not None else None, yd.data_ptr(), xd.numel(),
                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    torch.cuda.synchronize(dev)
    return yd.cpu().numpy()


def expand_label_runs(ends, cls, rlen, K):
    """cp_expand_label_runs: one read's label string from its runs."""
    ends = np.ascontiguousarray(ends, np.int32)
    cls = np.ascontiguousarray(cls, np.uint8)
    out = np.zeros(max(rlen, 1), np.uint8)
    check(lib().cp_expand_label_runs(ends.ctypes.data if len(ends) else None, cls.ctypes.data if len(cls) else None, len(ends), rlen, K,
                                     out.ctypes.data))
    return out[:rlen].tobytes()


class Batch:
    """A batch of reads resident in HBM in the flat layout of include/classpro_amd.h."""

    def __init__(self, seq, seq_off, prof, prof_off, device="cuda:0"):
        self.device = torch.device(device)
        self.nreads = len(seq_off) - 1
        self.total_bases = int(seq_off[-1])
        self.total_kmers = int(prof_off[-1])
        self.seq_off_h = np.ascontiguousarray(seq_off, np.int64)
        self.prof_off_h = np.ascontiguousarray(prof_off, np.int64)
        dev = self.device
        self.seq = torch.from_numpy(np.ascontiguousarray(seq, np.uint8)).to(dev)
        self.prof = torch.from_numpy(np.ascontiguousarray(prof, np.uint16).view(np.int16)).to(dev)
        self.seq_off = torch.from_numpy(self.seq_off_h).to(dev)
        self.prof_off = torch.from_numpy(self.prof_off_h).to(dev)
        self.labels = torch.zeros(max(self.total_bases, 1), dtype=torch.uint8, device=dev)

    @classmethod
    def from_device(cls, rd):
        """A batch over tensors that are already in HBM (a `DeviceSynth.reads()` result); nothing is copied."""
        b = cls.__new__(cls)
        b.device = rd["seq"].device
        b.nreads, b.total_bases, b.total_kmers = rd["nreads"], rd["total_bases"], rd["total_kmers"]
        b.seq_off_h, b.prof_off_h = rd["seq_off_h"], rd["prof_off_h"]
        b.seq, b.prof, b.seq_off, b.prof_off = rd["seq"], rd["prof"], rd["seq_off"], rd["prof_off"]
        b.labels = torch.zeros(max(b.total_bases, 1), dtype=torch.uint8, device=b.device)
        return b

    @classmethod
    def from_seqs(cls, seqs, K, device="cuda:0"):
        """A batch of reads alone: `prof` has room for every k-mer count (rlen-(K-1) per read, none for a read shorter
        than K) but is not filled; `KmerCounts.profiles(batch)` fills it on the device."""
        b = cls.__new__(cls)
        b.device = dev = torch.device(device)
        rl = np.array([len(s) for s in seqs], np.int64)
        b.seq_off_h = np.zeros(len(seqs) + 1, np.int64)
        b.prof_off_h = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum(rl, out=b.seq_off_h[1:])
        np.cumsum(np.maximum(rl - (K - 1), 0), out=b.prof_off_h[1:])
        b.nreads, b.total_bases, b.total_kmers = len(seqs), int(b.seq_off_h[-1]), int(b.prof_off_h[-1])
        flat = np.frombuffer(b"".join(bytes(s) for s in seqs), np.uint8)
        b.seq = torch.from_numpy(flat.copy() if len(flat) else np.zeros(1, np.uint8)).to(dev)
        b.prof = torch.empty(max(b.total_kmers, 8), dtype=torch.int16, device=dev)
        b.seq_off = torch.from_numpy(b.seq_off_h).to(dev)
        b.prof_off = torch.from_numpy(b.prof_off_h).to(dev)
        b.labels = torch.zeros(max(b.total_bases, 1), dtype=torch.uint8, device=dev)
        return b

    @classmethod
    def from_reads(cls, seqs, profiles, device="cuda:0"):
        from .synth import pack_batch
        return cls(*pack_batch(seqs, profiles), device=device)


class Classifier:
    """Global setup (ClassPro.c:536-554) + batched hot path."""

    def __init__(self, K=40, read_len=20000, hcov=20, dcov=40, device="cuda:0", model=None, pe=None):
        self.L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("classpro_amd runs on a HIP device only")
        torch.cuda.set_device(self.device)
        self.K, self.read_len = K, read_len
        p = C.c_void_p()
        if pe is not None:                                  # the error model as a table (cp_params_create_pe)
            pe = np.ascontiguousarray(pe, np.float64).reshape(3, 21)
            check(self.L.cp_params_create_pe(K, read_len, hcov, dcov, pe.ctypes.data, C.byref(p)))
        else:
            check(self.L.cp_params_create_model(K, read_len, hcov, dcov, model.encode() if model else None, C.byref(p)))
        self.p = p
        w = C.c_void_p()
        check(self.L.cp_workspace_create(C.byref(w)))
        self.ws = w

    def close(self):
        if getattr(self, "ws", None):
            self.L.cp_workspace_destroy(self.ws)
            self.ws = None
        if getattr(self, "p", None):
            self.L.cp_params_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables ----
    def export(self):
        cov = (C.c_int * 4)()
        dr, cmax, hc = C.c_double(), C.c_int(), C.c_double()
        cth = np.zeros((3, 21, 256, 2, 2), np.uint8)
        pe = np.zeros((3, 21), np.float64)
        lf = np.zeros(32768, np.float64)
        check(self.L.cp_params_export(self.p, cov, C.byref(dr), C.byref(cmax), C.byref(hc),
                                      cth.ctypes.data, pe.ctypes.data, lf.ctypes.data))
        return dict(cov=list(cov), dr_ratio=dr.value, cmax=cmax.value, hc_erate=hc.value,
                    cthres=cth, pe=pe, logfact=lf)

    def tables(self):
        """Device bytes of the look-up tables in use (0 = computed on the spot): dict(skel, uerr, petab)."""
        v = [C.c_size_t() for _ in range(3)]
        check(self.L.cp_params_tables(self.p, *[C.byref(x) for x in v]))
        return dict(skel=v[0].value, uerr=v[1].value, petab=v[2].value)

    # ---- pipeline ----
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def run(self, b, last_stage=STAGE_LABELS):
        check(self.L.cp_run_stages(self.p, self.ws, b.seq.data_ptr(), b.seq_off.data_ptr(),
                                   b.prof.data_ptr(), b.prof_off.data_ptr(), b.nreads, b.total_bases,
                                   b.total_kmers, b.labels.data_ptr(), last_stage, self._stream()))

    def classify(self, b, check_overflow=True):
        """ClassPro.c:229-271 for every read of the batch; returns the label bytes (host)."""
        check(self.L.cp_classify_batch(self.p, self.ws, b.seq.data_ptr(), b.seq_off.data_ptr(),
                                       b.prof.data_ptr(), b.prof_off.data_ptr(), b.nreads, b.total_bases,
                                       b.total_kmers, b.labels.data_ptr(), self._stream()))
        if check_overflow:
            check(self.L.cp_workspace_check(self.ws))
        return b.labels[:b.total_bases].cpu().numpy()

    def check(self):
        check(self.L.cp_workspace_check(self.ws))

    def label_runs(self, b, rerun=True):
        """The batch's labels as runs (cp_label_runs): classification without painting the label string, then per read
        (ends int32[n], cls uint8[n]); `expand_label_runs` rebuilds the strings on the host.  rerun=False: the runs of the
        batch last classified on this workspace (after classify() / run())."""
        if rerun:
            self.run(b, STAGE_CLASS_ALL)
        cap = int(self.L.cp_label_runs_capacity(self.ws))
        dev = self.device
        d_end = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        d_cls = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        d_nr = torch.empty(max(b.nreads, 1), dtype=torch.int32, device=dev)
        d_off = torch.empty(b.nreads + 1, dtype=torch.int64, device=dev)
        check(self.L.cp_label_runs(self.p, self.ws, d_end.data_ptr(), d_cls.data_ptr(), d_nr.data_ptr(), d_off.data_ptr(), self._stream()))
        check(self.L.cp_workspace_check(self.ws))
        ends, cls, nr, off = d_end.cpu().numpy(), d_cls.cpu().numpy(), d_nr.cpu().numpy(), d_off.cpu().numpy()
        return [(ends[off[r]:off[r] + nr[r]].copy(), cls[off[r]:off[r] + nr[r]].copy()) for r in range(b.nreads)]

    def find_seeds(self, b):
        """-s (seed.c:966-1032) on a batch already labelled by classify()/run(): returns (seed labels as host bytes
        in the layout of the labels, list per read of int32[n,2] repeat-mask intervals in read coordinates)."""
        seeds = torch.zeros(max(b.total_bases, 1), dtype=torch.uint8, device=self.device)
        check(self.L.cp_find_seeds_batch(self.p, self.ws, b.seq.data_ptr(), b.seq_off.data_ptr(), b.prof.data_ptr(),
                                         b.prof_off.data_ptr(), b.labels.data_ptr(), b.nreads, b.total_bases, b.total_kmers,
                                         seeds.data_ptr(), self._stream()))
        check(self.L.cp_workspace_check(self.ws))
        cap = int(self.L.cp_rep_masks_capacity(self.ws))
        cnt = np.zeros(max(b.nreads, 1), np.int32)
        off = np.zeros(b.nreads + 1, np.int64)
        pairs = np.zeros((max(cap, 1), 2), np.int32)
        check(self.L.cp_get_rep_masks(self.ws, cnt.ctypes.data, off.ctypes.data, pairs.ctypes.data, max(cap, 1)))
        b.seeds = seeds
        return seeds[:b.total_bases].cpu().numpy(), [pairs[off[r]:off[r] + cnt[r]].copy() for r in range(b.nreads)]

    def decode_profiles(self, codes, code_off, prof_off):
        """Fetch_Profile on the device: returns a device tensor of counts (int16 view of uint16)."""
        dev = self.device
        c = torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).to(dev)
        co = torch.from_numpy(np.ascontiguousarray(code_off, np.int64)).to(dev)
        po = torch.from_numpy(np.ascontiguousarray(prof_off, np.int64)).to(dev)
        out = torch.zeros(max(int(prof_off[-1]), 8), dtype=torch.int16, device=dev)
        check(self.L.cp_decode_profiles(self.ws, c.data_ptr(), co.data_ptr(), po.data_ptr(), len(code_off) - 1,
                                        out.data_ptr(), self._stream()))
        check(self.L.cp_workspace_check(self.ws))
        return out

    def unpack_bases(self, packed, pack_off, seq_off):
        """Dazzler 2-bit bases -> upper-case characters on the device (uint8 tensor)."""
        dev = self.device
        pk = torch.from_numpy(np.ascontiguousarray(packed, np.uint8)).to(dev)
        po = torch.from_numpy(np.ascontiguousarray(pack_off, np.int64)).to(dev)
        so = torch.from_numpy(np.ascontiguousarray(seq_off, np.int64)).to(dev)
        out = torch.zeros(max(int(seq_off[-1]), 8), dtype=torch.uint8, device=dev)
        check(self.L.cp_unpack_bases(pk.data_ptr(), po.data_ptr(), so.data_ptr(), len(seq_off) - 1, out.data_ptr(), self._stream()))
        torch.cuda.synchronize(dev)
        return out

    def workspace_bytes(self):
        return int(self.L.cp_workspace_bytes(self.ws))

    # ---- stage read-back (parity tests) ----
    def counts(self, b):
        n = b.nreads
        nc, ni, nr = (np.zeros(n, np.int32) for _ in range(3))
        off = np.zeros(n + 1, np.int64)
        check(self.L.cp_get_counts(self.ws, nc.ctypes.data, ni.ctypes.data, nr.ctypes.data, off.ctypes.data))
        return nc, ni, nr, off

    def intervals(self, b):
        """Per-read lists of (intvl[N], rintvl[M]) after a run of at least STAGE_WALL / STAGE_REL."""
        nc, ni, nr, off = self.counts(b)
        tot = int(off[-1])
        iv = np.zeros(max(tot, 1), INTVL_DTYPE)
        rv = np.zeros(max(tot, 1), INTVL_DTYPE)
        check(self.L.cp_get_intervals(self.ws, iv.ctypes.data, rv.ctypes.data, max(tot, 1)))
        out = []
        for r in range(b.nreads):
            o = int(off[r])
            out.append((iv[o:o + ni[r]].copy(), rv[o:o + nr[r]].copy()))
        return out

    def rel_asgn(self, b):
        nc, ni, nr, off = self.counts(b)
        tot = int(off[-1])
        fw = np.zeros(max(tot, 1), np.int8)
        bw = np.zeros(max(tot, 1), np.int8)
        check(self.L.cp_get_rel_asgn(self.ws, fw.ctypes.data, bw.ctypes.data, max(tot, 1)))
        return [(fw[int(off[r]):int(off[r]) + nr[r]].copy(), bw[int(off[r]):int(off[r]) + nr[r]].copy())
                for r in range(b.nreads)]

    def bitmap(self, b):
        nw = b.total_kmers // 64 + 1
        w = np.zeros(nw, np.uint64)
        check(self.L.cp_get_bitmap(self.ws, w.ctypes.data, nw))
        return w

    def seq_context(self, b):
        """calc_seq_context (context.c:8), dense, per read: list of (lctx[rlen,3], rctx[rlen,3])."""
        l = torch.zeros((max(b.total_bases, 1), 3), dtype=torch.uint8, device=self.device)
        r = torch.zeros_like(l)
        check(self.L.cp_seq_context(b.seq.data_ptr(), b.seq_off.data_ptr(), b.nreads, b.total_bases,
                                    l.data_ptr(), r.data_ptr(), self._stream()))
        lh, rh = l.cpu().numpy(), r.cpu().numpy()
        so = b.seq_off_h
        return [(lh[so[i]:so[i + 1]], rh[so[i]:so[i + 1]]) for i in range(b.nreads)]


class KmerTable:
    """Per-k-mer label table on the device (cp_kmer_table_*; semantics in include/classpro_amd.h): counts, for every
    distinct k-mer, how often each label E/H/D/R was given to it across the reads added, then gives the consensus label
    per k-mer, the statistics and the consistency figure of the reference's agg2cons.py.  canonical=True keys a k-mer and
    its reverse complement together.  initial_slots only matters for tests that force growth."""

    LABELS = "EHDR"

    def __init__(self, K, canonical=False, device="cuda:0", initial_slots=0):
        from ._lib import KmerStats
        self.L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("classpro_amd runs on a HIP device only")
        torch.cuda.set_device(self.device)
        self.K, self.canonical = K, bool(canonical)
        self._Stats = KmerStats
        t = C.c_void_p()
        check(self.L.cp_kmer_table_create(K, int(self.canonical), int(initial_slots), C.byref(t)))
        self.t = t

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "t", None):
            self.L.cp_kmer_table_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_tensors(self, seq, seq_off, labels):
        """Adds a batch given as device tensors in the flat layout: seq uint8, seq_off int64 [n+1], labels uint8."""
        n = seq_off.numel() - 1
        total = int(seq_off[-1].item()) if n > 0 else 0
        check(self.L.cp_kmer_table_add(self.t, seq.data_ptr(), seq_off.data_ptr(), labels.data_ptr(), n, total,
                                       self._stream()))

    def add(self, b):
        """Adds a `Batch` labelled by Classifier.classify / run (its `labels` tensor)."""
        check(self.L.cp_kmer_table_add(self.t, b.seq.data_ptr(), b.seq_off.data_ptr(), b.labels.data_ptr(), b.nreads,
                                       b.total_bases, self._stream()))

    def stats(self):
        s = self._Stats()
        check(self.L.cp_kmer_table_stats(self.t, C.byref(s)))
        d = {f: getattr(s, f) for f, _ in s._fields_}
        d["label_total"] = list(s.label_total)
        d["cns_total"] = list(s.cns_total)
        d["s_fixed"] = (s.s_fixed_hi << 64) | s.s_fixed_lo
        return d

    def consensus_tensors(self, seq, seq_off, labels):
        """Consensus labels for a batch given as device tensors: a new uint8 tensor in the layout of `labels`."""
        out = labels.clone()
        n = seq_off.numel() - 1
        total = int(seq_off[-1].item()) if n > 0 else 0
        check(self.L.cp_kmer_table_consensus(self.t, seq.data_ptr(), seq_off.data_ptr(), n, total, out.data_ptr(),
                                             self._stream()))
        return out

    def consensus(self, b):
        """Consensus labels for the reads of a labelled `Batch`: a device uint8 tensor in the layout of b.labels (K-1 'N',
        then the consensus label of each k-mer; a skipped k-mer keeps its own label)."""
        out = b.labels.clone()
        check(self.L.cp_kmer_table_consensus(self.t, b.seq.data_ptr(), b.seq_off.data_ptr(), b.nreads, b.total_bases,
                                             out.data_ptr(), self._stream()))
        return out

    def entries(self):
        """Occupied entries in key order: numpy (hi uint64, lo uint64, counts uint32[n, 4] in order E, H, D, R), key =
        hi << 63 | lo."""
        n = check(self.L.cp_kmer_table_export(self.t, None, None, None, 0))
        hi, lo = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        cnt = np.zeros((max(n, 1), 4), np.uint32)
        m = check(self.L.cp_kmer_table_export(self.t, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, n))
        assert m == n
        return hi[:n], lo[:n], cnt[:n]

    def sorted(self, label=None, min_total=1, min_pct=0):
        """A `SortedKmers` snapshot of the table (cp_kmer_table_sort; "Sorted k-mers of a label table" in
        include/classpro_amd.h): the keys whose consensus label is `label` (one of "E" "H" "D" "R"; None: every key),
        whose four counts sum to at least min_total (in [1, 32767]) and whose largest count c has 100 * c >= min_pct *
        total (min_pct in [0, 100]), ascending by key; `.counts` holds the totals.  The table is only read and the
        snapshot does not follow later adds."""
        if label is not None and not (isinstance(label, str) and len(label) == 1 and label in self.LABELS):
            raise ValueError('label must be None or one of "E" "H" "D" "R"')
        s = C.c_void_p()
        check(self.L.cp_kmer_table_sort(self.t, -1 if label is None else self.LABELS.index(label), int(min_total),
                                        int(min_pct), self._stream(), C.byref(s)))
        return SortedKmers(self, s)

    def class_hist(self):
        """cp_kmer_table_class_hist: (hist int64 [4, 32767], ilowcnt int64 [4], ihighcnt int64 [4]) as numpy, the FASTK
        histogram of the keys of each consensus class in the order E, H, D, R, a key's total standing for its count."""
        h, il, ih = np.zeros((4, 32767), np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64)
        check(self.L.cp_kmer_table_class_hist(self.t, h.ctypes.data, il.ctypes.data, ih.ctypes.data))
        return h, il, ih


class KmerCounts:
    """K-mer count table on the device (cp_kmer_counts_*; semantics in include/classpro_amd.h): counts every canonical
    k-mer of the batches added, then gives the per-read count profiles and the FASTK histogram that ClassPro starts
    from.  initial_slots only matters for tests that force growth.

    With filter_bits > 0 (rounded up to a power of two in [64, 2^40]) the table is a FILTERED one, which keeps the
    k-mers seen once out of its slots: `mark` every batch, then `add` the same batches, then `profiles`.  Profiles,
    histogram and n_kmers, n_distinct, n_skipped are those of the unfiltered table, exactly; `rel_labels` is refused."""

    def __init__(self, K, device="cuda:0", initial_slots=0, filter_bits=0):
        from ._lib import KmerCountStats, KmerFilterStats
        self.L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("classpro_amd runs on a HIP device only")
        torch.cuda.set_device(self.device)
        self.K = K
        self._Stats, self._FilterStats = KmerCountStats, KmerFilterStats
        t = C.c_void_p()
        if filter_bits:
            check(self.L.cp_kmer_counts_create_filtered(K, int(initial_slots), int(filter_bits), C.byref(t)))
        else:
            check(self.L.cp_kmer_counts_create(K, int(initial_slots), C.byref(t)))
        self.t = t

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "t", None):
            self.L.cp_kmer_counts_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_tensors(self, seq, seq_off):
        """Adds a batch given as device tensors in the flat layout: seq uint8, seq_off int64 [n+1]."""
        n = seq_off.numel() - 1
        total = int(seq_off[-1].item()) if n > 0 else 0
        check(self.L.cp_kmer_counts_add(self.t, seq.data_ptr(), seq_off.data_ptr(), n, total, self._stream()))

    def add(self, b):
        """Adds the reads of a `Batch`."""
        check(self.L.cp_kmer_counts_add(self.t, b.seq.data_ptr(), b.seq_off.data_ptr(), b.nreads, b.total_bases,
                                        self._stream()))

    def add_keys(self, lo, hi=None):
        """cp_kmer_counts_add_keys: adds the explicit keys hi << 63 | lo, +1 each, given as flat int64 (or uint64) tensors
        of equal length; hi=None: every hi is 0.  Raises ClassProError (CP_EINVAL) on a filtered table, and -- after the
        pass, with the other keys added -- for a key that does not fit 2K bits or whose lo is negative."""
        lo = lo.to(self.device).contiguous()
        if lo.dim() != 1 or lo.dtype not in (torch.int64, torch.uint64):
            raise ValueError("lo must be a flat int64 tensor")
        if hi is not None:
            hi = hi.to(self.device).contiguous()
            if hi.shape != lo.shape or hi.dtype not in (torch.int64, torch.uint64):
                raise ValueError("hi must be a flat int64 tensor as long as lo")
        n = lo.numel()
        check(self.L.cp_kmer_counts_add_keys(self.t, hi.data_ptr() if hi is not None and n else None, lo.data_ptr() if n else None,
                                             n, self._stream()))

    def mark_tensors(self, seq, seq_off):
        """The mark pass of a filtered table over a batch given as device tensors (as `add_tensors`)."""
        n = seq_off.numel() - 1
        total = int(seq_off[-1].item()) if n > 0 else 0
        check(self.L.cp_kmer_counts_mark(self.t, seq.data_ptr(), seq_off.data_ptr(), n, total, self._stream()))

    def mark(self, b):
        """The mark pass of a filtered table over the reads of a `Batch`: every batch is marked before the first `add`."""
        check(self.L.cp_kmer_counts_mark(self.t, b.seq.data_ptr(), b.seq_off.data_ptr(), b.nreads, b.total_bases,
                                         self._stream()))

    def filter_stats(self):
        """dict: filter_bits, filter_bytes, n_marked, n_counted, n_table_keys, n_outside, n_false (cp_kmer_filter_stats)."""
        s = self._FilterStats()
        check(self.L.cp_kmer_counts_filter_stats(self.t, C.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def profiles(self, batch):
        """Count profiles of a `Batch` (its `prof` tensor is filled in place, ready for Classifier.classify) or of a
        tuple of device tensors (seq uint8, seq_off int64 [n+1]): a uint16 device tensor in the `prof` layout, read r at
        prof_off[r] = sum of max(rlen-(K-1), 0) over the reads before it."""
        if isinstance(batch, Batch):
            seq, seq_off, prof_off, n, total = batch.seq, batch.seq_off, batch.prof_off, batch.nreads, batch.total_bases
            nk, out = batch.total_kmers, batch.prof
        else:
            seq, seq_off = batch
            n = seq_off.numel() - 1
            total = int(seq_off[-1].item()) if n > 0 else 0
            prof_off = torch.zeros(n + 1, dtype=torch.int64, device=seq_off.device)
            torch.cumsum((seq_off[1:] - seq_off[:-1] - (self.K - 1)).clamp(min=0), 0, out=prof_off[1:])
            nk = int(prof_off[-1].item())
            out = torch.empty(max(nk, 8), dtype=torch.int16, device=seq_off.device)
        check(self.L.cp_kmer_counts_profiles(self.t, seq.data_ptr(), seq_off.data_ptr(), prof_off.data_ptr(), n, total,
                                             out.data_ptr(), self._stream()))
        return out.view(torch.uint16)[:nk]

    def rel_labels(self, batch, packed=False, profiles=False, counts=None):
        """cp_kmer_counts_rel_labels: the labels of a batch of ANOTHER sequence set against this table, the count c of
        each k-mer giving E (0: absent, or a byte other than upper-case A C G T), H (1), D (2) or R (>= 3) after
        min(K-1, rlen) 'N' per read.  `batch` is a `Batch` or a tuple of device tensors (seq uint8, seq_off int64
        [n+1]).  Returns (labels, counts), or (labels, prof, counts) with profiles=True: labels a uint8 device tensor of
        seq_off[n] characters that `LabelAccuracy.add` takes as it is -- or, with packed=True, the 2-bit bytes of
        cp_pack_labels and their int64 offsets as (packed, pack_off); prof the relative profile, min(c, 32767) as uint16
        in the `prof` layout (a `Batch`'s own `prof` tensor is filled in place, as `profiles()` does); counts an int64
        device tensor [4], order E, H, D, R.  Pass a previous `counts` tensor to go on adding to it.  The table is not
        changed and an absent k-mer is no error.  Nothing is copied to the host."""
        if isinstance(batch, Batch):
            seq, seq_off, n, total = batch.seq, batch.seq_off, batch.nreads, batch.total_bases
        else:
            seq, seq_off = batch
            n = seq_off.numel() - 1
            total = int(seq_off[-1].item()) if n > 0 else 0
        dev = seq_off.device
        prof = prof_off = None
        nk = 0
        if profiles:
            if isinstance(batch, Batch):
                prof, prof_off, nk = batch.prof, batch.prof_off, batch.total_kmers
            else:
                prof_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                torch.cumsum((seq_off[1:] - seq_off[:-1] - (self.K - 1)).clamp(min=0), 0, out=prof_off[1:])
                nk = int(prof_off[-1].item()) if n > 0 else 0
                prof = torch.empty(max(nk, 8), dtype=torch.int16, device=dev)
        if counts is None:
            counts = torch.zeros(4, dtype=torch.int64, device=dev)
        lab = pk = pack_off = None
        if packed:
            pack_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum((seq_off[1:] - seq_off[:-1] + 3) >> 2, 0, out=pack_off[1:])
            pk = torch.empty(max(int(pack_off[-1].item()) if n > 0 else 0, 1), dtype=torch.uint8, device=dev)
        else:
            lab = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        ptr = lambda x: x.data_ptr() if x is not None else None
        check(self.L.cp_kmer_counts_rel_labels(self.t, seq.data_ptr(), seq_off.data_ptr(), n, total, ptr(prof),
                                               ptr(prof_off), ptr(lab), ptr(pk), ptr(pack_off), counts.data_ptr(),
                                               self._stream()))
        out = (pk, pack_off) if packed else lab[:total]
        if profiles:
            return out, prof.view(torch.uint16)[:nk], counts
        return out, counts

    def hist(self):
        """The FASTK histogram of the table as `hist_covs` and `fastk.write_fastk` take it:
        (1, 32767, ilowcnt, ihighcnt, int64[32767])."""
        h = np.zeros(32767, np.int64)
        il, ih = C.c_int64(), C.c_int64()
        check(self.L.cp_kmer_counts_hist(self.t, h.ctypes.data, C.byref(il), C.byref(ih)))
        return 1, 32767, il.value, ih.value, h

    def stats(self):
        """dict: n_kmers, n_skipped, n_distinct, slots, bytes, growths.  Raises ClassProError (CP_EINVAL) once after a
        profile pass that met a k-mer that was never added."""
        s = self._Stats()
        check(self.L.cp_kmer_counts_stats(self.t, C.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def sorted(self, min_count=1):
        """A `SortedKmers` snapshot of the table: every key with count >= min_count (in [1, 32767]; at least 2 on a
        filtered table), ascending by key.  The table is only read and the snapshot does not follow later adds."""
        s = C.c_void_p()
        check(self.L.cp_kmer_counts_sort(self.t, int(min_count), self._stream(), C.byref(s)))
        return SortedKmers(self, s)


class SortedKmers:
    """A sorted snapshot of a `KmerCounts` or a `KmerTable`, or one loaded from a FASTK k-mer table (`from_records`,
    `from_ktab`), which `find` and `profiles` query (cp_kmer_sorted_*; semantics in include/classpro_amd.h, "Sorted k-mers"
    and "Sorted k-mers as input").  len() is the number of entries; `.hi`, `.lo` (key = hi << 63 | lo) and `.counts` (exact) are int64 device
    tensors that VIEW the snapshot's memory; `.nbytes` is the device memory held.  A tensor taken from them keeps the
    snapshot alive, so the memory is freed when the object and all such tensors are gone -- or at once by `close()`,
    after which any tensor still held points at freed memory: clone what has to outlive an explicit `close()`."""

    def __init__(self, table, handle):
        self.L, self.device, self.K = table.L, table.device, table.K
        self._adopt(handle)

    def _adopt(self, handle):
        self.s = handle
        self.n = check(self.L.cp_kmer_sorted_size(self.s))
        self.nbytes = check(self.L.cp_kmer_sorted_bytes(self.s))
        p = [C.c_void_p() for _ in range(3)]
        check(self.L.cp_kmer_sorted_arrays(self.s, *[C.byref(x) for x in p]))
        self._ptr = [x.value for x in p]

    hi = property(lambda self: self._view(0))
    lo = property(lambda self: self._view(1))
    counts = property(lambda self: self._view(2))

    def _view(self, which):
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if self.n == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        ptr = self._ptr[which]
        iface = {"shape": (self.n,), "typestr": "<i8", "data": (ptr, False), "version": 2, "strides": None}
        # torch keeps `holder` for the life of the tensor and of every view of it; the holder keeps this object, so a
        # tensor that outlives the last name of the SortedKmers (`T.sorted().hi`) still points at live memory.  The
        # object itself holds no tensor (a new one per access), so there is no cycle through torch to keep it alive.
        holder = type("_KsView", (), {"__cuda_array_interface__": iface, "owner": self})()
        return torch.as_tensor(holder, device=self.device)

    def __len__(self):
        return self.n

    @classmethod
    def from_records(cls, K, index, records, device="cuda:0", piece=None):
        """A snapshot loaded from the payload of a FASTK k-mer table (cp_kmer_sorted_load_*; "Sorted k-mers as input" in
        include/classpro_amd.h): `index` the stub's int64 prefix index (numpy or tensor), `records` the records of all
        parts in file order as uint8 (numpy, or a tensor on the host or the device, any alignment), loaded in pieces of
        `piece` entries (None: one piece).  Raises ClassProError (CP_EINVAL) for an index that decreases, records that
        do not match it, or keys that are not strictly ascending."""
        self = cls.__new__(cls)
        self.L, self.device, self.K, self.s = lib(), torch.device(device), K, None
        if self.device.type != "cuda":
            raise ValueError("classpro_amd runs on a HIP device only")
        torch.cuda.set_device(self.device)
        idx = np.ascontiguousarray(index.cpu().numpy() if isinstance(index, torch.Tensor) else index, np.int64)
        ibyte = self.L.cp_ktab_ibyte(K)
        if ibyte and len(idx) != 1 << (8 * ibyte):
            raise ValueError("the index of a table of %d-mers has %d cells" % (K, 1 << (8 * ibyte)))
        pbyte = ((K + 3) >> 2) - ibyte + 2
        rec = records if isinstance(records, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(records, np.uint8))
        if rec.dtype != torch.uint8 or rec.dim() != 1 or rec.numel() % pbyte:
            raise ValueError("records must be a flat uint8 array of whole %d-byte records" % pbyte)
        n = rec.numel() // pbyte
        piece = max(n, 1) if piece is None else int(piece)
        if piece < 1:
            raise ValueError("piece must be positive")
        h = C.c_void_p()
        check(self.L.cp_kmer_sorted_load_begin(K, idx.ctypes.data, C.byref(h)))
        try:
            for e in range(0, n, piece):
                m = min(piece, n - e)
                part = rec[e * pbyte:(e + m) * pbyte]
                part = part if part.device == self.device else part.to(self.device)
                check(self.L.cp_kmer_sorted_load_records(h, m, part.data_ptr(), _stream_of(self.device)))
            check(self.L.cp_kmer_sorted_load_end(h, _stream_of(self.device)))
        except Exception:
            self.L.cp_kmer_sorted_destroy(h)
            raise
        self._adopt(h)
        return self

    @classmethod
    def from_ktab(cls, dirpath, root, device="cuda:0", piece=1 << 22):
        """`from_records` of the table `<dirpath>/<root>.ktab` and its parts (fastk.read_fastk_ktab_raw)."""
        from .fastk import read_fastk_ktab_raw
        K, _minval, _ibyte, index, records = read_fastk_ktab_raw(dirpath, root)
        return cls.from_records(K, index, records, device=device, piece=piece)

    def find(self, hi, lo):
        """cp_kmer_sorted_find: for keys hi << 63 | lo given as int64 device tensors of equal length, an int64 device
        tensor of their ordinals in the snapshot, -1 for a key that is absent."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if hi.shape != lo.shape or hi.dim() != 1 or hi.dtype != torch.int64 or lo.dtype != torch.int64:
            raise ValueError("hi and lo must be flat int64 tensors of equal length")
        hi, lo = hi.to(self.device).contiguous(), lo.to(self.device).contiguous()
        pos = torch.empty(hi.numel(), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_find(self.s, hi.data_ptr() if hi.numel() else None, lo.data_ptr() if hi.numel() else None,
                                             hi.numel(), pos.data_ptr() if hi.numel() else None, _stream_of(self.device)))
        return pos

    def profiles(self, batch, canonical=True, tally=None):
        """cp_kmer_sorted_profiles: the profiles of a `Batch` (its `prof` tensor is filled in place, ready for
        `threshold_labels` and `Classifier.classify`) or of a tuple of device tensors (seq uint8, seq_off int64 [n+1])
        RELATIVE to this snapshot: per k-mer min(count, 32767) of its key, 0 for a key that is absent and for a k-mer
        with a byte other than upper-case A C G T.  canonical=False looks the forward k-mer up (the snapshots of a
        forward `KmerTable`).  `tally`, an int64 device tensor [3], is added to: cells present, absent, with other
        bytes.  Returns a uint16 device tensor in the `prof` layout, as `KmerCounts.profiles` does."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if isinstance(batch, Batch):
            seq, seq_off, prof_off, n, total = batch.seq, batch.seq_off, batch.prof_off, batch.nreads, batch.total_bases
            nk, out = batch.total_kmers, batch.prof
        else:
            seq, seq_off = batch
            n = seq_off.numel() - 1
            total = int(seq_off[-1].item()) if n > 0 else 0
            prof_off = torch.zeros(n + 1, dtype=torch.int64, device=seq_off.device)
            torch.cumsum((seq_off[1:] - seq_off[:-1] - (self.K - 1)).clamp(min=0), 0, out=prof_off[1:])
            nk = int(prof_off[-1].item())
            out = torch.empty(max(nk, 8), dtype=torch.int16, device=seq_off.device)
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_profiles(self.s, 1 if canonical else 0, seq.data_ptr(), seq_off.data_ptr(),
                                                 prof_off.data_ptr(), n, total, out.data_ptr(),
                                                 tally.data_ptr() if tally is not None else None, _stream_of(self.device)))
        return out.view(torch.uint16)[:nk]

    def ktab(self, first=0, n=None):
        """(records, index): the FASTK .ktab records of the entries [first, first+n) (n = None: to the end) as a uint8
        device tensor, and the prefix index of the WHOLE snapshot as an int64 device tensor of 1 << 8*ibyte."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        n = self.n - first if n is None else n
        ibyte = self.L.cp_ktab_ibyte(self.K)
        pbyte = ((self.K + 3) >> 2) - ibyte + 2
        rec = torch.empty(max(n, 0) * pbyte, dtype=torch.uint8, device=self.device)
        idx = torch.empty((1 << (8 * ibyte)) if ibyte else 0, dtype=torch.int64, device=self.device)
        check(self.L.cp_kmer_sorted_ktab(self.s, int(first), int(n), rec.data_ptr() if rec.numel() else None,
                                         idx.data_ptr() if idx.numel() else None,
                                         C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return rec, idx

    _SET_OPS = {"and": 0, "or": 1, "sub": 2, "xor": 3}
    _CNT_OPS = {"left": 0, "sum": 1, "min": 2, "max": 3}

    def _combine(self, other, op, count, a_range, b_range, build):
        if op not in self._SET_OPS:
            raise ValueError("op must be one of 'and', 'or', 'sub', 'xor'")
        if count not in self._CNT_OPS:
            raise ValueError("count must be one of 'left', 'sum', 'min', 'max'")
        if not isinstance(other, SortedKmers):
            raise ValueError("the other operand must be a SortedKmers")
        if self.s is None or other.s is None:
            raise ValueError("SortedKmers is closed")
        if other.K != self.K or other.device != self.device:
            raise ValueError("the operands must hold k-mers of the same length on the same device")
        rng = self._range4(a_range, b_range)
        tally = (C.c_int64 * 4)()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_combine(self.s, other.s, self._SET_OPS[op], self._CNT_OPS[count], rng, tally,
                                                _stream_of(self.device), C.byref(h) if build else None))
        return h, tuple(tally)

    def combine(self, other, op, count="left", a_range=None, b_range=None):
        """cp_kmer_sorted_combine ("Set algebra on sorted k-mers" in include/classpro_amd.h): this snapshot (A) and
        `other` (B) of the same K as a new `SortedKmers`.  `op` is "and", "or", "sub" or "xor"; `count` is "left", "sum",
        "min" or "max"; a range is (lo, hi) on the operand's counts, either end None for open, and an entry outside its
        range counts as absent.  The result has `.tally == (only_a, only_b, both, out)`, holds memory of its own and keeps
        no reference to either operand.  Both operands are only read; `other` may be `self`."""
        h, tally = self._combine(other, op, count, a_range, b_range, True)
        out = SortedKmers.__new__(SortedKmers)
        out.L, out.device, out.K = self.L, self.device, self.K
        out._adopt(h)
        out.tally = tally
        return out

    @staticmethod
    def _range4(a_range, b_range):
        if a_range is None and b_range is None:
            return None
        ends = []
        for r in (a_range, b_range):
            lo, hi = (None, None) if r is None else r
            ends += [1 if lo is None else int(lo), (1 << 63) - 1 if hi is None else int(hi)]
        return (C.c_int64 * 4)(*ends)

    def read_hits(self, other, batch, canonical=True, a_range=None, b_range=None):
        """cp_kmer_sorted_read_hits ("Read hits in two sorted k-mer sets" in include/classpro_amd.h): this snapshot (A)
        and `other` (B) of the same K looked up together for every k-mer of a `Batch` or of a tuple of device tensors (seq
        uint8, seq_off int64 [n+1]).  Returns an int64 device tensor [n, 5]: per read the positions whose key is only in
        A, only in B, in both, the positions with a byte other than upper-case A C G T, and the number of times the A/B
        markers switch sides along the read.  Ranges are those of `combine`; `other` may be `self`."""
        if not isinstance(other, SortedKmers):
            raise ValueError("the other operand must be a SortedKmers")
        if self.s is None or other.s is None:
            raise ValueError("SortedKmers is closed")
        if other.K != self.K or other.device != self.device:
            raise ValueError("the operands must hold k-mers of the same length on the same device")
        if isinstance(batch, Batch):
            seq, seq_off, n, total = batch.seq, batch.seq_off, batch.nreads, batch.total_bases
        else:
            seq, seq_off = batch
            n = seq_off.numel() - 1
            total = int(seq_off[-1].item()) if n > 0 else 0
        hits = torch.empty((max(n, 0), 5), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_read_hits(self.s, other.s, 1 if canonical else 0, self._range4(a_range, b_range),
                                                  seq.data_ptr(), seq_off.data_ptr(), n, total,
                                                  hits.data_ptr() if n > 0 else None, _stream_of(self.device)))
        return hits

    RUN_NONE, RUN_A, RUN_B, RUN_BOTH, RUN_OTHER = 1, 2, 4, 8, 16      # the bits of `skip` and `emit`: 1 << state

    def read_runs(self, other, batch, skip=0, emit=None, canonical=True, a_range=None, b_range=None):
        """cp_kmer_sorted_read_runs ("Runs of k-mer states along reads" in include/classpro_amd.h): the k-mer positions of
        a `Batch` or of a tuple of device tensors (seq uint8, seq_off int64 [n+1]) looked up in this snapshot (A) and in
        `other` (B, or None for no second table) and reduced to runs of equal state on the device.  `skip` and `emit`
        are masks of 1 << state (states 0 none, 1 A, 2 B, 3 both, 4 other byte); positions in `skip` are transparent, runs
        outside `emit` (default: every state not skipped) are not returned.  Returns (run_off, runs): run_off an int64
        device tensor [n+1], the runs of read r being records run_off[r] .. run_off[r+1]; runs a dict of device tensors
        "first", "last", "n" (int64) and "read", "state" (int32).  One call with a guessed capacity, one more at the exact
        size when that was too small."""
        if other is not None and not isinstance(other, SortedKmers):
            raise ValueError("the other operand must be a SortedKmers or None")
        if self.s is None or (other is not None and other.s is None):
            raise ValueError("SortedKmers is closed")
        if other is not None and (other.K != self.K or other.device != self.device):
            raise ValueError("the operands must hold k-mers of the same length on the same device")
        skip = int(skip)
        emit = 0x1f & ~skip if emit is None else int(emit)
        if isinstance(batch, Batch):
            seq, seq_off, n, total = batch.seq, batch.seq_off, batch.nreads, batch.total_bases
        else:
            seq, seq_off = batch
            n = seq_off.numel() - 1
            total = int(seq_off[-1].item()) if n > 0 else 0
        run_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=self.device)
        capacity = max(1024, total // 16)
        count = C.c_int64()
        with torch.cuda.device(self.device):
            for _ in range(2):
                buf = torch.empty((capacity, 4), dtype=torch.int64, device=self.device)
                rc = self.L.cp_kmer_sorted_read_runs(self.s, other.s if other is not None else None, 1 if canonical else 0,
                                                     self._range4(a_range, b_range), skip, emit, seq.data_ptr(),
                                                     seq_off.data_ptr(), n, total, buf.data_ptr(), capacity,
                                                     run_off.data_ptr(), C.byref(count), _stream_of(self.device))
                if rc != CP_EOVERFLOW:                     # count is exact: once more at that size
                    break
                capacity = count.value
            check(rc)
        buf = buf[:count.value]
        tail = buf.view(torch.int32)[:, 6:]
        return run_off, {"first": buf[:, 0], "last": buf[:, 1], "n": buf[:, 2], "read": tail[:, 0], "state": tail[:, 1]}

    FIX_NONE, FIX_ONE, FIX_MANY, FIX_OPEN, FIX_NOCAND, FIX_CLASH = range(6)              # the status of a gap
    FIX_TALLY = ("none", "one", "many", "open", "nocand", "clash")

    @staticmethod
    def _flat_batch(batch):
        if isinstance(batch, Batch):
            return batch.seq, batch.seq_off, batch.nreads, batch.total_bases
        seq, seq_off = batch
        n = seq_off.numel() - 1
        return seq, seq_off, n, int(seq_off[-1].item()) if n > 0 else 0

    def read_fixes(self, batch, max_indel=1, canonical=True, count_range=None, capacity=None):
        """cp_kmer_sorted_read_fixes ("Fixing reads from a k-mer table" in include/classpro_amd.h): the gaps of a `Batch` or
        of a tuple of device tensors (seq uint8, seq_off int64 [n+1]) -- the runs of k-mer positions whose key this
        snapshot does not hold, or holds with a count outside `count_range` = (lo, hi), either end None for open -- each
        with the one edit of at most `max_indel` inserted or removed bases that closes it, where there is exactly one.
        Returns (fix_off, fixes, tally): fix_off an int64 device tensor [n+1], the gaps of read r being records
        fix_off[r] .. fix_off[r+1]; fixes a dict of device tensors "first", "last" (int64), "read" (int32), "status", "del",
        "nins", "nacc" (uint8), "ins" (uint8 [., 8]) and "records" (int64 [., 4], the records as `apply_fixes` takes them;
        the others are views of it); tally a dict of FIX_TALLY, the gaps by status.  One call with a guessed capacity
        (`capacity` records when given, else one per 16 bases), one more at the exact size when that was too small."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        seq, seq_off, n, total = self._flat_batch(batch)
        rng = None
        if count_range is not None:
            lo, hi = count_range
            rng = (C.c_int64 * 2)(1 if lo is None else int(lo), (1 << 63) - 1 if hi is None else int(hi))
        fix_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=self.device)
        tally = torch.zeros(6, dtype=torch.int64, device=self.device)
        capacity = max(1024, total // 16) if capacity is None else max(int(capacity), 0)
        count = C.c_int64()
        with torch.cuda.device(self.device):
            for _ in range(2):
                buf = torch.empty((capacity, 4), dtype=torch.int64, device=self.device)
                rc = self.L.cp_kmer_sorted_read_fixes(self.s, 1 if canonical else 0, rng, int(max_indel), seq.data_ptr(),
                                                      seq_off.data_ptr(), n, total, buf.data_ptr() if capacity else None,
                                                      capacity, fix_off.data_ptr(), C.byref(count), tally.data_ptr(),
                                                      _stream_of(self.device))
                if rc != CP_EOVERFLOW:                     # count is exact: once more at that size
                    break
                capacity = count.value
            check(rc)
        buf = buf[:count.value]
        b8 = buf.view(torch.uint8)
        fixes = {"first": buf[:, 0], "last": buf[:, 1], "read": buf.view(torch.int32)[:, 4], "status": b8[:, 20], "del": b8[:, 21],
                 "nins": b8[:, 22], "nacc": b8[:, 23], "ins": b8[:, 24:32], "records": buf}
        return fix_off, fixes, dict(zip(self.FIX_TALLY, tally.cpu().tolist()))

    def apply_fixes(self, batch, fix_off, fixes):
        """cp_apply_fixes: the batch with the fixes of status FIX_ONE applied and nothing else.  `fix_off` and `fixes` are
        what `read_fixes` of this batch returned (`fixes` the dict, or its "records" tensor).  Returns (seq, seq_off) as
        device tensors, uint8 and int64 [n+1]: a batch that every call here takes."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        seq, seq_off, n, total = self._flat_batch(batch)
        rec = fixes["records"] if isinstance(fixes, dict) else fixes
        if rec.dtype != torch.int64 or rec.dim() != 2 or rec.shape[1] != 4 or not rec.is_contiguous() or rec.device != self.device:
            raise ValueError("fixes must be the contiguous int64 records [., 4] of read_fixes on the snapshot's device")
        if fix_off.dtype != torch.int64 or fix_off.numel() != max(n, 0) + 1 or not fix_off.is_contiguous() or fix_off.device != self.device:
            raise ValueError("fix_off must be a contiguous int64 tensor [n+1] on the snapshot's device")
        if n > 0 and int(fix_off[-1].item()) > rec.shape[0]:
            raise ValueError("fix_off counts more records than fixes holds")
        capacity = total + 4 * rec.shape[0]
        out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=self.device)
        out_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=self.device)
        count = C.c_int64()
        with torch.cuda.device(self.device):
            check(self.L.cp_apply_fixes(seq.data_ptr(), seq_off.data_ptr(), n, total, self.K, rec.data_ptr() if rec.shape[0] else None,
                                        fix_off.data_ptr(), out.data_ptr(), capacity, out_off.data_ptr(), C.byref(count),
                                        _stream_of(self.device)))
        return out[:count.value], out_off

    PATH_TALLY = ("positions", "present", "absent", "other", "segments", "joined", "walks")

    def read_paths(self, U, batch, coverage=None, support=None, capacity=None):
        """cp_kmer_sorted_read_paths ("Reads through the unitig graph" in include/classpro_amd.h): the k-mer positions of a
        `Batch` or of a tuple of device tensors (seq uint8, seq_off int64 [n+1]) located in the unitigs `U` of this
        snapshot -- a `Unitigs` made by `unitigs(where=True)`; `support` also needs `links=True` -- and reduced to segments
        on the device.  Returns (seg_off, segs, tally): seg_off an int64 device tensor [n+1], the segments of read r
        being records seg_off[r] .. seg_off[r+1]; segs a dict of device tensors "first", "x" (int64) and "n", "q", "read",
        "flags" (int32); tally a dict of PATH_TALLY.  coverage=True / support=True allocate zeroed int64 tensors [len(U)]
        / [U.nlinks] and return them as tally["coverage"] / tally["support"]; a tensor passed instead is added to and
        returned there.  One call with a guessed capacity (`capacity` records when given, else one per 16 bases), one
        more at the exact size when that was too small (the call that overflows adds nothing to either tensor)."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if not isinstance(U, Unitigs) or U.u is None:
            raise ValueError("U must be a Unitigs that holds its sequences")
        if U.K != self.K or U.device != self.device:
            raise ValueError("the unitigs must be of this snapshot's K and device")
        if U.utg is None or U.at is None or U.utg.numel() != self.n:
            raise ValueError("the unitigs must be made with where=True from this snapshot")
        want_sup = support is not None and support is not False
        want_cov = coverage is not None and coverage is not False
        if want_sup and U.g is None:
            raise ValueError("support needs unitigs made with links=True")
        cov = sup = None
        if want_cov:
            cov = torch.zeros(len(U), dtype=torch.int64, device=self.device) if coverage is True else coverage
            if cov.dtype != torch.int64 or cov.dim() != 1 or cov.numel() != len(U) or cov.device != self.device or not cov.is_contiguous():
                raise ValueError("coverage must be a contiguous int64 tensor of len(U) on the snapshot's device")
        if want_sup:
            sup = torch.zeros(U.nlinks, dtype=torch.int64, device=self.device) if support is True else support
            if sup.dtype != torch.int64 or sup.dim() != 1 or sup.numel() != U.nlinks or sup.device != self.device or not sup.is_contiguous():
                raise ValueError("support must be a contiguous int64 tensor of U.nlinks on the snapshot's device")
        if isinstance(batch, Batch):
            seq, seq_off, n, total = batch.seq, batch.seq_off, batch.nreads, batch.total_bases
        else:
            seq, seq_off = batch
            n = seq_off.numel() - 1
            total = int(seq_off[-1].item()) if n > 0 else 0
        seg_off = torch.zeros(max(n, 0) + 1, dtype=torch.int64, device=self.device)
        capacity = max(1024, total // 16) if capacity is None else max(int(capacity), 1)
        count = C.c_int64()
        tally = (C.c_int64 * len(self.PATH_TALLY))()
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        with torch.cuda.device(self.device):
            for _ in range(2):
                buf = torch.empty((capacity, 4), dtype=torch.int64, device=self.device)
                rc = self.L.cp_kmer_sorted_read_paths(self.s, U.u, ptr(U.utg), ptr(U.at), U.g if want_sup else None,
                                                      seq.data_ptr(), seq_off.data_ptr(), n, total, buf.data_ptr(), capacity,
                                                      seg_off.data_ptr(), ptr(cov), ptr(sup), tally, C.byref(count),
                                                      _stream_of(self.device))
                if rc != CP_EOVERFLOW:                     # count is exact: once more at that size
                    break
                capacity = count.value
            check(rc)
        buf = buf[:count.value]
        tail = buf.view(torch.int32)[:, 4:]
        res = dict(zip(self.PATH_TALLY, tally))
        if want_cov:
            res["coverage"] = cov
        if want_sup:
            res["support"] = sup
        return seg_off, {"first": buf[:, 0], "x": buf[:, 1], "n": tail[:, 0], "q": tail[:, 1], "read": tail[:, 2],
                         "flags": tail[:, 3]}, res

    def compare(self, other, a_range=None, b_range=None):
        """(only_a, only_b, both): the tally of `combine` with nothing built (cp_kmer_sorted_combine with out == NULL)."""
        return self._combine(other, "and", "left", a_range, b_range, False)[1][:3]

    _CMP_WEIGHTS = {"keys": 0, "a": 1, "b": 2}

    def compare_hist(self, other, xmax=8, ymax=1000, weight="keys", a_range=None, b_range=None):
        """cp_kmer_sorted_compare_hist ("Count comparison of sorted k-mers" in include/classpro_amd.h): a numpy int64
        [xmax+1, ymax+1] whose cell [x, y] sums, over the keys with min(count in this snapshot, xmax) == x and
        min(count in `other`, ymax) == y (0 for a side the key is not in), 1 for weight "keys", this snapshot's count
        for "a" and the other's for "b".  Ranges are those of `combine`; `other` may be `self`."""
        if weight not in self._CMP_WEIGHTS:
            raise ValueError("weight must be one of 'keys', 'a', 'b'")
        if not isinstance(other, SortedKmers):
            raise ValueError("the other operand must be a SortedKmers")
        if self.s is None or other.s is None:
            raise ValueError("SortedKmers is closed")
        if other.K != self.K or other.device != self.device:
            raise ValueError("the operands must hold k-mers of the same length on the same device")
        xmax, ymax = int(xmax), int(ymax)
        if not (1 <= xmax <= 32767 and 1 <= ymax <= 32767 and (xmax + 1) * (ymax + 1) <= 1 << 22):
            raise ValueError("xmax and ymax must lie in [1, 32767] and span at most 2^22 cells")
        mat = np.zeros((xmax + 1, ymax + 1), np.int64)
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_compare_hist(self.s, other.s, self._range4(a_range, b_range),
                                                     self._CMP_WEIGHTS[weight], xmax, ymax, mat.ctypes.data,
                                                     _stream_of(self.device)))
        return mat

    _HET_TALLY = ("keys", "paired", "multi", "pairs", "unique", "out")

    def het_pairs(self, xmax=1000, ymax=1000, unique=True, count_range=None, degrees=False, table=False):
        """cp_kmer_sorted_het_pairs ("Heterozygous pairs of sorted k-mers" in include/classpro_amd.h): the pairs of keys
        of this snapshot that differ only at the centre base.  Returns (matrix, tally): a numpy int64 [xmax+1, ymax+1]
        whose cell [a, b] counts the pairs with min(smaller count, xmax) == a and min(larger count, ymax) == b -- the
        unique pairs (both members have no other partner) with unique=True, every pair otherwise -- and a dict with
        "keys", "paired", "multi", "pairs", "unique" and "out".  `count_range` is (lo, hi) as in `combine`: a key outside
        it counts as absent.  degrees=True appends the degree of every entry as a uint8 device tensor, table=True a
        new `SortedKmers` of the members of the counted pairs, which keeps no reference to this one."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        xmax, ymax = int(xmax), int(ymax)
        if not (1 <= xmax <= 32767 and 1 <= ymax <= 32767 and (xmax + 1) * (ymax + 1) <= 1 << 22):
            raise ValueError("xmax and ymax must lie in [1, 32767] and span at most 2^22 cells")
        rng = None
        if count_range is not None:
            lo, hi = count_range
            rng = (C.c_int64 * 2)(1 if lo is None else int(lo), (1 << 63) - 1 if hi is None else int(hi))
        mat = np.zeros((xmax + 1, ymax + 1), np.int64)
        tally = (C.c_int64 * 6)()
        deg = torch.zeros(self.n, dtype=torch.uint8, device=self.device) if degrees else None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_het_pairs(self.s, rng, 1 if unique else 0, xmax, ymax, mat.ctypes.data, tally,
                                                  deg.data_ptr() if degrees and self.n else None, _stream_of(self.device),
                                                  C.byref(h) if table else None))
        res = [mat, dict(zip(self._HET_TALLY, tally))]
        if degrees:
            res.append(deg)
        if table:
            out = SortedKmers.__new__(SortedKmers)
            out.L, out.device, out.K = self.L, self.device, self.K
            out._adopt(h)
            res.append(out)
        return tuple(res)

    def _derived(self, handle):
        out = SortedKmers.__new__(SortedKmers)
        out.L, out.device, out.K = self.L, self.device, self.K
        out._adopt(handle)
        return out

    def het_sites(self, mates=False):
        """cp_kmer_sorted_het_sites ("Phasing heterozygous sites from reads" in include/classpro_amd.h): the entries of this
        snapshot of heterozygous k-mers paired into sites.  Returns (mark, nsites, tally): mark an int32 device tensor
        [len], site << 1 | allele for a mated entry and -1 otherwise; tally a dict with "mated" and "unmated".  mates=True
        appends mate, an int64 device tensor [len]."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        mark = torch.empty(self.n, dtype=torch.int32, device=self.device)
        mate = torch.empty(self.n, dtype=torch.int64, device=self.device) if mates else None
        ns, tally = C.c_int64(), (C.c_int64 * 2)()
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_het_sites(self.s, mate.data_ptr() if mates and self.n else None,
                                                  mark.data_ptr() if self.n else None, C.byref(ns), tally, _stream_of(self.device)))
        res = (mark, ns.value, {"mated": tally[0], "unmated": tally[1]})
        return res + (mate,) if mates else res

    LINK_TALLY = ("markers", "links", "self")

    def read_links(self, batch, mark, capacity=None, canonical=True, tally=None):
        """cp_kmer_sorted_read_links: the links of a `Batch` or of a tuple of device tensors (seq uint8, seq_off int64
        [n+1]) under `mark` (of `het_sites`), in batch order.  Returns (links, tally): links an int64 device tensor of the
        keys min(s,s') << 32 | max(s,s') << 1 | (a ^ a'); tally an int64 device tensor [3], order LINK_TALLY, which is
        added to -- pass a previous one to go on.  capacity=None: a counting call, then the call at the exact size; with a
        capacity that is too small ClassProError (CP_EOVERFLOW) is raised and the tally is untouched."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        seq, seq_off, n, total = self._flat_batch(batch)
        if mark.dtype != torch.int32 or mark.numel() != self.n or not mark.is_contiguous() or mark.device != self.device:
            raise ValueError("mark must be the contiguous int32 tensor [len] of het_sites on the snapshot's device")
        if tally is None:
            tally = torch.zeros(3, dtype=torch.int64, device=self.device)
        count = C.c_int64()
        args = (self.s, mark.data_ptr() if self.n else None, 1 if canonical else 0, seq.data_ptr(), seq_off.data_ptr(), n, total)
        with torch.cuda.device(self.device):
            if capacity is None:
                rc = self.L.cp_kmer_sorted_read_links(*args, None, 0, C.byref(count), None, _stream_of(self.device))
                if rc != CP_EOVERFLOW:
                    check(rc)
                capacity = count.value
            capacity = max(int(capacity), 0)
            buf = torch.empty(max(capacity, 1), dtype=torch.int64, device=self.device)
            check(self.L.cp_kmer_sorted_read_links(*args, buf.data_ptr() if capacity else None, capacity, C.byref(count),
                                                   tally.data_ptr(), _stream_of(self.device)))
        return buf[:count.value], tally

    def phase_split(self, mark, block, side):
        """cp_kmer_sorted_phase_split: the two marker tables (A, B) of this snapshot under `mark` (of `het_sites`) and
        `block`, `side` (of `phase_forest`): new `SortedKmers` that keep no reference to this one."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if mark.dtype != torch.int32 or mark.numel() != self.n or block.dtype != torch.int64 or side.dtype != torch.uint8 \
                or block.numel() != side.numel():
            raise ValueError("mark int32 [len], block int64 [nsites] and side uint8 [nsites] are wanted")
        mark, block, side = mark.contiguous(), block.contiguous(), side.contiguous()
        ns, out = block.numel(), []
        with torch.cuda.device(self.device):
            for which in (0, 1):
                h = C.c_void_p()
                check(self.L.cp_kmer_sorted_phase_split(self.s, mark.data_ptr() if self.n else None, block.data_ptr() if ns else None,
                                                        side.data_ptr() if ns else None, ns, which, _stream_of(self.device),
                                                        C.byref(h)))
                out.append(self._derived(h))
        return tuple(out)

    def phase(self, batches, count_range=None, min_support=2, canonical=True):
        """The driver of "Phasing heterozygous sites from reads": P = the unique heterozygous pairs of this snapshot under
        `count_range` (`het_pairs`), its sites, the links of every batch of `batches` (an iterable of what `read_links`
        takes) accumulated in a `KmerCounts` of K = 32, the forest and the split.  Returns a dict: "P", "A", "B"
        (`SortedKmers`), "mark", "block", "side" (device tensors), "nsites", and the tallies "sites" (mated, unmated),
        "links" (LINK_TALLY) and "forest" (PHASE_TALLY).  The phase of one block relative to another is arbitrary."""
        P = self.het_pairs(xmax=1, ymax=1, unique=True, count_range=count_range, table=True)[2]
        acc = edges = None
        try:
            mark, ns, sites = P.het_sites()
            acc = KmerCounts(32, device=self.device)
            tally = torch.zeros(3, dtype=torch.int64, device=self.device)
            for b in batches:
                links, tally = P.read_links(b, mark, canonical=canonical, tally=tally)
                acc.add_keys(links)
            edges = acc.sorted(1)
            block, side, forest = phase_forest(edges, ns, min_support)
            A, B = P.phase_split(mark, block, side)
        except Exception:
            P.close()
            raise
        finally:
            if edges is not None:
                edges.close()
            if acc is not None:
                acc.close()
        return {"P": P, "A": A, "B": B, "mark": mark, "block": block, "side": side, "nsites": ns, "sites": sites,
                "links": dict(zip(self.LINK_TALLY, tally.cpu().tolist())), "forest": forest}

    def unitigs(self, count_range=None, adjacency=False, where=False, sequences=True, links=False, components=False):
        """cp_kmer_sorted_unitigs ("Unitigs of sorted k-mers" in include/classpro_amd.h): the unitigs of the de Bruijn
        graph of the keys of this snapshot.  Returns a `Unitigs`: len() unitigs, `.seq` (uint8, upper-case A C G T), `.off`
        (int64 [len+1]), `.kc` (the exact sum of the counts of a unitig's nodes) and `.flag` (bit 0 = circular) as device
        tensors, `.tally` a dict, `.strings()`.  `count_range` is (lo, hi) as in `combine`: a key outside it counts as
        absent.  adjacency=True sets `.adj`, the adjacency byte of every entry (uint8); where=True sets `.utg` and `.at`,
        the unitig of every entry and 2 * (its place in it) + (1 when spelled reversed), -1 for an entry that is not in.
        sequences=False asks for no unitig object: with `where` the chains are still ranked and numbered (the tally is
        complete), without it only the adjacency pass runs and the tally's unitig fields are 0.  The object owns its
        memory and keeps no reference to the snapshot.
        links=True or components=True also calls cp_kmer_sorted_unitig_links ("Links between unitigs") with the same
        range and the where arrays of the first call, made internally: `.loff` (int64 [2*len+1]), `.link` (the target
        oriented unitig 2v+o of every arc) and `.base` (its base 0..3) as device tensors that view a second object,
        `.link_tally` a dict, `.links()` the arcs as a host list of (x, c, y); components=True adds `.comp`, the smallest
        unitig of every unitig's connected component, and fills the tally's components and largest_bases.  Both read the
        ends of the sequences: with sequences=False they raise ValueError."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        rng = None
        if count_range is not None:
            lo, hi = count_range
            rng = (C.c_int64 * 2)(1 if lo is None else int(lo), (1 << 63) - 1 if hi is None else int(hi))
        graph = links or components
        if graph and not sequences:
            raise ValueError("links and components are read off the ends of the sequences: sequences=False cannot have them")
        tally = (C.c_int64 * len(Unitigs.TALLY))()
        adj = torch.zeros(self.n, dtype=torch.uint8, device=self.device) if adjacency else None
        utg = torch.full((self.n,), -1, dtype=torch.int64, device=self.device) if where or graph else None
        at = torch.full((self.n,), -1, dtype=torch.int64, device=self.device) if where or graph else None
        ptr = lambda x: x.data_ptr() if x is not None and self.n else None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_unitigs(self.s, rng, tally, ptr(adj), ptr(utg), ptr(at), _stream_of(self.device),
                                                C.byref(h) if sequences else None))
        U = Unitigs(self.L, self.device, self.K, h if sequences else None, dict(zip(Unitigs.TALLY, tally)), adj,
                    utg if where else None, at if where else None)
        if graph:
            ltally, g = (C.c_int64 * len(Unitigs.LINK_TALLY))(), C.c_void_p()
            with torch.cuda.device(self.device):
                rc = self.L.cp_kmer_sorted_unitig_links(self.s, rng, h, ptr(utg), ptr(at), ltally, 1 if components else 0,
                                                        _stream_of(self.device), C.byref(g))
            if rc != 0:
                U.close()
            check(rc)
            U._adopt_graph(g, dict(zip(Unitigs.LINK_TALLY, ltally)), components)
        return U

    PRUNE_TALLY = ("unitigs", "islands", "tips", "bubbles", "removed_keys", "removed_bases", "kept_keys")

    def prune(self, U, islands=0, tips=0, bubbles=0, weight=None, table=True):
        """cp_kmer_sorted_unitig_prune ("Pruning the unitig graph" in include/classpro_amd.h): the islands, tips and simple
        bubbles of the unitig graph `U`, a `Unitigs` of THIS snapshot made with where=True, links=True.  `islands`, `tips`
        and `bubbles` are the limits in bases, 0 switching a rule off; `weight` an int64 device tensor [len(U)] that takes
        the place of `U.kc`.  Returns (table, why, tally): a new `SortedKmers` of the entries of the unitigs that stay (None
        with table=False), which keeps no reference to this one, the mark of every unitig as a uint8 device tensor (0 kept,
        1 island, 2 tip, 3 bubble) and a dict of PRUNE_TALLY."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if not isinstance(U, Unitigs) or U.u is None or U.g is None or U.utg is None:
            raise ValueError("prune needs a Unitigs made with where=True, links=True that is not closed")
        if U.K != self.K or U.utg.numel() != self.n:
            raise ValueError("the Unitigs are not of this snapshot")
        limits = (C.c_int64 * 3)(int(islands), int(tips), int(bubbles))
        if min(limits) < 0:
            raise ValueError("a limit must not be negative")
        if weight is not None:
            if weight.dtype != torch.int64 or weight.dim() != 1 or weight.numel() != len(U):
                raise ValueError("weight must be a flat int64 tensor with one value per unitig")
            weight = weight.to(self.device).contiguous()
        why = torch.zeros(len(U), dtype=torch.uint8, device=self.device)
        tally, h = (C.c_int64 * len(self.PRUNE_TALLY))(), C.c_void_p()
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_unitig_prune(self.s, U.u, U.utg.data_ptr() if self.n else None, U.g,
                                                     weight.data_ptr() if weight is not None and len(U) else None, limits,
                                                     why.data_ptr() if len(U) else None, tally, _stream_of(self.device),
                                                     C.byref(h) if table else None))
        out = None
        if table:
            out = SortedKmers.__new__(SortedKmers)
            out.L, out.device, out.K = self.L, self.device, self.K
            out._adopt(h)
        return out, why, dict(zip(self.PRUNE_TALLY, tally))

    def clean(self, count_range=None, islands=0, tips=0, bubbles=0, rounds=10):
        """The loop of tabclean: rounds of `unitigs` (where arrays), links (no components) and `prune`, the first with
        `count_range`, the later ones on the previous result with no range, until a round removes nothing or `rounds`
        rounds are done.  Returns (table, tallies): a new `SortedKmers` and the tally of every round; what it makes in
        between is closed."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        if int(rounds) < 1:
            raise ValueError("rounds must be positive")
        cur, tallies = self, []
        for r in range(int(rounds)):
            try:
                U = cur.unitigs(count_range if r == 0 else None, where=True, links=True)
                try:
                    nxt, _, t = cur.prune(U, islands, tips, bubbles)
                finally:
                    U.close()
            finally:
                if cur is not self:
                    cur.close()
            cur = nxt
            tallies.append(t)
            if t["removed_keys"] == 0:
                break
        return cur, tallies

    def hist(self):
        """cp_kmer_sorted_hist: the FASTK histogram of the snapshot's counts in the shape `KmerCounts.hist` returns,
        (1, 32767, ilowcnt, ihighcnt, int64[32767])."""
        if self.s is None:
            raise ValueError("SortedKmers is closed")
        h = np.zeros(32767, np.int64)
        il, ih = C.c_int64(), C.c_int64()
        with torch.cuda.device(self.device):
            check(self.L.cp_kmer_sorted_hist(self.s, h.ctypes.data, C.byref(il), C.byref(ih)))
        return 1, 32767, il.value, ih.value, h

    def close(self):
        if getattr(self, "s", None):
            self.L.cp_kmer_sorted_destroy(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Unitigs:
    """The result of `SortedKmers.unitigs` (a cp_unitigs and the per-entry tensors asked for).  The tensors `.seq`, `.off`,
    `.kc` and `.flag` VIEW the object's device memory and keep it alive; `close()` frees it at once, after which a tensor
    still held points at freed memory.  With links= or components= it also holds a cp_unitig_graph, which `.loff`, `.link`,
    `.base` and `.comp` view in the same way and `close()` frees with the first."""
    TALLY = ("keys", "unitigs", "bases", "circular", "longest", "isolated", "tips", "branching", "arcs", "rounds", "jump_ns")
    LINK_TALLY = ("links", "dead_ends", "tip_unitigs", "isolated_unitigs", "self", "components", "largest_bases", "rounds")

    def __init__(self, L, device, K, handle, tally, adj, utg, at):
        self.L, self.device, self.K, self.u, self.tally = L, device, K, handle, tally
        self.adj, self.utg, self.at = adj, utg, at
        self.n, self.bases, self._ptr = tally["unitigs"], tally["bases"], [None] * 4
        if handle is not None:
            self.n, self.bases = L.cp_unitigs_count(handle), L.cp_unitigs_bases(handle)
            p = [C.c_void_p() for _ in range(4)]
            check(L.cp_unitigs_arrays(handle, *[C.byref(x) for x in p]))
            self._ptr = [x.value for x in p]
        self.g, self.link_tally, self.nlinks, self._gptr, self._with_comp = None, None, 0, [None] * 4, False

    def _adopt_graph(self, handle, tally, with_comp):
        self.g, self.link_tally, self.nlinks, self._with_comp = handle, tally, self.L.cp_unitig_graph_links(handle), with_comp
        p = [C.c_void_p() for _ in range(4)]
        check(self.L.cp_unitig_graph_arrays(handle, *[C.byref(x) for x in p]))
        self._gptr = [x.value for x in p]

    def __len__(self):
        return self.n

    def _tensor(self, ptr, n, typestr, dtype, pad):
        if n == 0 or not ptr:
            return torch.zeros(pad, dtype=dtype, device=self.device)
        iface = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        holder = type("_UgView", (), {"__cuda_array_interface__": iface, "owner": self})()
        return torch.as_tensor(holder, device=self.device)

    def _view(self, which, n, typestr, dtype):
        if self.u is None:
            raise ValueError("Unitigs holds no sequences (sequences=False) or is closed")
        return self._tensor(self._ptr[which], n, typestr, dtype, n if which == 1 else 0)

    def _gview(self, which, n, typestr, dtype):
        if self.g is None or (which == 3 and not self._with_comp):
            raise ValueError("Unitigs holds no links or no components (links=, components=) or is closed")
        return self._tensor(self._gptr[which], n, typestr, dtype, n if which == 0 else 0)

    seq = property(lambda self: self._view(0, self.bases, "|u1", torch.uint8))
    off = property(lambda self: self._view(1, self.n + 1, "<i8", torch.int64))
    kc = property(lambda self: self._view(2, self.n, "<i8", torch.int64))
    flag = property(lambda self: self._view(3, self.n, "|u1", torch.uint8))
    loff = property(lambda self: self._gview(0, 2 * self.n + 1, "<i8", torch.int64))
    link = property(lambda self: self._gview(1, self.nlinks, "<i8", torch.int64))
    base = property(lambda self: self._gview(2, self.nlinks, "|u1", torch.uint8))
    comp = property(lambda self: self._gview(3, self.n, "<i8", torch.int64))

    def links(self):
        """The arcs as a list of (x, c, y) in order: the oriented unitig x = 2u+o reaches y by the base c (everything comes
        to the host)."""
        loff, link, base = self.loff.cpu().tolist(), self.link.cpu().tolist(), self.base.cpu().tolist()
        return [(x, base[k], link[k]) for x in range(2 * self.n) for k in range(loff[x], loff[x + 1])]

    def strings(self):
        """The sequences as a list of `str`, in order (everything comes to the host)."""
        text, off = bytes(self.seq.cpu().numpy()).decode(), self.off.cpu().tolist()
        return [text[off[u]:off[u + 1]] for u in range(self.n)]

    def close(self):
        if getattr(self, "u", None):
            self.L.cp_unitigs_destroy(self.u)
            self.u = None
        if getattr(self, "g", None):
            self.L.cp_unitig_graph_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def unitig_n50(lengths):
    """cp_unitig_n50: the largest L such that the unitigs of at least L bases hold at least half of all bases (0 for
    none); `lengths` is any sequence or tensor of non-negative integers."""
    v = lengths.cpu().numpy() if isinstance(lengths, torch.Tensor) else lengths
    v = np.ascontiguousarray(v, np.int64).reshape(-1)
    return check(lib().cp_unitig_n50(v.ctypes.data if len(v) else None, len(v)))


def path_walks(seg_off, segs, nodes, K):
    """The walks of the segments that `SortedKmers.read_paths` returned, on the host: a maximal chain of a read's segments in
    which every one but the first is joined.  `nodes` holds the number of nodes of every unitig (`U.off[1:] - U.off[:-1]
    - (K-1)`); tensors, arrays and lists are taken alike.  Returns a list of (read, first, end, path, path_length, q) in
    read order -- the GAF fields: the bases [first, end) of the read run along `path` (">u" / "<u" per segment) from base
    q of the path on, path_length being the bases of its unitigs less K-1 per join."""
    host = lambda v: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).tolist()
    off, nodes, K = host(seg_off), host(nodes), int(K)
    cols = [host(segs[k]) for k in ("first", "n", "x", "q", "read", "flags")]
    out = []
    for r in range(len(off) - 1):
        for i in range(off[r], off[r + 1]):
            first, n, x, q, read, flags = (c[i] for c in cols)
            if read != r:
                raise ValueError("segment %d is of read %d, not of read %d" % (i, read, r))
            step = ("<" if x & 1 else ">") + str(x >> 1)
            if (flags & 1) and i > off[r]:
                w = out[-1]
                w[2], w[3], w[4] = first + n + K - 1, w[3] + step, w[4] + nodes[x >> 1]
            else:
                out.append([r, first, first + n + K - 1, step, nodes[x >> 1] + K - 1, q])
    return [tuple(w) for w in out]


def bin_calls(hits, only_a, only_b, min_markers=1, normalise=True):
    """cp_bin_call for every row of `hits` (the tensor of `SortedKmers.read_hits`, or any int64 [n, 5] array): a `bytes` of
    'A', 'B' or 'U' per read.  `only_a` and `only_b` are the sizes of the two marker sets, `A.compare(B)[:2]` with the
    ranges of the hits; they weigh the counts when `normalise` is set.  A read with nA + nB < min_markers is 'U'."""
    h = hits.cpu().numpy() if isinstance(hits, torch.Tensor) else hits
    h = np.ascontiguousarray(h, np.int64).reshape(-1, 5)
    L = lib()
    out = bytearray(len(h))
    for i in range(len(h)):
        out[i] = check(L.cp_bin_call(h[i].ctypes.data, int(only_a), int(only_b), int(min_markers), 1 if normalise else 0))
    return bytes(out)


RUN_DTYPE = np.dtype([("first", np.int64), ("last", np.int64), ("n", np.int64), ("read", np.int32), ("state", np.int32)])


def run_blocks(runs, min_n=1):
    """cp_run_blocks: the runs of ONE read, every state that is not skipped emitted, as a list of (first, last, n, read,
    state) tuples or the dict of `SortedKmers.read_runs` cut to that read.  Runs with n < min_n are dropped, neighbours of
    equal state among the rest are merged.  Returns (blocks, dropped): a list of such tuples and the number of dropped
    runs."""
    if isinstance(runs, dict):
        cols = [runs[k].cpu().numpy() if isinstance(runs[k], torch.Tensor) else np.asarray(runs[k]) for k in RUN_DTYPE.names]
        runs = list(zip(*[c.tolist() for c in cols]))
    arr = np.array([tuple(int(x) for x in r) for r in runs], RUN_DTYPE).reshape(-1)
    out = np.zeros(max(len(arr), 1), RUN_DTYPE)
    dropped = C.c_int64()
    nb = check(lib().cp_run_blocks(arr.ctypes.data if len(arr) else out.ctypes.data, len(arr), int(min_n), out.ctypes.data,
                                   C.byref(dropped)))
    return [tuple(int(x) for x in b) for b in out[:nb].tolist()], dropped.value


PHASE_TALLY = ("edges", "kept", "tied", "weak", "forest", "conflicts", "blocks", "single", "largest", "rounds", "bad")


def phase_forest(edges, nsites, min_support=2):
    """cp_phase_forest ("Phasing heterozygous sites from reads" in include/classpro_amd.h): `edges` is the `SortedKmers` of a
    `KmerCounts` of K = 32 that holds the link keys (`KmerCounts.add_keys`, `sorted(1)`).  Returns (block, side, tally):
    block an int64 and side a uint8 device tensor [nsites], tally a dict of PHASE_TALLY."""
    if edges.s is None:
        raise ValueError("SortedKmers is closed")
    nsites = int(nsites)
    room = nsites if 0 < nsites < 1 << 31 else 0           # anything else is the library's to refuse
    block = torch.empty(room, dtype=torch.int64, device=edges.device)
    side = torch.empty(room, dtype=torch.uint8, device=edges.device)
    tally = (C.c_int64 * len(PHASE_TALLY))()
    with torch.cuda.device(edges.device):
        check(edges.L.cp_phase_forest(edges.s, nsites, int(min_support), block.data_ptr() if room else None,
                                      side.data_ptr() if room else None, tally, _stream_of(edges.device)))
    return block, side, dict(zip(PHASE_TALLY, tally))


def kmer_qv(K, a_only, a_total):
    """cp_kmer_qv: (qv, err) by Merqury's rule from the "a"-weighted `compare_hist` of an assembly against its reads:
    `a_only` the sum of column 0, `a_total` the sum of the whole matrix.  qv is inf when a_only is 0."""
    qv, err = C.c_double(), C.c_double()
    check(lib().cp_kmer_qv(int(K), int(a_only), int(a_total), C.byref(qv), C.byref(err)))
    return qv.value, err.value


def ktab_tile():
    """cp_ktab_tile: the entries one block sorts on chip (a build constant; tests place sizes around it)."""
    return lib().cp_ktab_tile()


def _stream_of(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def threshold_labels(batch, thresholds, K, packed=False, counts=None):
    """cp_threshold_labels (the per-read loop of ClassGS.c:228-248): a count c is E if c < thresholds[0], else H if
    c < thresholds[1], else D if c < thresholds[2], else R; every read gets min(K-1, rlen) 'N' first.  `batch` is a
    `Batch` or a tuple of device tensors (prof int16/uint16 payload, prof_off int64 [n+1], seq_off int64 [n+1]); reads
    shorter than K are allowed.  Returns (labels, counts): labels a uint8 device tensor of seq_off[n] characters -- or,
    with packed=True, the 2-bit bytes of cp_pack_labels and their int64 offsets as (packed, pack_off) -- and counts an
    int64 device tensor [4], order E, H, D, R.  Pass a previous `counts` tensor to go on adding to it.  Nothing is
    copied to the host."""
    if isinstance(batch, Batch):
        prof, prof_off, seq_off = batch.prof, batch.prof_off, batch.seq_off
    else:
        prof, prof_off, seq_off = batch
    dev = seq_off.device
    if dev.type != "cuda":
        raise ValueError("classpro_amd runs on a HIP device only")
    n = seq_off.numel() - 1
    if isinstance(batch, Batch):                           # the host knows the size: no read-back, nothing waits for the stream
        total = batch.total_bases
    else:
        total = int(seq_off[-1].item()) if n > 0 else 0
    t = (C.c_int32 * 3)(*[int(x) for x in thresholds])
    if counts is None:
        counts = torch.zeros(4, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        if packed:
            clen = (seq_off[1:] - seq_off[:-1] + 3) >> 2
            pack_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            torch.cumsum(clen, 0, out=pack_off[1:])
            out = torch.empty(max(int(pack_off[-1].item()) if n > 0 else 0, 1), dtype=torch.uint8, device=dev)
            check(lib().cp_threshold_labels(K, t, prof.data_ptr(), prof_off.data_ptr(), seq_off.data_ptr(), n, total, None,
                                            out.data_ptr(), pack_off.data_ptr(), counts.data_ptr(), _stream_of(dev)))
            return (out, pack_off), counts
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        check(lib().cp_threshold_labels(K, t, prof.data_ptr(), prof_off.data_ptr(), seq_off.data_ptr(), n, total,
                                        out.data_ptr(), None, None, counts.data_ptr(), _stream_of(dev)))
    return out, counts


class LabelAccuracy:
    """class2acc's counting (class2acc.c:141-316, default report) for label strings in HBM (cp_acc_*; semantics in
    include/classpro_amd.h): an accumulator over batches.  max_e_pct / rep_pct are class2acc's -f / -r."""

    STATES = "ERHD"                                        # order of the confusion matrix's rows and columns

    def __init__(self, K, max_e_pct=100, rep_pct=0, device="cuda:0"):
        from ._lib import AccStats
        self.L = lib()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("classpro_amd runs on a HIP device only")
        torch.cuda.set_device(self.device)
        self.K = K
        self._Stats = AccStats
        a = C.c_void_p()
        check(self.L.cp_acc_create(K, float(max_e_pct), float(rep_pct), C.byref(a)))
        self.a = a

    def close(self):
        if getattr(self, "a", None):
            self.L.cp_acc_destroy(self.a)
            self.a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, est, truth, seq_off=None):
        """Adds a batch: `est` / `truth` uint8 device tensors in the label layout and `seq_off` int64 [n+1]; or
        add(batch, truth) for a `Batch` labelled by Classifier.classify / run (its `labels` tensor is the estimate)."""
        total = None
        if isinstance(est, Batch):                         # the host knows the size: no read-back, nothing waits for the stream
            est, seq_off, total = est.labels, est.seq_off, est.total_bases
        n = seq_off.numel() - 1
        if total is None:
            total = int(seq_off[-1].item()) if n > 0 else 0
        if est.numel() < total or truth.numel() < total:
            raise ValueError("LabelAccuracy.add: a label tensor is shorter than seq_off[-1]")
        check(self.L.cp_acc_add(self.a, est.data_ptr(), truth.data_ptr(), seq_off.data_ptr(), n, total,
                                _stream_of(self.device)))

    def stats(self):
        """dict: cfm (4x4 list, truth row, estimate column, order E R H D), ntot/ncor/nfne (all, _normal, _repeat),
        n_reads, n_reads_filtered, n_invalid, accuracy and fn_error in percent (nan without counted k-mers).
        Raises ClassProError (CP_EINVAL) when a label position held a character other than E/H/D/R."""
        s = self._Stats()
        check(self.L.cp_acc_read(self.a, C.byref(s)))
        d = {f: getattr(s, f) for f, _ in s._fields_ if f != "cfm"}
        d["cfm"] = [list(row) for row in s.cfm]
        d["accuracy"] = 100.0 * s.ncor / s.ntot if s.ntot else float("nan")
        d["fn_error"] = 100.0 * s.nfne / s.ntot if s.ntot else float("nan")
        return d

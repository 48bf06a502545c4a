"""ClassGS on a real MI355X (`-m gpu`): cp_threshold_labels and the label-accuracy accumulator against numpy restatements
of src/ClassGS.c:228-248 and src/class2acc.c:141-316, on small_ds, on adversarial batches and on a batch above 2^31
bases (there against the same rules written in torch on the device); the command against the outputs of the
reference's own ClassGS (tests/golden/classgs.json) and, for -A, against our class2acc.  Everything here is integers
and bytes: zero tolerance."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import classgs_case as cc
from conftest import ROOT

pytestmark = pytest.mark.gpu
TOOLS = os.path.join(ROOT, "classpro_amd")
GUARD = 64
STATE = {ord("E"): 0, ord("R"): 1, ord("H"): 2, ord("D"): 3}                 # class2acc's stoc order


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


# ---- numpy restatements ---------------------------------------------------------------------------------------
def np_labels(profs, rlens, thres, K):
    """ClassGS.c:228-248 per read: min(K-1, rlen) 'N', then the chain over the counts."""
    return [np.concatenate([np.full(min(K - 1, n), ord("N"), np.uint8), cc.chain_labels(p, thres)]) for p, n in zip(profs, rlens)]


def np_pack(labels):
    """ctos (N, E -> 0, R -> 1, H -> 2, D -> 3) + Compress_Read per read, concatenated."""
    from classpro_amd.dazz import pack_2bit
    code = np.zeros(256, np.uint8)
    code[ord("R")], code[ord("H")], code[ord("D")] = 1, 2, 3
    return np.concatenate([pack_2bit(code[l]) for l in labels] + [np.zeros(0, np.uint8)])


def np_accuracy(est, truth, K, max_e_pct=100, rep_pct=0):
    """class2acc.c:141-316 (default report) for lists of per-read label arrays."""
    s = dict(cfm=[[0] * 4 for _ in range(4)], ntot=0, ncor=0, nfne=0, ntot_normal=0, ncor_normal=0, nfne_normal=0,
             ntot_repeat=0, ncor_repeat=0, nfne_repeat=0, n_reads=len(est), n_reads_filtered=0, n_invalid=0)
    lut = np.full(256, -1, np.int64)
    for ch, v in STATE.items():
        lut[ch] = v
    for e, t in zip(est, truth):
        rtot = len(e) - (K - 1)
        if rtot <= 0:
            continue
        ei, ti = lut[e[K - 1:]], lut[t[K - 1:]]
        assert ei.min() >= 0 and ti.min() >= 0
        cell = np.bincount(4 * ti + ei, minlength=16)
        for i in range(4):
            for j in range(4):
                s["cfm"][i][j] += int(cell[4 * i + j])
        rcor, rfne = int((ei == ti).sum()), int(((ti == 0) & (ei != 0)).sum())
        rcomp_e, rcomp_r = int((ti == 0).sum()), int((ti == 1).sum())
        if float(rcomp_e) / float(rtot) * 100 > max_e_pct:
            s["n_reads_filtered"] += 1
            continue
        kind = "repeat" if float(rcomp_r) / float(rtot) * 100 > rep_pct else "normal"
        for k, v in (("ntot", rtot), ("ncor", rcor), ("nfne", rfne)):
            s[k] += v
            s[k + "_" + kind] += v
    return s


def flat(torch, arrays, dtype, pad=8):
    """Concatenation on the device (+ the int64 offsets), padded so that the tensor never is empty."""
    off = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(a) for a in arrays], out=off[1:])
    h = np.concatenate([np.asarray(a, dtype) for a in arrays] + [np.zeros(pad, dtype)])
    if dtype == np.uint16:
        h = h.view(np.int16)
    return torch.from_numpy(h).cuda(), torch.from_numpy(off).cuda(), off


def run_threshold(torch, profs, rlens, thres, K):
    """cp_threshold_labels with all three outputs into guarded buffers, then each output alone; returns host arrays."""
    from classpro_amd._lib import lib, check
    L = lib()
    prof, prof_off, _ = flat(torch, profs, np.uint16)
    so = np.zeros(len(rlens) + 1, np.int64)
    np.cumsum(rlens, out=so[1:])
    pko = np.zeros(len(rlens) + 1, np.int64)
    np.cumsum([(n + 3) // 4 for n in rlens], out=pko[1:])
    seq_off, pack_off = torch.from_numpy(so).cuda(), torch.from_numpy(pko).cuda()
    total, ptotal = int(so[-1]), int(pko[-1])
    t = (C.c_int32 * 3)(*thres)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for want_lab, want_pack, want_cnt in [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)]:
        lab = torch.full((total + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        pk = torch.full((ptotal + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        cnt = torch.tensor([1000, 2000, 3000, 4000], dtype=torch.int64, device="cuda")       # "added to"
        check(L.cp_threshold_labels(K, t, prof.data_ptr(), prof_off.data_ptr(), seq_off.data_ptr(), len(rlens), total,
                                    lab.data_ptr() + GUARD if want_lab else None, pk.data_ptr() + GUARD if want_pack else None,
                                    pack_off.data_ptr() if want_pack else None, cnt.data_ptr() if want_cnt else None, st))
        torch.cuda.synchronize()
        lab, pk, cnt = lab.cpu().numpy(), pk.cpu().numpy(), cnt.cpu().numpy() - np.array([1000, 2000, 3000, 4000])
        for buf, n, want in ((lab, total, want_lab), (pk, ptotal, want_pack)):
            assert (buf[:GUARD] == 0xAA).all() and (buf[GUARD + n:] == 0xAA).all(), "a write outside the output"
            assert want or (buf == 0xAA).all(), "an output that was not asked for was written"
        assert want_cnt or not cnt.any()
        outs.append((lab[GUARD:GUARD + total] if want_lab else None, pk[GUARD:GUARD + ptotal] if want_pack else None,
                     cnt if want_cnt else None))
    # cp_pack_labels of the character output (the layout the packed output must have)
    d_lab = torch.from_numpy(np.concatenate([outs[0][0], np.zeros(8, np.uint8)])).cuda()
    d_pk = torch.zeros(ptotal + 8, dtype=torch.uint8, device="cuda")
    check(L.cp_pack_labels(d_lab.data_ptr(), seq_off.data_ptr(), pack_off.data_ptr(), len(rlens), d_pk.data_ptr(), st))
    torch.cuda.synchronize()
    return outs, d_pk.cpu().numpy()[:ptotal]


def check_threshold(torch, profs, rlens, thres, K):
    want = np_labels(profs, rlens, thres, K)
    wl = np.concatenate(want + [np.zeros(0, np.uint8)])
    wp = np_pack(want)
    wc = np.array([int((wl == ord(ch)).sum()) for ch in "EHDR"])
    outs, repacked = run_threshold(torch, profs, rlens, thres, K)
    assert np.array_equal(repacked, wp)
    for lab, pk, cnt in outs:
        assert lab is None or np.array_equal(lab, wl), thres
        assert pk is None or np.array_equal(pk, wp), thres
        assert cnt is None or np.array_equal(cnt, wc), (thres, cnt, wc)
    return wc


ADVERSARIAL_THRESHOLDS = [(8, 25, 60), (30, 10, 50), (60, 25, 8), (20, 20, 20), (0, 0, 0), (-5, -1, 7), (-2 ** 31, 0, 2 ** 31 - 1),
                          (8, 70000, 2 ** 31 - 1), (65535, 65536, 65537), (1, 32767, 65535), (32768, 65535, 65536),
                          (70000, 80000, 90000)]


def adversarial_batch(K, seed):
    rng = np.random.default_rng(seed)
    rlens = [0, 1, K - 2, K - 1, K, K + 1, 200000] + [K + 15 + m for m in range(16)] + [2 * K + 100 + m for m in range(16)]
    rlens += [int(x) for x in rng.integers(1, 3000, 60)]
    rlens = [max(n, 0) for n in rlens]
    rng.shuffle(rlens)
    profs = []
    for n in rlens:
        m = max(n - (K - 1), 0)
        p = np.repeat(rng.integers(0, 90, m // 3 + 1), 3)[:m].astype(np.uint16)
        if m:
            idx = rng.integers(0, m, max(m // 20, 3))
            p[idx] = rng.choice([0, 1, 32767, 32768, 65535, 65534, 7, 8, 24, 25, 59, 60], len(idx))
        profs.append(p)
    return profs, [int(n) for n in rlens]


# ---- cp_threshold_labels ---------------------------------------------------------------------------------------
def test_threshold_labels_small_ds(torch_dev, small_ds):
    from classpro_amd.api import Batch, threshold_labels
    K = small_ds["K"] if "K" in small_ds else 40
    profs, rlens = list(small_ds["profiles"]), [len(s) for s in small_ds["seqs"]]
    for thres in [(8, 25, 60), (30, 10, 50)]:
        wc = check_threshold(torch_dev, profs, rlens, thres, K)
        assert (wc > 0).sum() >= 3
    # the Python mirror on a Batch: labels, packed bytes, counts; a second call goes on adding
    b = Batch.from_reads(small_ds["seqs"], small_ds["profiles"])
    want = np_labels(profs, rlens, (8, 25, 60), K)
    wl = np.concatenate(want)
    lab, cnt = threshold_labels(b, (8, 25, 60), K)
    assert np.array_equal(lab[:b.total_bases].cpu().numpy(), wl)
    wc = np.array([int((wl == ord(ch)).sum()) for ch in "EHDR"])
    assert np.array_equal(cnt.cpu().numpy(), wc) and np.array_equal(wc, np.bincount(np.searchsorted(np.frombuffer(b"DEHR", np.uint8), wl[wl != ord("N")]), minlength=4)[[1, 2, 0, 3]])
    (pk, pko), cnt2 = threshold_labels((b.prof, b.prof_off, b.seq_off), (8, 25, 60), K, packed=True, counts=cnt)
    assert np.array_equal(pk[:int(pko[-1])].cpu().numpy(), np_pack(want))
    assert cnt2 is cnt and np.array_equal(cnt.cpu().numpy(), 2 * wc)


@pytest.mark.parametrize("K", [40, 41, 42, 43, 5, 2])
def test_threshold_labels_adversarial(torch_dev, K):
    """Unsorted, equal, negative and > 65535 thresholds; counts 0, 32767, 65535; reads of length 0, 1, K-2, K-1, K, K+1,
    every remainder mod 16, 200 000; K with every value of (K-1) % 4."""
    profs, rlens = adversarial_batch(K, 100 + K)
    assert {n % 16 for n in rlens} == set(range(16)) and max(rlens) == 200000
    for thres in ADVERSARIAL_THRESHOLDS:
        check_threshold(torch_dev, profs, rlens, thres, K)


def test_threshold_labels_bad_arguments(torch_dev):
    from classpro_amd._lib import lib, ClassProError, check
    t = (C.c_int32 * 3)(1, 2, 3)
    x = torch_dev.zeros(16, dtype=torch_dev.int64, device="cuda")
    with pytest.raises(ClassProError) as e:
        check(lib().cp_threshold_labels(40, t, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, None, None, None, None, None))
    assert e.value.code == -1
    with pytest.raises(ClassProError):                     # packed output without its offsets
        check(lib().cp_threshold_labels(40, t, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, None, x.data_ptr(), None, None, None))


# ---- label accuracy --------------------------------------------------------------------------------------------
def acc_stats(torch, est, truth, K, max_e_pct, rep_pct, order=None, splits=1):
    from classpro_amd.api import LabelAccuracy
    A = LabelAccuracy(K, max_e_pct, rep_pct)
    idx = list(range(len(est))) if order is None else list(order)
    per = (len(idx) + splits - 1) // splits
    for a in range(0, len(idx), per):
        part = idx[a:a + per]
        e, so, _ = flat(torch, [est[i] for i in part], np.uint8, pad=16)
        t, _, _ = flat(torch, [truth[i] for i in part], np.uint8, pad=16)
        A.add(e, t, so)
    s = A.stats()
    A.close()
    return s


def compare_stats(got, want):
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)


@pytest.mark.parametrize("settings", [(100, 0), (50, 5), (12.5, 0.75), (0, 100)], ids=str)
def test_label_accuracy_small_ds(torch_dev, small_ds, settings):
    K = 40
    profs, rlens = list(small_ds["profiles"]), [len(s) for s in small_ds["seqs"]]
    est = np_labels(profs, rlens, (8, 25, 60), K)
    truth = np_labels(list(small_ds["rel_profiles"]), rlens, (1, 2, 3), K)       # prof2class: 0 E, 1 H, 2 D, >= 3 R
    want = np_accuracy(est, truth, K, *settings)
    assert want["ntot"] > 0 or settings == (0, 100)
    one = acc_stats(torch_dev, est, truth, K, *settings)
    compare_stats(one, want)
    rng = np.random.default_rng(3)
    three = acc_stats(torch_dev, est, truth, K, *settings, order=rng.permutation(len(est)), splits=3)
    compare_stats(three, want)
    assert repr(three) == repr(one)                          # (the percentages are nan when nothing is counted)


@pytest.mark.parametrize("K", [40, 42, 5])
def test_label_accuracy_adversarial(torch_dev, K):
    profs, rlens = adversarial_batch(K, 300 + K)
    rng = np.random.default_rng(K)
    est = np_labels(profs, rlens, (8, 25, 60), K)
    truth = np_labels([np.where(rng.random(len(p)) < 0.2, rng.integers(0, 90, len(p)), p) for p in profs], rlens, (10, 25, 50), K)
    for settings in [(100, 0), (30, 20), (7.5, 33.3)]:
        want = np_accuracy(est, truth, K, *settings)
        compare_stats(acc_stats(torch_dev, est, truth, K, *settings), want)
        compare_stats(acc_stats(torch_dev, est, truth, K, *settings, order=rng.permutation(len(est)), splits=3), want)
    assert want["n_reads_filtered"] > 0 and want["ntot_repeat"] > 0 and want["ntot_normal"] > 0
    assert all(v > 0 for row in want["cfm"] for v in row)         # every cell of the confusion matrix is exercised


def test_label_accuracy_invalid_character(torch_dev, small_ds):
    from classpro_amd.api import LabelAccuracy
    from classpro_amd._lib import ClassProError
    K = 40
    profs, rlens = list(small_ds["profiles"])[:20], [len(s) for s in small_ds["seqs"]][:20]
    est = np_labels(profs, rlens, (8, 25, 60), K)
    truth = [x.copy() for x in est]
    truth[3][K - 2] = ord("X")                               # inside the prefix: not looked at
    A = LabelAccuracy(K)
    e, so, _ = flat(torch_dev, est, np.uint8, pad=16)
    t, _, _ = flat(torch_dev, truth, np.uint8, pad=16)
    A.add(e, t, so)
    s = A.stats()
    assert s["n_invalid"] == 0 and s["ncor"] == s["ntot"] == sum(rlens) - 20 * (K - 1)
    truth[3][K - 1] = ord("N")
    truth[7][len(truth[7]) - 1] = ord("e")
    est[9][len(est[9]) // 2] = 0
    e, _, _ = flat(torch_dev, est, np.uint8, pad=16)
    t, _, _ = flat(torch_dev, truth, np.uint8, pad=16)
    A.add(e, t, so)
    with pytest.raises(ClassProError) as err:
        A.stats()
    assert err.value.code == -1 and "3 label positions" in str(err.value)
    A.close()


# ---- a batch above 2^31 bases ------------------------------------------------------------------------------------
def test_batch_above_2_31_bases(torch_dev):
    """56 Mbp x 40: 2.24 Gbases in ONE call of each kernel, against the same rules written in torch on the device."""
    torch = torch_dev
    from classpro_amd.api import Batch, LabelAccuracy, threshold_labels
    from classpro_amd.synth_dev import DeviceSynth
    from classpro_amd._lib import lib, check
    K = 40
    ds = DeviceSynth(genome_len=56_000_000, cov=40, read_len=20000, K=K, seed=4)
    rd = ds.reads(0, ds.n_reads, truth=True)
    ds.check()
    b = Batch.from_device(rd)
    assert b.total_bases > 2 ** 31
    del ds
    t_est, t_tru = (8, 25, 60), (1, 2, 3)
    lab, cnt = threshold_labels(b, t_est, K)
    (pk, pko), cnt_p = threshold_labels(b, t_est, K, packed=True)
    # the chain in torch, in chunks of k-mer space; k-mer i of read r sits at label position i + (r+1)(K-1)
    nk = b.total_kmers
    E, H, D, R = (ord(c) for c in "EHDR")

    def chain(c, t):
        c = c.to(torch.int32) & 0xFFFF
        out = torch.full_like(c, R, dtype=torch.uint8)
        out[c < t[2]] = D
        out[c < t[1]] = H
        out[c < t[0]] = E
        return out
    want = torch.empty(nk, dtype=torch.uint8, device="cuda")
    got = torch.empty(nk, dtype=torch.uint8, device="cuda")
    truth = torch.full((b.total_bases,), ord("N"), dtype=torch.uint8, device="cuda")
    step = 1 << 27
    for a in range(0, nk, step):
        e = min(a + step, nk)
        k = torch.arange(a, e, device="cuda")
        r = torch.searchsorted(b.prof_off, k, right=True) - 1
        pos = k + (r + 1) * (K - 1)
        want[a:e] = chain(b.prof[a:e], t_est)
        got[a:e] = lab[pos]
        truth[pos] = chain(rd["truth"][a:e], t_tru)
        del k, r, pos
    assert torch.equal(got, want)
    assert int((lab[:b.total_bases] == ord("N")).sum().item()) == b.nreads * (K - 1)
    pre = (b.seq_off[:-1, None] + torch.arange(K - 1, device="cuda")[None, :]).reshape(-1)
    assert bool((lab[pre] == ord("N")).all())
    wc = [int((want == ch).sum().item()) for ch in (E, H, D, R)]
    assert cnt.tolist() == wc and cnt_p.tolist() == wc and sum(wc) == nk
    # the packed output against cp_pack_labels of the character output
    pk2 = torch.zeros_like(pk)
    check(lib().cp_pack_labels(lab.data_ptr(), b.seq_off.data_ptr(), pko.data_ptr(), b.nreads, pk2.data_ptr(),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(pk, pk2)
    del pk, pk2, got
    # label accuracy: per-read sums from prefix sums over k-mer space, the decisions in float64 as class2acc writes them
    tk = torch.empty(nk, dtype=torch.uint8, device="cuda")
    for a in range(0, nk, step):
        e = min(a + step, nk)
        tk[a:e] = chain(rd["truth"][a:e], t_tru)

    def per_read(x):
        c = torch.zeros(nk + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(x, 0, dtype=torch.int64, out=c[1:])
        return c[b.prof_off[1:]] - c[b.prof_off[:-1]]
    rtot = b.prof_off[1:] - b.prof_off[:-1]
    rcor, rfne = per_read(want == tk), per_read((tk == E) & (want != E))
    rce, rcr = per_read(tk == E), per_read(tk == R)
    # -f / -r in the middle of this set's own per-read rates, so that all three kinds of read occur
    max_e = float((rce.double() / rtot.double() * 100).median().item())
    rep = float((rcr.double() / rtot.double() * 100).quantile(0.75).item()) if b.nreads < 10 ** 6 else 0.0
    A = LabelAccuracy(K, max_e, rep)
    A.add(lab, truth, b.seq_off)
    s = A.stats()
    A.close()
    filt = rce.double() / rtot.double() * 100 > max_e
    isrep = (rcr.double() / rtot.double() * 100 > rep) & ~filt
    norm = ~filt & ~isrep
    code = {E: 0, R: 1, H: 2, D: 3}
    for tc, i in code.items():
        for ec, j in code.items():
            assert s["cfm"][i][j] == int(((tk == tc) & (want == ec)).sum().item()), (i, j)
    keep = ~filt
    assert s["n_reads"] == b.nreads and s["n_reads_filtered"] == int(filt.sum().item()) and s["n_invalid"] == 0
    assert 0 < s["n_reads_filtered"] < b.nreads and int(isrep.sum().item()) > 0 and int(norm.sum().item()) > 0
    for name, m in (("", keep), ("_normal", norm), ("_repeat", isrep)):
        assert s["ntot" + name] == int(rtot[m].sum().item())
        assert s["ncor" + name] == int(rcor[m].sum().item())
        assert s["nfne" + name] == int(rfne[m].sum().item())


# ---- the command -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "classgs.json")))


def run_tool(args, timeout=300):
    """One process at a time, each under its own time limit."""
    return subprocess.run(args, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("tiny", [True, False], ids=["tiny", "notiny"])
@pytest.mark.parametrize("kind", cc.KINDS)
def test_command_matches_reference(torch_dev, golden, kind, tiny, tmp_path):
    d = str(tmp_path)
    cc.build_scenario(d, kind, tiny)
    assert cc.input_sha(d) == golden["scenarios"][cc.scenario_id(kind, tiny)]["input_sha256"]
    for thres in cc.THRESHOLDS:
        g = golden["cases"][cc.case_id(kind, tiny, thres)]
        r = run_tool([os.path.join(TOOLS, "ClassGS"), os.path.join(d, "reads")] + list(thres))
        assert r.returncode == g["returncode"] == 0, r.stderr
        assert r.stderr.replace(d, "{dir}") == g["stderr"] and r.stdout == ""
        data = open(os.path.join(d, "reads.GS.class"), "rb").read()
        assert len(data) == g["size"] and hashlib.sha256(data).hexdigest() == g["sha256"], thres
        assert sum(1 for ch in "EHDR" if g["counts"][ch] > 0) >= 3 or thres == ("0", "0", "0")
        os.remove(os.path.join(d, "reads.GS.class"))


@pytest.mark.parametrize("kind,tiny", [("fasta", True), ("fasta.gz", False), ("db", True), ("dam", False)])
def test_command_accuracy_matches_class2acc(torch_dev, kind, tiny, tmp_path):
    """-A prints what our class2acc (pinned to the reference's binary by tests/test_eval_tools.py) prints for the two
    files, and the .GS.class is the one written without -A."""
    d = str(tmp_path)
    cc.build_scenario(d, kind, tiny)
    subprocess.check_call([os.path.join(TOOLS, "prof2class"), os.path.join(d, "truth.prof"), os.path.join(d, "reads")])
    truth = os.path.join(d, "truth.class")
    for thres in [("8", "25", "60"), ("30", "10", "50")]:
        r0 = run_tool([os.path.join(TOOLS, "ClassGS"), os.path.join(d, "reads")] + list(thres))
        assert r0.returncode == 0, r0.stderr
        plain = open(os.path.join(d, "reads.GS.class"), "rb").read()
        r = run_tool([os.path.join(TOOLS, "ClassGS"), "-A" + truth, os.path.join(d, "reads")] + list(thres))
        assert r.returncode == 0, r.stderr
        assert r.stderr == r0.stderr and open(os.path.join(d, "reads.GS.class"), "rb").read() == plain
        q = run_tool([os.path.join(TOOLS, "class2acc"), os.path.join(d, "reads.GS.class"), truth])
        assert q.returncode == 0 and r.stdout == q.stdout and "Confusion Matrix" in r.stdout
    # a truth file of another read set: class2acc's message
    recs = open(truth).read().split("\n")
    recs[0] = "@other x"
    open(os.path.join(d, "renamed.class"), "w").write("\n".join(recs))
    r = run_tool([os.path.join(TOOLS, "ClassGS"), "-A" + os.path.join(d, "renamed.class"), os.path.join(d, "reads"), "8", "25", "60"])
    assert r.returncode == 1 and "Read 1 inconsistent names: " in r.stderr and "vs other (truth)" in r.stderr


def test_command_refuses_a_bad_profile(torch_dev, tmp_path):
    """A code string that does not expand to rlen-(K-1) counts: ClassPro's message (the reference does not check)."""
    from classpro_amd import fastk
    d = str(tmp_path)
    rng = np.random.default_rng(1)
    seqs = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]) for n in (500, 700)]
    with open(os.path.join(d, "reads.fa"), "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">r%d\n" % i + s + b"\n")
    profs = [rng.integers(1, 50, 500 - 39).astype(np.uint16), rng.integers(1, 50, 700 - 39 - 5).astype(np.uint16)]
    fastk.write_fastk(d, "reads", 40, profs, (1, 32767, 0, 0, np.zeros(32767, np.int64)), nparts=1)
    r = run_tool([os.path.join(TOOLS, "ClassGS"), os.path.join(d, "reads"), "8", "25", "60"])
    assert r.returncode == 1 and "Read 2: rlen (700) != plen+Km1 (695)" in r.stderr

"""ClassGS kernels (cp_threshold_labels, cp_acc_add) on BASELINE configs[2]: rates and the accuracy of both label sets.

    python scripts/classgs_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--launches 20] [--out FILE]

The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) with its ground truth, labelled
by the classifier (in sub-batches) and by cp_threshold_labels (the whole set in one call), and both label sets are
scored against the truth with LabelAccuracy.  Rates: device events around `--launches` launches after 3 warm-up
launches, on the whole set; bytes are computed from the shapes (thresholds: 2 B per k-mer in, 1 B per base or 0.25 B per
base out; accuracy: 2 B per base in).  cp_scan_candidates is timed in the same process on the same counts (2 B per
k-mer in, 1/8 B out): this project's own figure for a streaming read of the counts.

Thresholds.  A real run takes them from GenomeScope, which is not part of this project; for the synthetic set they are
derived from the set's own k-mer histogram by a fixed rule that stands in for it:
    E/H  the count with the fewest k-mers between 1 and the haploid peak (the first minimum of the histogram);
    H/D  the midpoint of the haploid and diploid peaks, (hcov + dcov + 1) // 2 (peaks from process_global_hist);
    D/R  the repeat threshold of the classifier, dcov + (int)(5 sqrt(dcov)) (N_SIGMA_RCOV of const.c, ClassPro.c:547).
Prints one JSON line; with --out also writes the report (profiles/classgs_configs2.txt is such a run).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd._lib import lib, check                                              # noqa: E402
from classpro_amd.api import Batch, Classifier, LabelAccuracy, hist_covs, threshold_labels   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                                        # noqa: E402

K = 40


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def derive_thresholds(hist, hcov, dcov, repeat_cov):
    low, _high, _il, _ih, h = hist
    lo = max(1, low)
    eh = lo + int(np.argmin(h[lo - low:hcov - low + 1]))
    return [eh, (hcov + dcov + 1) // 2, int(repeat_cov)]


def timed(fn, launches, warmup=3):
    """Seconds per launch: device events around `launches` calls after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / launches


def truth_labels(rd, b):
    """The truth label string in the label layout (relative profile 0 E, 1 H, 2 D, >= 3 R, as prof2class)."""
    dev = b.device
    ehdr = torch.tensor([ord(c) for c in "EHDR"], dtype=torch.uint8, device=dev)
    out = torch.full((max(b.total_bases, 1),), ord("N"), dtype=torch.uint8, device=dev)
    step = 1 << 27
    for a in range(0, b.total_kmers, step):
        e = min(a + step, b.total_kmers)
        k = torch.arange(a, e, device=dev)
        r = torch.searchsorted(b.prof_off, k, right=True) - 1
        out[k + (r + 1) * (K - 1)] = ehdr[rd["truth"][a:e].long().clamp(max=3)]
        del k, r
    return out


def score(est, truth, seq_off):
    A = LabelAccuracy(K)
    A.add(est, truth, seq_off)
    s = A.stats()
    A.close()
    return dict(accuracy_pct=s["accuracy"], fn_error_pct=s["fn_error"], ncor=s["ncor"], ntot=s["ntot"], cfm_ERHD=s["cfm"])


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = lib()
    t0 = time.time()
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    low, high, il, ih, h = ds.hist
    hcov, dcov = hist_covs(h, low, high, il, ih, 0)
    clf = Classifier(K=K, read_len=a.read_len, hcov=hcov, dcov=dcov, device=str(dev))
    thres = derive_thresholds(ds.hist, hcov, dcov, clf.export()["cov"][1])
    rd = ds.reads(0, ds.n_reads, truth=True)
    b = Batch.from_device(rd)
    truth = truth_labels(rd, b)
    nb, nk = b.total_bases, b.total_kmers
    res = dict(metric="ClassGS kernels", config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome, K=K,
               reads=b.nreads, total_bases=nb, total_kmers=nk, hcov=hcov, dcov=dcov, thresholds=thres, launches=a.launches,
               setup_s=time.time() - t0)

    # the classifier's labels, in sub-batches, into one label string
    lab_cp = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    so = ds.seq_off_all
    for first, count in ds.plan_batches(int(a.batch_mbases * 1e6)):
        sub = Batch.from_device(ds.reads(first, count))
        clf.classify(sub, check_overflow=False)
        clf.check()
        lab_cp[int(so[first]):int(so[first]) + sub.total_bases] = sub.labels[:sub.total_bases]
        del sub

    # cp_threshold_labels: characters + counts, packed + counts
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    t3 = (C.c_int32 * 3)(*thres)
    lab_gs, counts = threshold_labels(b, thres, K)
    (pk, pko), _ = threshold_labels(b, thres, K, packed=True)
    scratch = torch.zeros(4, dtype=torch.int64, device=dev)
    args = (K, t3, b.prof.data_ptr(), b.prof_off.data_ptr(), b.seq_off.data_ptr(), b.nreads, nb)
    t_lab = timed(lambda: check(L.cp_threshold_labels(*args, lab_gs.data_ptr(), None, None, scratch.data_ptr(), st)), a.launches)
    t_pk = timed(lambda: check(L.cp_threshold_labels(*args, None, pk.data_ptr(), pko.data_ptr(), scratch.data_ptr(), st)), a.launches)
    bytes_lab, bytes_pk = 2 * nk + nb, 2 * nk + int(pko[-1].item())
    # cp_acc_add (its memset of the per-read counters and its boundary pass included)
    A = LabelAccuracy(K)
    t_acc = timed(lambda: A.add(lab_gs, truth, b.seq_off), a.launches)
    A.close()
    bytes_acc = 2 * nb
    # cp_scan_candidates on the same counts
    bitmap = torch.zeros(nk // 64 + 2, dtype=torch.int64, device=dev)
    t_scan = timed(lambda: check(L.cp_scan_candidates(clf.p, b.prof.data_ptr(), nk, bitmap.data_ptr(), st)), a.launches)
    bytes_scan = 2 * nk + nk // 8
    res.update(threshold_labels=dict(s=t_lab, bytes=bytes_lab, tb_per_s=bytes_lab / t_lab / 1e12, gkmers_per_s=nk / t_lab / 1e9),
               threshold_packed=dict(s=t_pk, bytes=bytes_pk, tb_per_s=bytes_pk / t_pk / 1e12, gkmers_per_s=nk / t_pk / 1e9),
               acc_add=dict(s=t_acc, bytes=bytes_acc, tb_per_s=bytes_acc / t_acc / 1e12, gbases_per_s=nb / t_acc / 1e9),
               scan_candidates=dict(s=t_scan, bytes=bytes_scan, tb_per_s=bytes_scan / t_scan / 1e12),
               label_counts_EHDR=counts.tolist())
    res["accuracy_classpro"] = score(lab_cp, truth, b.seq_off)
    res["accuracy_classgs"] = score(lab_gs, truth, b.seq_off)
    res["value"], res["unit"] = res["threshold_labels"]["tb_per_s"], "TB/s"
    clf.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        scan = res["scan_candidates"]["tb_per_s"]
        with open(a.out, "w") as f:
            f.write("ClassGS kernels on one MI355X, BASELINE configs[2] (synthetic 200 Mbp diploid, 40x HiFi, %d reads, %.1f Gbases,\n"
                    "K = %d), the whole set in one call: `python scripts/classgs_bench.py`.  Device events around %d launches after\n"
                    "3 warm-up launches; bytes from the shapes.\n\n" % (b.nreads, nb / 1e9, K, a.launches))
            f.write("Thresholds (stand-in for GenomeScope, rule in scripts/classgs_bench.py): E/H %d (first minimum of the histogram),\n"
                    "H/D %d (midpoint of the peaks %d and %d), D/R %d (the classifier's repeat threshold)\n\n" % (thres[0], thres[1], hcov, dcov, thres[2]))
            for name, key, per in (("cp_threshold_labels, characters + counts", "threshold_labels", "2 B/k-mer in + 1 B/base out"),
                                   ("cp_threshold_labels, packed + counts", "threshold_packed", "2 B/k-mer in + 0.25 B/base out"),
                                   ("cp_acc_add", "acc_add", "2 B/base in"),
                                   ("cp_scan_candidates (same process)", "scan_candidates", "2 B/k-mer in + 1/8 B/k-mer out")):
                r = res[key]
                f.write("  %-42s %7.3f ms  %6.2f GB  %5.2f TB/s  (%s)  %4.2f x scan\n"
                        % (name, r["s"] * 1e3, r["bytes"] / 1e9, r["tb_per_s"], per, r["tb_per_s"] / scan))
            f.write("\nAccuracy against the truth (class2acc, default options: every read, every k-mer)\n")
            for name, key in (("ClassPro (the classifier)", "accuracy_classpro"), ("ClassGS (global thresholds)", "accuracy_classgs")):
                r = res[key]
                f.write("  %-28s %8.4f %%  (= %d / %d), FN error %.4f %%\n" % (name, r["accuracy_pct"], r["ncor"], r["ntot"], r["fn_error_pct"]))
            f.write("  labels of ClassGS (E, H, D, R): %s\n" % res["label_counts_EHDR"])
            f.write("\nRaw JSON line:\n%s\n" % line)


if __name__ == "__main__":
    main()

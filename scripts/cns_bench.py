"""Per-k-mer label table (class2cns, cp_kmer_table_*) on BASELINE configs[2]: one JSON line.

    python scripts/cns_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--cpu-mbases 50] [--no-cpu]

The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py), labelled by the classifier
in sub-batches and added to a forward table and then to a canonical one.  Reported: the table-build rate (bases added
per second of cp_kmer_table_add, growth steps included), the consensus-pass rate (forward table), distinct keys, final
slots, table bytes, growth steps, the consistency of both modes, and the class2acc-style agreement with the truth labels
of per-read labels against consensus labels.  The CPU baseline times the reference's text pipeline on a sample of the
first reads: `class2cns` (dump) | LC_ALL=C sort --parallel=16 | uniq -c, then agg2cons.py's mcf / harmonic-mean pass.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, Classifier, KmerTable, hist_covs   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                         # noqa: E402

K = 40
EHDR = torch.tensor([ord(c) for c in "EHDR"], dtype=torch.uint8)


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--cpu-mbases", type=float, default=50)
    ap.add_argument("--no-cpu", action="store_true")
    return ap.parse_args()


def truth_chars(rd, b):
    """Truth labels of every k-mer (relative profile 0 E, 1 H, 2 D, >= 3 R, as prof2class) and the base index of each
    k-mer end in the label layout."""
    dev = b.device
    nk = b.total_kmers
    k = torch.arange(nk, device=dev)
    r = torch.searchsorted(b.prof_off, k, right=True) - 1
    pos = k + (r + 1) * (K - 1)
    t = rd["truth"][:nk].long().clamp(max=3)
    return EHDR.to(dev)[t], pos


def run_mode(a, ds, clf, canonical, consensus):
    dev = ds.device
    T = KmerTable(K, canonical=canonical, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    t_add = 0.0
    bases = 0
    for first, count in batches:
        rd = ds.reads(first, count)
        b = Batch.from_device(rd)
        clf.classify(b, check_overflow=False)
        clf.check()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        T.add(b)
        torch.cuda.synchronize(dev)
        t_add += time.perf_counter() - t0
        bases += b.total_bases
        del rd, b
    s = T.stats()
    out = dict(build_gbases_per_s=bases / t_add / 1e9, build_s=t_add, bases=bases, n_kmers=s["n_kmers"],
               distinct=s["n_distinct"], unanimous=s["n_unanimous"], skipped=s["n_skipped"], slots=s["slots"],
               table_bytes=s["bytes"], growths=s["growths"], consistency=s["consistency"],
               label_total=s["label_total"], cns_total=s["cns_total"])
    if consensus:
        t_cns = 0.0
        agree_read = agree_cns = n = 0
        for first, count in batches:
            rd = ds.reads(first, count, truth=True)
            b = Batch.from_device(rd)
            clf.classify(b, check_overflow=False)
            clf.check()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            c = T.consensus(b)
            torch.cuda.synchronize(dev)
            t_cns += time.perf_counter() - t0
            tr, pos = truth_chars(rd, b)
            agree_read += int((b.labels[pos] == tr).sum().item())
            agree_cns += int((c[pos] == tr).sum().item())
            n += pos.numel()
            del rd, b, c, tr, pos
        T.stats()                                          # deferred errors of the consensus pass
        out.update(consensus_gbases_per_s=bases / t_cns / 1e9, consensus_s=t_cns,
                   accuracy_per_read=agree_read / n, accuracy_consensus=agree_cns / n)
    T.close()
    torch.cuda.empty_cache()
    return out


def cpu_baseline(a, ds, clf):
    """The reference's text pipeline on the first reads (about --cpu-mbases), timed step by step."""
    from classpro_amd import fastk
    so = ds.seq_off_all
    count = int(np.searchsorted(so, a.cpu_mbases * 1e6, side="left"))
    rd = ds.reads(0, count)
    b = Batch.from_device(rd)
    lab = clf.classify(b)
    seq = rd["seq"][:b.total_bases].cpu().numpy()
    d = tempfile.mkdtemp(prefix="cns_bench")
    est = os.path.join(d, "est.class")
    with open(est, "wb") as f:
        for i in range(count):
            s, e = so[i], so[i + 1]
            f.write(b"@read%d\n%s\n+\n%s\n" % (i + 1, seq[s:e].tobytes(), lab[s:e].tobytes()))
    fastk.write_fastk(d, "reads", K, [np.zeros(int(so[i + 1] - so[i]) - K + 1, np.uint16) for i in range(count)], ds.hist)
    cns = os.path.join(ROOT, "classpro_amd", "class2cns")
    env = dict(os.environ, LC_ALL="C")
    t0 = time.perf_counter()
    with open(os.path.join(d, "kmers"), "wb") as f:
        subprocess.run([cns, est, os.path.join(d, "reads")], stdout=f, check=True)
    t1 = time.perf_counter()
    subprocess.run("sort --parallel=16 -S 4G -T %s %s/kmers | uniq -c > %s/cnt" % (d, d, d), shell=True, check=True, env=env)
    t2 = time.perf_counter()
    n, inv_sum, prev, best, tot = 0, 0.0, None, 0, 0   # agg2cons.py: per k-mer mcf = max / total, then hmean
    with open(os.path.join(d, "cnt"), "rb") as f:
        for line in f:
            c, km, _l = line.split()
            if km != prev and prev is not None:
                n += 1
                inv_sum += tot / best
                best = tot = 0
            c = int(c)
            best, tot, prev = max(best, c), tot + c, km
    if prev is not None:
        n += 1
        inv_sum += tot / best
    t3 = time.perf_counter()
    txt_bytes = os.path.getsize(os.path.join(d, "kmers"))
    subprocess.run(["rm", "-rf", d], check=True)
    return dict(cpu_sample_bases=b.total_bases, cpu_dump_s=t1 - t0, cpu_sort_uniq_s=t2 - t1, cpu_python_s=t3 - t2,
                cpu_total_s=t3 - t0, cpu_gbases_per_s=b.total_bases / (t3 - t0) / 1e9, cpu_dump_bytes=txt_bytes,
                cpu_consistency=n / inv_sum if n else float("nan"))


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    t0 = time.time()
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    low, high, il, ih, h = ds.hist
    hcov, dcov = hist_covs(h, low, high, il, ih, 0)
    clf = Classifier(K=K, read_len=a.read_len, hcov=hcov, dcov=dcov, device=str(dev))
    res = dict(metric="class2cns table build", config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               K=K, reads=ds.n_reads, total_bases=ds.total_bases, setup_s=time.time() - t0)
    fw = run_mode(a, ds, clf, False, True)
    cn = run_mode(a, ds, clf, True, False)
    res["forward"] = fw
    res["canonical"] = cn
    res["value"] = fw["build_gbases_per_s"]
    res["unit"] = "Gbases/s"
    if not a.no_cpu:
        res.update(cpu_baseline(a, ds, clf))
    clf.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

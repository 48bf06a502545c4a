"""Per-class sorted k-mer tables (class2ktab, cp_kmer_table_sort / cp_kmer_table_class_hist) on BASELINE configs[2]: one
JSON line.

    python scripts/cnstab_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--cli-genome 25e6]
                                   [--workdir DIR] [--no-cli] [--no-export]

Library leg: the 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py), labelled by the
classifier in sub-batches of 500 Mbases and added to a canonical label table and, in the same process, to a count
table.  Reported: the seconds of each of the four class sorts (cp_kmer_table_sort, min_total 1, min_pct 0), of the
label = -1 sort, of cp_kmer_table_class_hist, of the encode over all four class snapshots (cp_kmer_sorted_ktab in
ranges of 16 M entries through one buffer), the entries per class, the snapshot bytes, and cp_kmer_counts_sort(1) on
the count table for comparison.  Both identities of "Sorted k-mers of a label table" are checked on the device: the
label = -1 snapshot equals the count table's (keys, counts, index, records range by range), and the four class
snapshots partition it (each strictly ascending, the sizes and the four indices add up, and a 64-bit hash summed over
the entries of the four equals that of the whole: equal as multisets, up to a hash collision).  The four class
histograms are summed against cp_kmer_counts_hist.

Export leg: cp_kmer_table_export, the host-side path that the snapshots replace, on a table of the first 1 Gbase only
(the full export needs about 45 GB of host memory).

Command leg: a 1-Gbase set of the same generator (--cli-genome) is labelled and written as a .class file with a .prof
stub under --workdir, and `class2ktab` runs on it once; reported are its wall seconds and the bytes it wrote.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, Classifier, KmerCounts, KmerTable, hist_covs   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                                     # noqa: E402

K = 40
RANGE = 16 << 20
PBYTE = ((K + 3) >> 2) - 3 + 2
LABELS = "EHDR"


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--cli-genome", type=float, default=25e6)
    ap.add_argument("--export-mbases", type=float, default=1000)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--no-export", action="store_true")
    return ap.parse_args()


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def ascending(s):
    if len(s) < 2:
        return True
    return bool(((s.hi[1:] > s.hi[:-1]) | ((s.hi[1:] == s.hi[:-1]) & (s.lo[1:] > s.lo[:-1]))).all())


def entry_hash(s):
    """The sum over the entries of a 64-bit mix of (hi, lo, count), wrapping: equal multisets give equal sums."""
    acc = 0
    for e in range(0, len(s), RANGE):
        hi, lo, c = s.hi[e:e + RANGE], s.lo[e:e + RANGE], s.counts[e:e + RANGE]
        x = (lo * -7046029254386353131) ^ (hi * -4417276706812531889) ^ (c * 1609587929392839161)
        x = (x ^ (x >> 29)) * -4658895280553007687
        x = x ^ (x >> 32)
        acc = (acc + int(x.sum().item())) & ((1 << 64) - 1)
    return acc


def encode_all(snaps, rec, idx, stream):
    for s in snaps:
        n = len(s)
        for e in range(0, max(n, 1), RANGE):
            rc = s.L.cp_kmer_sorted_ktab(s.s, e, min(RANGE, n - e), rec.data_ptr(), idx.data_ptr() if e == 0 else None, stream)
            assert rc == 0, rc


def library_leg(a, dev, ds, clf):
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    T, Cn = KmerTable(K, canonical=True, device=str(dev)), KmerCounts(K, device=str(dev))
    E = None if a.no_export else KmerTable(K, canonical=True, device=str(dev))
    bases = export_bases = 0
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        clf.classify(b, check_overflow=False)
        clf.check()
        T.add(b)
        Cn.add(b)
        if E is not None and export_bases < a.export_mbases * 1e6:
            E.add(b)
            export_bases += b.total_bases
        bases += b.total_bases
        del b
    st, cst = T.stats(), Cn.stats()
    say("tables built: %d distinct keys" % st["n_distinct"])
    out = dict(total_bases=bases, distinct=st["n_distinct"], unanimous=st["n_unanimous"], slots=st["slots"],
               table_bytes=st["bytes"], cns_total=st["cns_total"], count_table_distinct=cst["n_distinct"])
    export = None
    if E is not None:                                      # first, while the host and the device hold nothing else
        t0 = time.perf_counter()
        hi, lo, cnt = E.entries()
        export = dict(bases=export_bases, entries=int(len(hi)), export_s=time.perf_counter() - t0,
                      host_bytes=int(hi.nbytes + lo.nbytes + cnt.nbytes))
        say("export: %s" % export)
        del hi, lo, cnt
        E.close()
        torch.cuda.empty_cache()

    t, (h, il, ih) = timed(dev, T.class_hist)
    low, high, ilow, ihigh, want = Cn.hist()
    out["class_hist_s"] = t
    out["class_hist_sums_to_count_hist"] = bool(np.array_equal(h.sum(0), want) and int(il.sum()) == ilow
                                                and int(ih.sum()) == ihigh)
    t, cs = timed(dev, lambda: Cn.sorted(1))
    out["counts_sort_s"], out["counts_sort_entries"] = t, len(cs)
    t, every = timed(dev, lambda: T.sorted())
    out["all_sort_s"], out["all_entries"], out["all_snapshot_bytes"] = t, len(every), every.nbytes
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rec = torch.empty(RANGE * PBYTE, dtype=torch.uint8, device=dev)
    rec2 = torch.empty(RANGE * PBYTE, dtype=torch.uint8, device=dev)
    idx = torch.empty(1 << 24, dtype=torch.int64, device=dev)
    idx2 = torch.empty(1 << 24, dtype=torch.int64, device=dev)
    same = len(every) == len(cs) and all(torch.equal(getattr(every, f), getattr(cs, f)) for f in ("hi", "lo", "counts"))
    for e in range(0, len(every), RANGE):
        if not same:
            break
        m = min(RANGE, len(every) - e)
        assert every.L.cp_kmer_sorted_ktab(every.s, e, m, rec.data_ptr(), idx.data_ptr() if e == 0 else None, stream) == 0
        assert cs.L.cp_kmer_sorted_ktab(cs.s, e, m, rec2.data_ptr(), idx2.data_ptr() if e == 0 else None, stream) == 0
        same = torch.equal(rec[:m * PBYTE], rec2[:m * PBYTE]) and (e > 0 or torch.equal(idx, idx2))
    out["all_equals_counts_sort"] = bool(same)
    whole_hash, whole_idx = entry_hash(every), idx2.clone()
    cs.close()
    every.close()
    del rec2, idx2
    torch.cuda.empty_cache()

    snaps, per = [], {}
    for l in LABELS:
        t, s = timed(dev, lambda: T.sorted(l))
        snaps.append(s)
        per[l] = dict(sort_s=t, entries=len(s), snapshot_bytes=s.nbytes, keys_in_hist=int(h[LABELS.index(l)].sum()),
                      occurrences=int(s.counts.sum().item()) if len(s) else 0)
        say("class %s: %s" % (l, per[l]))
    out["classes"] = per
    out["class_sorts_total_s"] = sum(p["sort_s"] for p in per.values())
    out["class_snapshot_bytes_total"] = sum(p["snapshot_bytes"] for p in per.values())
    t, _ = timed(dev, lambda: encode_all(snaps, rec, idx, stream))
    out["encode_all_classes_s"] = t
    out["encode_entries"] = sum(len(s) for s in snaps)
    isum = torch.zeros_like(whole_idx)
    for s in snaps:
        isum += s.ktab(0, 0)[1]
    out["classes_partition_all"] = bool(all(ascending(s) for s in snaps) and sum(len(s) for s in snaps) == out["all_entries"]
                                        and torch.equal(isum, whole_idx)
                                        and sum(entry_hash(s) for s in snaps) & ((1 << 64) - 1) == whole_hash
                                        and [p["occurrences"] for p in per.values()] == st["cns_total"]
                                        and [p["entries"] for p in per.values()] == [p["keys_in_hist"] for p in per.values()])
    for s in snaps:
        s.close()
    T.close()
    Cn.close()
    torch.cuda.empty_cache()
    return out, export


def command_leg(a, dev, clf_args):
    work = tempfile.mkdtemp(prefix="cnstab_bench_", dir=a.workdir)
    try:
        ds = DeviceSynth(genome_len=int(a.cli_genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
        clf = Classifier(device=str(dev), **clf_args)
        est = os.path.join(work, "reads.class")
        bases = 0
        with open(est, "wb") as f:
            for first, count in ds.plan_batches(int(a.batch_mbases * 1e6)):
                rd = ds.reads(first, count)
                b = Batch.from_device(rd)
                lab = clf.classify(b)
                seq, off = rd["seq"].cpu().numpy(), rd["seq_off_h"]
                for r in range(count):
                    f.write(b"@r%d\n" % (first + r))
                    f.write(seq[off[r]:off[r + 1]].tobytes())
                    f.write(b"\n+\n")
                    f.write(lab[off[r]:off[r + 1]].tobytes())
                    f.write(b"\n")
                bases += rd["total_bases"]
                del rd, b
        clf.close()
        del ds
        torch.cuda.empty_cache()
        with open(os.path.join(work, "reads.prof"), "wb") as f:      # class2ktab reads K from the stub alone
            f.write(struct.pack("<ii", K, 0))
        say("wrote %s: %d bases" % (est, bases))
        out = dict(total_bases=bases, class_bytes=os.path.getsize(est))
        d = os.path.join(work, "out")
        os.mkdir(d)
        t0 = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "classpro_amd", "class2ktab"), "-v", "-N" + os.path.join(d, "reads"), est,
                            os.path.join(work, "reads")], capture_output=True, text=True)
        out["class2ktab_s"] = time.perf_counter() - t0
        if r.returncode != 0:
            raise RuntimeError("class2ktab failed: %s" % r.stderr)
        out["stderr"] = r.stderr.strip().split("\n")
        files = [os.path.join(d, f) for f in os.listdir(d)]
        out["files"] = len(files)
        out["bytes_written"] = sum(os.path.getsize(p) for p in files)
        out["ktab_bytes"] = sum(os.path.getsize(p) for p in files if "ktab" in p)
        return out
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    low, high, il, ih, h = ds.hist
    hcov, dcov = hist_covs(h, low, high, il, ih, 0)
    clf_args = dict(K=K, read_len=a.read_len, hcov=hcov, dcov=dcov)
    clf = Classifier(device=str(dev), **clf_args)
    res = dict(metric="class2ktab per-class sorted k-mer tables", K=K,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome)
    res["library"], export = library_leg(a, dev, ds, clf)
    if export is not None:
        res["export"] = export
    clf.close()
    del ds
    torch.cuda.empty_cache()
    if not a.no_cli:
        res["command"] = command_leg(a, dev, clf_args)
        res["command"]["config"] = "genome %d, cov %g" % (a.cli_genome, a.cov)
    res["value"], res["unit"] = res["library"]["class_sorts_total_s"], "s"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

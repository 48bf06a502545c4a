"""K-mer count table (kprof, cp_kmer_counts_*) on BASELINE configs[2]: one JSON line.

    python scripts/kprof_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--counts-only] [--filter-log2 N ...]

The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of 500 Mbases.
Reported for the count table: the add rate with growth from the default size and again with the table pre-sized (no
growth), the profile-pass rate, the histogram time, distinct keys, slots, bytes, growth steps, hist_covs of the counted
histogram next to that of the set's own, the fraction of cells where counted and synthesised profiles agree, and the
classifier's agreement with the truth on counted against synthesised profiles.

The yardstick is the label table in the same process: KmerTable(K, canonical=True).add on the same batches (labelled by
the classifier) and its consensus pass, each measured twice; the spread between the two repeats is the margin.  The count
table does a subset of that work per occurrence, so `add_ok` / `profile_ok` say whether its rates are not lower:
rate >= mean of the two baseline repeats - their spread.  --counts-only skips the baselines (for a run under a profiler,
or of another build of the library named by CLASSPRO_AMD_LIB).

--filter-log2 N ... adds a leg per N, under the key "filtered": the FILTERED count table (KmerCounts(filter_bits=2^N),
DESIGN.md 9.10) on the same batches -- mark, count and profile rates, table keys, keys kept outside, false positives,
final slots and bytes, and the peak device bytes of the build (filter + failure bitmaps + table + the old table during
the last rehash; computed from the first-batch sizing, the final slots and the growth steps: exact when every step
doubled the table, "peak_exact", otherwise the bound final + final/2) -- and whether its statistics and low histogram
bins equal the unfiltered table's.  Without the flag the output is what it was.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, Classifier, KmerCounts, KmerTable, hist_covs   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                                     # noqa: E402

K = 40
EHDR = torch.tensor([ord(c) for c in "EHDR"], dtype=torch.uint8)


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--counts-only", action="store_true")
    ap.add_argument("--filter-log2", type=int, nargs="+", default=[])
    return ap.parse_args()


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def label_table(ds, clf, batches, canonical, consensus_repeats):
    """The existing label table on the same batches: add rate, then `consensus_repeats` timed consensus passes."""
    dev = ds.device
    T = KmerTable(K, canonical=canonical, device=str(dev))
    t_add, bases = 0.0, 0
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        clf.classify(b, check_overflow=False)
        clf.check()
        t_add += timed(dev, lambda: T.add(b))
        bases += b.total_bases
        del b
    s = T.stats()
    out = dict(add_gbases_per_s=bases / t_add / 1e9, add_s=t_add, distinct=s["n_distinct"], slots=s["slots"],
               table_bytes=s["bytes"], growths=s["growths"], consensus_gbases_per_s=[], consensus_s=[])
    for _ in range(consensus_repeats):
        t_cns = 0.0
        for first, count in batches:
            b = Batch.from_device(ds.reads(first, count))
            clf.classify(b, check_overflow=False)
            clf.check()
            out_t = b.labels.clone()                       # KmerTable.consensus without its clone in the timed part
            t_cns += timed(dev, lambda: T.L.cp_kmer_table_consensus(T.t, b.seq.data_ptr(), b.seq_off.data_ptr(), b.nreads,
                                                                     b.total_bases, out_t.data_ptr(), T._stream()))
            del b, out_t
        T.stats()
        out["consensus_gbases_per_s"].append(bases / t_cns / 1e9)
        out["consensus_s"].append(t_cns)
    T.close()
    torch.cuda.empty_cache()
    return out


def count_table(ds, batches, initial_slots, clf=None):
    """The count table: add rate; with `clf` also the profile pass (twice: timed alone, then compared), the histogram
    and the classifier on counted against synthesised profiles."""
    dev = ds.device
    T = KmerCounts(K, device=str(dev), initial_slots=initial_slots)
    t_add, bases = 0.0, 0
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        t_add += timed(dev, lambda: T.add(b))
        bases += b.total_bases
        del b
    s = T.stats()
    out = dict(add_gbases_per_s=bases / t_add / 1e9, add_s=t_add, bases=bases, n_kmers=s["n_kmers"],
               distinct=s["n_distinct"], skipped=s["n_skipped"], slots=s["slots"], table_bytes=s["bytes"],
               growths=s["growths"])
    if clf is None:
        T.close()
        torch.cuda.empty_cache()
        return out
    hist = [None]
    out["hist_s"] = timed(dev, lambda: hist.__setitem__(0, T.hist()))
    low, high, il, ih, h = hist[0]
    out["hist_covs_counted"] = list(hist_covs(h, low, high, il, ih, 0))
    out["hist_covs_set"] = list(hist_covs(ds.hist[4], *ds.hist[:4], 0))
    out["hist_low_bins_counted"] = [int(x) for x in h[:4]]
    out["hist_low_bins_set"] = [int(x) for x in ds.hist[4][:4]]
    out["ilowcnt"], out["ihighcnt"] = il, ih
    clf_c = Classifier(K=K, read_len=clf.read_len, hcov=out["hist_covs_counted"][0], dcov=out["hist_covs_counted"][1],
                       device=str(dev))
    for rep in range(2):
        t_prof = 0.0
        same = cells = ok_syn = ok_cnt = 0
        for first, count in batches:
            rd = ds.reads(first, count, truth=True)
            b = Batch.from_device(rd)
            if rep == 0:
                dst = torch.empty_like(b.prof)
                t_prof += timed(dev, lambda: T.L.cp_kmer_counts_profiles(T.t, b.seq.data_ptr(), b.seq_off.data_ptr(),
                                                                         b.prof_off.data_ptr(), b.nreads, b.total_bases,
                                                                         dst.data_ptr(), T._stream()))
                del dst
            else:                                              # the comparisons, outside the timed run
                nk = b.total_kmers
                k = torch.arange(nk, device=dev)
                r = torch.searchsorted(b.prof_off, k, right=True) - 1
                pos = k + (r + 1) * (K - 1)
                del k, r
                tr = EHDR.to(dev)[rd["truth"][:nk].long().clamp(max=3)]
                clf.classify(b, check_overflow=False)
                clf.check()
                ok_syn += int((b.labels[pos] == tr).sum().item())
                syn = b.prof[:nk].clone()
                T.profiles(b)
                same += int((b.prof[:nk] == syn).sum().item())
                cells += nk
                clf_c.classify(b, check_overflow=False)
                clf_c.check()
                ok_cnt += int((b.labels[pos] == tr).sum().item())
                del pos, tr, syn
            del rd, b
        T.stats()                                              # deferred errors of the profile pass
        if rep == 0:
            out["profile_gbases_per_s"] = bases / t_prof / 1e9
            out["profile_s"] = t_prof
        else:
            out.update(profile_cells=cells, profile_agreement=same / cells, accuracy_synthesised=ok_syn / cells,
                       accuracy_counted=ok_cnt / cells)
    clf_c.close()
    T.close()
    torch.cuda.empty_cache()
    return out


def filtered_table(ds, batches, log2_bits, unfiltered):
    """The filtered count table: mark, count and profile rates over the same batches, and what the filter kept out."""
    dev = ds.device
    T = KmerCounts(K, device=str(dev), filter_bits=1 << log2_bits)
    filter_bytes = T.filter_stats()["filter_bytes"]
    t_mark = t_add = t_prof = 0.0
    first_bases = None
    bases = 0
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        t_mark += timed(dev, lambda: T.mark(b))
        bases += b.total_bases
        if first_bases is None:
            first_bases = b.total_bases
        del b
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        t_add += timed(dev, lambda: T.add(b))
        del b
    s, f = T.stats(), T.filter_stats()
    low, high, il, ih, h = T.hist()
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        dst = torch.empty_like(b.prof)
        t_prof += timed(dev, lambda: T.L.cp_kmer_counts_profiles(T.t, b.seq.data_ptr(), b.seq_off.data_ptr(),
                                                                 b.prof_off.data_ptr(), b.nreads, b.total_bases,
                                                                 dst.data_ptr(), T._stream()))
        del b, dst
    T.stats()
    T.close()
    torch.cuda.empty_cache()
    single = int(h[0])
    sized = max(1 << 20, 1 << (first_bases // 2 - 1).bit_length())         # the first-batch sizing of a filtered table
    peak = s["bytes"] + (32 * (s["slots"] // 2) if s["growths"] else 0)    # bytes: table + failure bitmaps + filter
    return dict(filter_log2=log2_bits, filter_bytes=filter_bytes, mark_gbases_per_s=bases / t_mark / 1e9, mark_s=t_mark,
                count_gbases_per_s=bases / t_add / 1e9, count_s=t_add, profile_gbases_per_s=bases / t_prof / 1e9,
                profile_s=t_prof, n_kmers=s["n_kmers"], distinct=s["n_distinct"], skipped=s["n_skipped"],
                table_keys=f["n_table_keys"], outside=f["n_outside"], false_positives=f["n_false"],
                false_share_of_singletons=f["n_false"] / max(single, 1), slots=s["slots"], table_bytes=s["bytes"],
                growths=s["growths"], peak_bytes=peak, peak_exact=s["slots"] == sized << s["growths"],
                hist_low_bins=[int(x) for x in h[:4]], ilowcnt=il, ihighcnt=ih,
                same_as_unfiltered=(s["n_kmers"] == unfiltered["n_kmers"] and s["n_distinct"] == unfiltered["distinct"]
                                    and s["n_skipped"] == unfiltered["skipped"] and il == unfiltered["ilowcnt"]
                                    and ih == unfiltered["ihighcnt"]
                                    and [int(x) for x in h[:4]] == unfiltered["hist_low_bins_counted"]))


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    t0 = time.time()
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    hcov, dcov = hist_covs(ds.hist[4], *ds.hist[:4], 0)
    clf = Classifier(K=K, read_len=a.read_len, hcov=hcov, dcov=dcov, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    res = dict(metric="kprof count table", config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               K=K, reads=ds.n_reads, total_bases=ds.total_bases, batches=len(batches), setup_s=time.time() - t0)
    if not a.counts_only:
        res["label_canonical_1"] = label_table(ds, clf, batches, True, 2)
    cnt = count_table(ds, batches, 0, clf)
    res["counts"] = cnt
    if not a.counts_only:
        res["label_canonical_2"] = label_table(ds, clf, batches, True, 0)
    res["counts_presized"] = count_table(ds, batches, cnt["slots"])
    if not a.counts_only:
        res["label_forward"] = label_table(ds, clf, batches, False, 1)
        adds = [res["label_canonical_1"]["add_gbases_per_s"], res["label_canonical_2"]["add_gbases_per_s"]]
        cns = res["label_canonical_1"]["consensus_gbases_per_s"]
        res["baseline_add_gbases_per_s"], res["baseline_add_spread"] = sum(adds) / 2, abs(adds[0] - adds[1])
        res["baseline_consensus_gbases_per_s"], res["baseline_consensus_spread"] = sum(cns) / 2, abs(cns[0] - cns[1])
        res["add_ok"] = cnt["add_gbases_per_s"] >= res["baseline_add_gbases_per_s"] - res["baseline_add_spread"]
        res["profile_ok"] = (cnt["profile_gbases_per_s"]
                             >= res["baseline_consensus_gbases_per_s"] - res["baseline_consensus_spread"])
        res["profile_ok_vs_forward"] = (cnt["profile_gbases_per_s"] >= res["label_forward"]["consensus_gbases_per_s"][0]
                                        - res["baseline_consensus_spread"])
    if a.filter_log2:
        res["filtered"] = [filtered_table(ds, batches, n, cnt) for n in a.filter_log2]
    res["value"], res["unit"] = cnt["add_gbases_per_s"], "Gbases/s"
    clf.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

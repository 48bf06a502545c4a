"""Relative labels (genome2class, cp_kmer_counts_rel_labels) on BASELINE configs[2]: one JSON line, and with --out the
text of profiles/truth_configs2.txt.

    python scripts/truth_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--repeats 5] [--out FILE]

The configs[2] set is generated on the device (DeviceSynth, the set of bench.py).  Its two haplotypes -- `gen & 3` and
`(gen >> 2) & 3` of the synthesiser's genome, as A C G T bytes: two contigs -- are added to a count table in pieces that
overlap by K-1 bases, as genome2class adds an assembly.  Then every read batch goes through
  fused          cp_kmer_counts_rel_labels: characters + counts; the same with the relative profile; packed + counts;
  chain          what it replaces: cp_kmer_counts_profiles into a buffer, then cp_threshold_labels with thresholds 1 2 3
                 (characters + counts),
on the same batch in the same process: one warm-up each, then --repeats timed runs each, interleaved.  A repeat's rate
is the set's bases over the sum of its batch times (a synchronised wall clock around each call); reported are the
median and the spread (max - min) of the repeats, and `fused_ok`: median(fused) >= median(chain) - spread.
Last, the labels from the table against DeviceSynth's by-construction truth, by label pair: information, not a gate
(low-complexity runs and chance repeats are counted exactly by a table and not by construction).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd._lib import ClassProError, check, lib        # noqa: E402
from classpro_amd.api import Batch, KmerCounts                  # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                  # noqa: E402

K = 40
VARIANTS = ("fused_labels", "fused_labels_profile", "fused_packed", "chain")


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--piece-mbases", type=float, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    return ap.parse_args()


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def add_genome(dev, haps, piece, initial_slots=0):
    """The haplotypes into a fresh table, a batch per piece of `piece` + K-1 bases; (table, seconds, pieces)."""
    T = KmerCounts(K, device=str(dev), initial_slots=initial_slots)
    t, n = 0.0, 0
    for h in haps:
        for s in range(0, h.numel() - (K - 1), piece):
            x = h[s:s + piece + K - 1]
            off = torch.tensor([0, x.numel()], dtype=torch.int64, device=dev)
            t += timed(dev, lambda: T.add_tensors(x, off))
            n += 1
    return T, t, n


def main():
    a = parse()
    assert a.repeats >= 5, "medians of at least five repeats"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = lib()
    t0 = time.time()
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    haps = [acgt[(ds.gen & 3).long()], acgt[((ds.gen >> 2) & 3).long()]]
    gbases = sum(h.numel() for h in haps)
    piece = int(a.piece_mbases * 1e6)
    res = dict(metric="relative labels", config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               K=K, reads=ds.n_reads, total_bases=ds.total_bases, genome_bases=gbases, setup_s=time.time() - t0)

    # ---- the genome into the table: a small throw-away add first (warm-up), then twice into a fresh table
    W, _, _ = add_genome(dev, [haps[0][:4_000_000]], piece)
    W.close()
    adds = []
    for rep in range(2):
        T, t, npieces = add_genome(dev, haps, piece)
        s = T.stats()
        adds.append(dict(s=t, gbases_per_s=gbases / t / 1e9, growths=s["growths"]))
        if rep == 0:
            T.close()
            del T
            torch.cuda.empty_cache()
    res.update(pieces=npieces, piece_bases=piece, add=adds, n_kmers=s["n_kmers"], distinct=s["n_distinct"],
               skipped=s["n_skipped"], slots=s["slots"], table_bytes=s["bytes"])

    # ---- the reads
    st = T._stream()
    thres = (C.c_int32 * 3)(1, 2, 3)
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    times = {v: [0.0] * a.repeats for v in VARIANTS}
    pairs = torch.zeros(16, dtype=torch.int64, device=dev)           # [truth by construction][from the table], E H D R
    totals = {v: None for v in VARIANTS}
    bases = 0
    for first, count in batches:
        rd = ds.reads(first, count, truth=True)
        b = Batch.from_device(rd)
        n, total, nk = b.nreads, b.total_bases, b.total_kmers
        bases += total
        lab = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        prof = torch.empty(max(nk, 8), dtype=torch.int16, device=dev)
        pko = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum((b.seq_off[1:] - b.seq_off[:-1] + 3) >> 2, 0, out=pko[1:])
        pk = torch.empty(max(int(pko[-1].item()), 1), dtype=torch.uint8, device=dev)
        cnt = {v: torch.zeros(4, dtype=torch.int64, device=dev) for v in VARIANTS}
        seq, so, po = b.seq.data_ptr(), b.seq_off.data_ptr(), b.prof_off.data_ptr()
        run = dict(
            fused_labels=lambda: check(L.cp_kmer_counts_rel_labels(T.t, seq, so, n, total, None, None, lab.data_ptr(), None,
                                                                    None, cnt["fused_labels"].data_ptr(), st)),
            fused_labels_profile=lambda: check(L.cp_kmer_counts_rel_labels(T.t, seq, so, n, total, prof.data_ptr(), po,
                                                                            lab.data_ptr(), None, None,
                                                                            cnt["fused_labels_profile"].data_ptr(), st)),
            fused_packed=lambda: check(L.cp_kmer_counts_rel_labels(T.t, seq, so, n, total, None, None, None, pk.data_ptr(),
                                                                    pko.data_ptr(), cnt["fused_packed"].data_ptr(), st)),
            chain=lambda: (check(L.cp_kmer_counts_profiles(T.t, seq, so, po, n, total, prof.data_ptr(), st)),
                           check(L.cp_threshold_labels(K, thres, prof.data_ptr(), po, so, n, total, lab.data_ptr(), None,
                                                       None, cnt["chain"].data_ptr(), st))))
        for v in VARIANTS:                                           # warm-up, and the chain's labels as the yardstick
            run[v]()
        torch.cuda.synchronize(dev)
        chain_lab = lab.clone()
        run["fused_labels_profile"]()
        torch.cuda.synchronize(dev)
        assert torch.equal(lab, chain_lab), "the fused call and the chain disagree"
        ours = prof[:nk].long().clamp(max=3)                          # int16 storage, values in [0, 32767]
        pairs += torch.bincount(rd["truth"][:nk].long().clamp(max=3) * 4 + ours, minlength=16)
        del chain_lab, ours
        for v in VARIANTS:
            cnt[v].zero_()
        for rep in range(a.repeats):
            for v in VARIANTS:
                times[v][rep] += timed(dev, run[v])
        for v in VARIANTS:
            c = (cnt[v] // a.repeats).tolist()
            totals[v] = c if totals[v] is None else [x + y for x, y in zip(totals[v], c)]
        del rd, b, lab, prof, pk, pko
    try:                                                             # the chain's profile pass met absent k-mers: its
        T.stats()                                                    # deferred error, reported once
        res["chain_deferred_error"] = False
    except ClassProError:
        res["chain_deferred_error"] = True
    T.close()
    assert all(totals[v] == totals["chain"] for v in VARIANTS), totals
    res.update(batches=len(batches), read_bases=bases, label_counts=totals["chain"])
    for v in VARIANTS:
        r = [bases / t / 1e9 for t in times[v]]
        res[v] = dict(gbases_per_s=r, median=statistics.median(r), spread=max(r) - min(r))
    margin = max(res["chain"]["spread"], res["fused_labels"]["spread"])
    res["margin"] = margin
    res["fused_ok"] = res["fused_labels"]["median"] >= res["chain"]["median"] - margin
    res["fused_profile_ok"] = res["fused_labels_profile"]["median"] >= res["chain"]["median"] - margin
    p = pairs.reshape(4, 4).tolist()
    res["truth_by_construction_vs_table"] = p
    res["truth_differs"] = sum(p[i][j] for i in range(4) for j in range(4) if i != j)
    res["value"], res["unit"] = res["fused_labels"]["median"], "Gbases/s"
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(report(res))


def report(r):
    g = lambda v: "%.2f Gbases/s median of %d (min %.2f, max %.2f, spread %.2f)" % (
        r[v]["median"], len(r[v]["gbases_per_s"]), min(r[v]["gbases_per_s"]), max(r[v]["gbases_per_s"]), r[v]["spread"])
    lines = [
        "Relative labels (genome2class: cp_kmer_counts_add of the genome, cp_kmer_counts_rel_labels of the reads) on one",
        "MI355X, BASELINE %s (synthetic diploid, %d reads, %.2f Gbases, K = %d), generated on the device:" % (
            r["config"], r["reads"], r["read_bases"] / 1e9, r["K"]),
        "`python scripts/truth_bench.py --out profiles/truth_configs2.txt`.",
        "",
        "Genome into the count table (two haplotypes as two contigs, %d bases, %d pieces of %d + K-1 bases)" % (
            r["genome_bases"], r["pieces"], r["piece_bases"]),
    ]
    for i, a in enumerate(r["add"]):
        lines.append("  add, fresh table %d     %.2f Gbases/s (%.3f s, %d growth steps)" % (i + 1, a["gbases_per_s"], a["s"], a["growths"]))
    lines += [
        "  k-mers / distinct      %d / %d, skipped %d" % (r["n_kmers"], r["distinct"], r["skipped"]),
        "  slots / bytes          %d / %.1f GB (%d bytes)" % (r["slots"], r["table_bytes"] / 1e9, r["table_bytes"]),
        "",
        "Reads through the table (%d batches, one warm-up and %d timed repeats of each form per batch, interleaved;" % (
            r["batches"], len(r["chain"]["gbases_per_s"])),
        "a repeat's rate = all bases / the sum of its batch times, synchronised wall clock around each call)",
        "  fused, characters + counts             %s" % g("fused_labels"),
        "  fused, characters + profile + counts   %s" % g("fused_labels_profile"),
        "  fused, packed + counts                 %s" % g("fused_packed"),
        "  chain: cp_kmer_counts_profiles, then   %s" % g("chain"),
        "  cp_threshold_labels 1 2 3 (characters + counts)",
        "  margin (the larger spread of chain and fused characters)   %.2f Gbases/s" % r["margin"],
        "  fused characters not slower than the chain: %s (%.2f against %.2f - %.2f)" % (
            "yes" if r["fused_ok"] else "NO", r["fused_labels"]["median"], r["chain"]["median"], r["margin"]),
        "  fused characters + profile not slower than the chain: %s (%.2f against %.2f - %.2f)" % (
            "yes" if r["fused_profile_ok"] else "NO", r["fused_labels_profile"]["median"], r["chain"]["median"], r["margin"]),
        "  label counts E H D R   %s (the same from all four forms; the fused labels equal the chain's on every batch)" % r["label_counts"],
        "  the chain's profile pass left the table's deferred error set: %s" % ("yes" if r["chain_deferred_error"] else "no"),
        "",
        "Labels from the table against DeviceSynth's by-construction truth, k-mer positions (information, not a gate)",
        "  rows: by construction E H D R; columns: from the table E H D R",
    ]
    for i, row in enumerate(r["truth_by_construction_vs_table"]):
        lines.append("  %s  %s" % ("EHDR"[i], " ".join("%13d" % x for x in row)))
    tot = sum(sum(row) for row in r["truth_by_construction_vs_table"])
    lines.append("  differing: %d of %d positions (%.4f %%)" % (r["truth_differs"], tot, 100.0 * r["truth_differs"] / max(tot, 1)))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    main()

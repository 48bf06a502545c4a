"""Phasing heterozygous sites from reads (tabphase, cp_kmer_sorted_read_links, cp_kmer_counts_add_keys, cp_phase_forest) on
BASELINE configs[2]: one JSON line, and with --out a text file that holds the summary and the line
(profiles/phase_configs2.txt).

    python scripts/phase_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of
500 Mbases; F = `KmerCounts.sorted(1)` of all reads, P = its unique heterozygous pairs under the range 5-.  After one
untimed pass over all batches, two timed passes in which the same batch goes through
  links     read_links(P, mark) at the exact capacity (the counting call is not timed)
  add_keys  add_keys of those links into a KmerCounts of K = 32
  profiles  one cp_kmer_sorted_profiles on P                                     a call that existed before
  runs      cp_kmer_sorted_read_runs(P) in absence mode (emit NONE)              a call that existed before
one after the other, each timed with a device synchronise on both sides.  Then the sort of the link table, the forest and
the split, and for scale `unitigs(components=True)` on P.  Reported: Gbases/s of the read passes, the keys per second of
add_keys, the seconds of the forest per edge, every tally, the block N50 in sites, and the score against the generator's
truth: DeviceSynth.gen holds both haplotypes per position (A | B << 2 | snp << 4), the two strings are spelled from it, each
is counted into a table of its own, and every k-mer of P is looked up in both.  A site is SCORED when it lies in a block and
its low k-mer occurs in exactly one haplotype; the score is the share of scored sites whose side agrees with that
haplotype, each block taken with whichever of its two flips agrees more.  That score is a Hamming distance: one wrong edge
of the forest flips everything behind it, so the sign of every kept edge between two scored sites is held against the
haplotypes as well, which says how good the votes are before the forest chooses among them.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, KmerCounts, SortedKmers, phase_forest   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth   # noqa: E402

K = 40
RANGE = (5, None)
CALLS = ("links", "add_keys", "profiles", "runs")


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--min-support", type=int, default=2)
    ap.add_argument("--out", default=None)
    return ap.parse_args()


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def n50(sizes):
    sizes = sorted(sizes, reverse=True)
    half, run = sum(sizes) / 2, 0
    for s in sizes:
        run += s
        if run >= half:
            return s
    return 0


def truth_of(ds, P, mark, dev):
    """Per site, the haplotype (0 or 1) that alone holds its low k-mer, -1 where both or neither do."""
    lut = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    off = torch.tensor([0, ds.G], dtype=torch.int64, device=dev)
    held = []
    for shift in (0, 2):
        hap = lut[((ds.gen >> shift) & 3).long()]
        T = KmerCounts(K, device=str(dev))
        T.add_tensors(hap, off)
        S = T.sorted(1)
        T.close()
        held.append(S.find(P.hi, P.lo) >= 0)
        S.close()
        del hap
    low = (mark >= 0) & ((mark & 1) == 0)                  # in site order: the low members ascend with their sites
    in_a, in_b = held[0][low], held[1][low]
    truth = torch.full_like(in_a, -1, dtype=torch.int64)
    truth[in_a & ~in_b] = 0
    truth[in_b & ~in_a] = 1
    return truth


def score(truth, block, side):
    """(scored sites, those that agree under the better flip of their block)"""
    sizes = torch.bincount(block, minlength=block.numel())
    ok = (truth >= 0) & (sizes[block] >= 2)
    b, agree = block[ok], (side[ok].long() == truth[ok]).long()
    n = torch.bincount(b, minlength=block.numel())
    g = torch.bincount(b, weights=agree.double(), minlength=block.numel()).long()
    return int(ok.sum()), int(torch.maximum(g, n - g).sum())


def edge_truth(edges, truth, min_support):
    """(kept edges between two sites of known haplotype, those whose sign is the truth's): says how good the votes are
    before the forest chooses among them."""
    key, cnt = edges.lo, edges.counts
    if key.numel() == 0:
        return 0, 0
    pair, inv = torch.unique_consecutive(key >> 1, return_inverse=True)
    cis = torch.zeros(pair.numel(), dtype=torch.int64, device=key.device).index_add_(0, inv, cnt * ((key & 1) == 0))
    trans = torch.zeros_like(cis).index_add_(0, inv, cnt * ((key & 1) == 1))
    s, t = pair >> 31, pair & 0x7FFFFFFF
    kept = (torch.maximum(cis, trans) >= min_support) & (cis != trans) & (truth[s] >= 0) & (truth[t] >= 0)
    right = kept & ((trans > cis).long() == (truth[s] ^ truth[t]))
    return int(kept.sum()), int(right.sum())


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    T = KmerCounts(K, device=str(dev))
    for first, count in batches:
        rd = ds.reads(first, count)
        T.add_tensors(rd["seq"], rd["seq_off"])
        del rd
    F = T.sorted(1)
    T.close()
    t_pairs, res_p = timed(dev, lambda: F.het_pairs(xmax=1, ymax=1, unique=True, count_range=RANGE, table=True))
    P = res_p[2]
    nf = len(F)
    F.close()
    t_sites, (mark, nsites, sites) = timed(dev, P.het_sites)
    truth = truth_of(ds, P, mark, dev)
    say("F %d entries, P %d, %d sites" % (nf, len(P), nsites))
    res = dict(metric="phasing heterozygous sites from reads", K=K, range="5-", min_support=a.min_support,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, batches=len(batches), f_entries=nf, p_entries=len(P), nsites=nsites, sites=sites,
               het_pairs_s=t_pairs, het_sites_s=t_sites, samples=[])
    for rnd in range(3):                                   # the first pass loads every code object and is dropped
        acc = KmerCounts(32, device=str(dev))
        t = dict.fromkeys(CALLS, 0.0)
        tally = torch.zeros(3, dtype=torch.int64, device=dev)
        nlinks = 0
        for first, count in batches:
            b = Batch.from_device(ds.reads(first, count))
            n = P.read_links(b, mark)[0].numel()           # the size, untimed
            dt, (links, tally) = timed(dev, lambda: P.read_links(b, mark, capacity=n, tally=tally))
            t["links"] += dt
            t["add_keys"] += timed(dev, lambda: acc.add_keys(links))[0]
            t["profiles"] += timed(dev, lambda: P.profiles(b))[0]
            t["runs"] += timed(dev, lambda: P.read_runs(None, b, emit=SortedKmers.RUN_NONE))[0]
            nlinks += n
            del b, links
        leg = dict(links=dict(zip(SortedKmers.LINK_TALLY, tally.tolist())))
        for c in CALLS:
            leg[c + "_s"] = t[c]
        for c in ("links", "profiles", "runs"):
            leg[c + "_gbases_per_s"] = ds.total_bases / t[c] / 1e9
        leg["add_keys_mkeys_per_s"] = nlinks / max(t["add_keys"], 1e-9) / 1e6
        leg["ratio_to_profiles"], leg["ratio_to_runs"] = t["profiles"] / t["links"], t["runs"] / t["links"]
        leg["sort_s"], edges = timed(dev, lambda: acc.sorted(1))
        acc.close()
        leg["forest_s"], (block, side, forest) = timed(dev, lambda: phase_forest(edges, nsites, a.min_support))
        leg["forest"], leg["edge_keys"] = forest, len(edges)
        leg["forest_ns_per_key"] = leg["forest_s"] / max(len(edges), 1) * 1e9
        leg["known_kept_edges"], leg["right_kept_edges"] = edge_truth(edges, truth, a.min_support)
        edges.close()
        leg["split_s"], (A, B) = timed(dev, lambda: P.phase_split(mark, block, side))
        leg["a_entries"], leg["b_entries"] = len(A), len(B)
        A.close()
        B.close()
        sizes = torch.bincount(block)
        leg["block_n50_sites"] = n50(sizes[sizes >= 2].tolist())
        leg["scored_sites"], leg["agreeing_sites"] = score(truth, block, side)
        say("pass %d: %s" % (rnd, leg))
        if rnd:
            res["samples"].append(leg)
    t_u, U = timed(dev, lambda: P.unitigs(components=True))
    res["unitigs_components_s"], res["unitigs"] = t_u, len(U)
    U.close()
    res["value"], res["unit"] = max(s["links_gbases_per_s"] for s in res["samples"]), "Gbases/s"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tabphase, phasing heterozygous sites from reads on one MI355X: `python scripts/phase_bench.py`, one process, two\n"
                    "timed passes over all batches after one untimed pass, the four read calls interleaved batch by batch.\n\n")
            f.write("%s, K = %d: %d bases in %d sub-batches; F = KmerCounts.sorted(1) of all reads, %d entries; P = its unique pairs\n"
                    "under 5-, %d entries, %d sites (het_pairs %.3f s, het_sites %.3f s).\n"
                    % (res["config"], K, ds.total_bases, len(batches), nf, len(P), nsites, t_pairs, t_sites))
            for i, r in enumerate(res["samples"]):
                f.write("sample %d\n" % (i + 1))
                f.write("  read_links    %.2f Gbases/s (%.2f s): %.3f of profiles on P (%.2f), %.3f of read_runs in absence mode (%.2f)\n"
                        % (r["links_gbases_per_s"], r["links_s"], r["ratio_to_profiles"], r["profiles_gbases_per_s"], r["ratio_to_runs"],
                           r["runs_gbases_per_s"]))
                f.write("  add_keys      %.1f M keys/s (%.3f s); sort %.3f s, %d keys\n"
                        % (r["add_keys_mkeys_per_s"], r["add_keys_s"], r["sort_s"], r["edge_keys"]))
                f.write("  forest        %.3f s, %.1f ns per key; split %.3f s\n" % (r["forest_s"], r["forest_ns_per_key"], r["split_s"]))
                f.write("  tallies       %s; %s; A %d, B %d entries; block N50 %d sites\n"
                        % (r["links"], r["forest"], r["a_entries"], r["b_entries"], r["block_n50_sites"]))
                f.write("  truth         %d of %d scored sites agree with the generator's haplotypes, a flip per block allowed (%.4f %%)\n"
                        % (r["agreeing_sites"], r["scored_sites"], 100.0 * r["agreeing_sites"] / max(r["scored_sites"], 1)))
                f.write("                %d of %d kept edges between two scored sites carry the sign the haplotypes give (%.4f %%)\n"
                        % (r["right_kept_edges"], r["known_kept_edges"], 100.0 * r["right_kept_edges"] / max(r["known_kept_edges"], 1)))
            f.write("for scale     unitigs(components=True) on P: %.3f s, %d unitigs\n" % (t_u, res["unitigs"]))
            f.write("not measured  hardware counters, other K, a form of the marker kernel with fewer LDS cells per lane, the tabphase\n"
                    "              command on files of this scale\n")
            f.write("\nRaw JSON line:\n" + line + "\n")
    P.close()


if __name__ == "__main__":
    main()

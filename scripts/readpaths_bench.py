"""Reads threaded through the unitig graph (tabpath, cp_kmer_sorted_read_paths) on BASELINE configs[2]: one JSON line, and
with --out a text file that holds the summary and the line (profiles/readpaths_configs2.txt).

    python scripts/readpaths_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of
500 Mbases; S = `KmerCounts.sorted(1)` of all reads, K = 40.  For the graph without a count range (many short unitigs) and
with the range 5- (few long ones): the unitigs with their where arrays and links, once; then, batch by batch over ALL reads
and --rounds times after one untimed pass, the same batch goes through
  paths           read_paths, the records only
  paths+cov       the same with the coverage added
  paths+cov+sup   the same with coverage and support added
  read_runs       read_runs(S), absence mode (skip 0, every state emitted), the same range      a yardstick from before
  profiles        one cp_kmer_sorted_profiles on S                                              a yardstick from before
one after the other, each timed with a device synchronise on both sides, so the samples are interleaved.  The untimed pass
finds the number of segments of every batch, which the timed passes give as the capacity: one call per batch, as a tool
that has seen a batch of its source would make it.  Checked once, in the untimed pass, at this scale and on the device:
sum(coverage) == PRESENT and sum(support) == JOINED.  Reported: Gbases/s of each and the ratios to the two yardsticks, the
segments, joins and walks, the unitigs touched and the links crossed.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, KmerCounts, unitig_n50   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth   # noqa: E402

K = 40
RANGES = (("all", None), ("range 5-", (5, None)))
CALLS = ("paths", "paths+cov", "paths+cov+sup", "read_runs", "profiles")


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--rounds", type=int, default=2)
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
    S = T.sorted(1)
    T.close()
    say("all reads: %d entries" % len(S))
    res = dict(metric="reads threaded through the unitig graph", K=K, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, batches=len(batches), entries=len(S), graph={}, cases={})
    for name, rng in RANGES:
        t_u, U = timed(dev, lambda: S.unitigs(rng, where=True, links=True))
        lens = (U.off[1:] - U.off[:-1]).cpu()
        res["graph"][name] = dict(unitigs=len(U), links=U.nlinks, keys=U.tally["keys"], n50=unitig_n50(lens), seconds=t_u)
        say("%s: %s" % (name, res["graph"][name]))
        cov = torch.zeros(len(U), dtype=torch.int64, device=dev)
        sup = torch.zeros(U.nlinks, dtype=torch.int64, device=dev)
        scratch_cov, scratch_sup = torch.zeros_like(cov), torch.zeros_like(sup)
        caps, legs = [None] * len(batches), []
        for rnd in range(a.rounds + 1):                    # the first pass loads every code object and is dropped
            t = {c: 0.0 for c in CALLS}
            tally = dict(positions=0, present=0, absent=0, other=0, segments=0, joined=0, walks=0)
            for i, (first, count) in enumerate(batches):
                b = Batch.from_device(ds.reads(first, count))
                c_, s_ = (cov, sup) if rnd == 0 else (scratch_cov, scratch_sup)
                calls = {"paths": lambda: S.read_paths(U, b, capacity=caps[i]),
                         "paths+cov": lambda: S.read_paths(U, b, coverage=scratch_cov, capacity=caps[i]),
                         "paths+cov+sup": lambda: S.read_paths(U, b, coverage=c_, support=s_, capacity=caps[i]),
                         "read_runs": lambda: S.read_runs(None, b, a_range=rng),
                         "profiles": lambda: S.profiles(b)}
                for c in CALLS:
                    dt, out = timed(dev, calls[c])
                    t[c] += dt
                    if c == "paths+cov+sup":
                        for k in tally:
                            tally[k] += out[2][k]
                        caps[i] = out[2]["segments"]
                    del out
                del b
            if rnd == 0:
                sums_hold = int(cov.sum()) == tally["present"] and int(sup.sum()) == tally["joined"]
                touched, crossed = int((cov != 0).sum()), int((sup != 0).sum())
                say("untimed pass, %s: %s; sums hold: %s" % (name, tally, sums_hold))
                continue
            leg = {c + "_s": t[c] for c in CALLS}
            leg.update({c + "_gbases_per_s": ds.total_bases / t[c] / 1e9 for c in CALLS})
            for c in CALLS[:3]:
                leg[c + " / read_runs"] = t["read_runs"] / t[c]          # above 1: faster than the yardstick
                leg[c + " / profiles"] = t["profiles"] / t[c]
            legs.append(leg)
            say("round %d, %s: %s" % (rnd, name, leg))
        res["cases"][name] = dict(tally=tally, touched=touched, crossed=crossed, sums_hold=sums_hold, rounds=legs)
        U.close()
        del U, cov, sup, scratch_cov, scratch_sup
    res["value"], res["unit"] = min(r["paths_gbases_per_s"] for r in res["cases"]["all"]["rounds"]), "Gbases/s"
    S.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tabpath, reads threaded through the unitig graph (cp_kmer_sorted_read_paths) on one MI355X:\n"
                    "`python scripts/readpaths_bench.py`, one process, %d round(s) over all batches after one untimed pass; every\n"
                    "figure below is one sample per round, the five calls interleaved batch by batch.\n\n" % a.rounds)
            f.write("%s, K = %d: %d bases in %d sub-batches.  S = sorted(1) of all reads, %d entries.\n"
                    % (res["config"], K, ds.total_bases, len(batches), len(S) if S.s else res["entries"]))
            for name, _ in RANGES:
                g, c = res["graph"][name], res["cases"][name]
                f.write("\n%s: %d unitigs, N50 %d, %d links, %d k-mers in (%.2f s for unitigs, where arrays and links)\n"
                        % (name, g["unitigs"], g["n50"], g["links"], g["keys"], g["seconds"]))
                f.write("  %s\n" % ", ".join("%d %s" % (c["tally"][k], k) for k in c["tally"]))
                f.write("  %d of %d unitigs touched, %d of %d links crossed; sum(coverage) == PRESENT and sum(support) == JOINED: %s\n"
                        % (c["touched"], g["unitigs"], c["crossed"], g["links"], c["sums_hold"]))
                for i, r in enumerate(c["rounds"]):
                    f.write("  round %d  %s\n" % (i, ", ".join("%s %.2f" % (k, r[k + "_gbases_per_s"]) for k in CALLS) + " Gbases/s"))
                    f.write("           %s\n" % ", ".join("%s %.3f" % (k, r[k]) for k in r if " / " in k))
            f.write("\nThis is the first form of the kernels (a 64-bit word per base stored by the look-up pass, a counting pass, a\n"
                    "one-block scan and a writing pass that reads the words twice); no second form was built, so there is no\n"
                    "A/B here.  Not measured: hardware counters, other K, contigs as the source, and the tabpath command\n"
                    "itself (reading the files and writing GAF and GFA on the host) on files of this scale.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

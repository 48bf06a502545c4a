"""Runs of k-mer states along reads (tabtrack, cp_kmer_sorted_read_runs) on BASELINE configs[2]: one JSON line, and with
--out a text file that holds the summary and the line (profiles/readruns_configs2.txt).

    python scripts/readruns_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of
500 Mbases.  A = `KmerCounts.sorted(1)` of the first half of the sub-batches, B = that of the second half (the pair of
scripts/readhits_bench.py), F = A or B with the counts summed: the table of all reads.  Then, batch by batch over ALL reads
and --rounds times after one untimed pass, the same batch goes through
  phase     read_runs(A, B), skip NONE | BOTH | OTHER, emit A | B      against   read_hits(A, B)
  absence   read_runs(F), skip 0, every state emitted                  against   one cp_kmer_sorted_profiles on F
  absence   the same with the range 3- on F                            against   the same profiles call
one after the other, each timed with a device synchronise on both sides, so the samples are interleaved.  The yardsticks
are calls that existed before, on the same tables and batches.  Checked once, in the untimed pass: phase runs - 1 per read
against the switches of read_hits, and the NONE total of the absence runs against the absent cells of the profiles.
Reported per round: Gbases/s of each, the runs, and the bytes that come down (32 per run and 8 per read) against the 2
bytes per base of a profile.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, KmerCounts, SortedKmers   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth   # noqa: E402

K = 40
PHASE_SKIP = SortedKmers.RUN_NONE | SortedKmers.RUN_BOTH | SortedKmers.RUN_OTHER
RUNS = ("phase", "absence", "absence_3")
YARD = {"phase": "read_hits", "absence": "profiles", "absence_3": "profiles"}


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


def snapshot_of(ds, dev, batches):
    T = KmerCounts(K, device=str(dev))
    for first, count in batches:
        rd = ds.reads(first, count)
        T.add_tensors(rd["seq"], rd["seq_off"])
        del rd
    s = T.sorted(1)
    T.close()
    return s


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    half = len(batches) // 2
    A = snapshot_of(ds, dev, batches[:half])
    B = snapshot_of(ds, dev, batches[half:])
    F = A.combine(B, "or", count="sum")
    say("A %d entries, B %d entries, F %d entries" % (len(A), len(B), len(F)))
    res = dict(metric="runs of k-mer states along reads", K=K,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, batches=len(batches), a_entries=len(A), b_entries=len(B), f_entries=len(F), rounds=[])
    calls = {"phase": lambda b: A.read_runs(B, b, skip=PHASE_SKIP),
             "absence": lambda b: F.read_runs(None, b),
             "absence_3": lambda b: F.read_runs(None, b, a_range=(3, None)),
             "read_hits": lambda b: A.read_hits(B, b),
             "profiles": lambda b: F.profiles(b)}
    for rnd in range(a.rounds + 1):                        # the first pass loads every code object and is dropped
        t = {c: 0.0 for c in calls}
        nruns, reads, ok = {r: 0 for r in RUNS}, 0, True
        for first, count in batches:
            b = Batch.from_device(ds.reads(first, count))
            out = {}
            for c, fn in calls.items():
                dt, out[c] = timed(dev, lambda: fn(b))
                t[c] += dt
            for r in RUNS:
                nruns[r] += out[r][1]["n"].numel()
            if rnd == 0:                                   # the identities, once
                off = out["phase"][0]
                ok = ok and torch.equal((off[1:] - off[:-1] - 1).clamp(min=0), out["read_hits"][:, 4])
                tally = torch.zeros(3, dtype=torch.int64, device=dev)
                F.profiles(b, tally=tally)
                r = out["absence"][1]
                ok = ok and int(r["n"][r["state"] == 0].sum()) == int(tally[1])
            reads += b.nreads
            del b, out
        leg = dict(reads=reads)
        for c in calls:
            leg[c + "_s"], leg[c + "_gbases_per_s"] = t[c], ds.total_bases / t[c] / 1e9
        for r in RUNS:
            leg[r + "_runs"] = nruns[r]
            leg[r + "_ratio"] = t[YARD[r]] / t[r]          # above 1: faster than its yardstick
            leg[r + "_bytes_down"] = 32 * nruns[r] + 8 * (reads + len(batches))
        if rnd == 0:
            res["identities_hold"] = ok
            say("untimed pass: %s; identities hold: %s" % (leg, ok))
            continue
        res["rounds"].append(leg)
        say("round %d: %s" % (rnd, leg))
    res["value"], res["unit"] = min(r["phase_gbases_per_s"] for r in res["rounds"]), "Gbases/s"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tabtrack, runs of k-mer states along reads (cp_kmer_sorted_read_runs) on one MI355X:\n"
                    "`python scripts/readruns_bench.py`, one process, %d round(s) over all batches after one untimed pass; every\n"
                    "figure below is one sample per round, the five calls interleaved batch by batch.\n\n" % a.rounds)
            f.write("%s, K = %d: %d bases in %d sub-batches, %d reads.\n" % (res["config"], K, ds.total_bases, len(batches),
                                                                            res["rounds"][0]["reads"]))
            f.write("  A, B, F           KmerCounts.sorted(1) of the first and of the second half of the sub-batches, and A or B\n"
                    "                    with the counts summed: %d, %d and %d entries\n" % (len(A), len(B), len(F)))
            for i, r in enumerate(res["rounds"]):
                f.write("  round %d           phase read_runs(A, B) %.2f Gbases/s, read_hits(A, B) %.2f: ratio %.3f\n"
                        "                    absence read_runs(F) %.2f Gbases/s, one profiles(F) %.2f: ratio %.3f\n"
                        "                    absence read_runs(F:3-) %.2f Gbases/s: ratio %.3f\n"
                        % (i, r["phase_gbases_per_s"], r["read_hits_gbases_per_s"], r["phase_ratio"], r["absence_gbases_per_s"],
                           r["profiles_gbases_per_s"], r["absence_ratio"], r["absence_3_gbases_per_s"], r["absence_3_ratio"]))
            r = res["rounds"][-1]
            for name in RUNS:
                f.write("  %-17s %d runs, %d bytes down against %d of a profile (2 per base): %.4f of it\n"
                        % (name, r[name + "_runs"], r[name + "_bytes_down"], 2 * ds.total_bases,
                           r[name + "_bytes_down"] / (2 * ds.total_bases)))
            f.write("  identities        phase runs - 1 per read equal to the switches of read_hits, NONE total of the absence runs\n"
                    "                    equal to the absent cells of the profiles: %s\n" % res["identities_hold"])
            f.write("\nRaw JSON line:\n" + line + "\n")
    for s in (A, B, F):
        s.close()


if __name__ == "__main__":
    main()

"""The unitigs of one sorted k-mer table (tabunitig, cp_kmer_sorted_unitigs) on BASELINE configs[2]: one JSON line, and with
--out a text file that holds the summary and the line (profiles/unitig_configs2.txt).

    python scripts/unitig_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of 500
Mbases; S = `KmerCounts.sorted(1)` of all reads, K = 40.  After one untimed pass, --rounds samples, interleaved, with the
count range 5- and without it, of `unitigs` in two forms -- the adjacency pass alone (the bytes and the tally) and the whole
call (sequences, count sums, flags) -- and in the same process, on the same snapshot, the yardsticks from before this call
existed: `cp_kmer_sorted_het_pairs` with the degrees only (three to six look-ups per entry against the eight here), `S.find`
of S's own keys (one bucket search per key) and `S.compare(S)` (one streaming pass over the entries).  Every call is timed
with a device synchronise on both sides.  The jump rounds and the time they took come from the call's own tally."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import KmerCounts, _stream_of, check, unitig_n50   # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                           # noqa: E402

K = 40
RANGES = (("all", None), ("range 5-", (5, None)))


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


def degrees_only(S, deg, rng):
    r = None if rng is None else (C.c_int64 * 2)(rng[0], (1 << 63) - 1)
    check(S.L.cp_kmer_sorted_het_pairs(S.s, r, 1, 1, 1, None, None, deg.data_ptr(), _stream_of(S.device), None))


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    T = KmerCounts(K, device=str(dev))
    for first, count in ds.plan_batches(int(a.batch_mbases * 1e6)):
        rd = ds.reads(first, count)
        T.add_tensors(rd["seq"], rd["seq_off"])
        del rd
    S = T.sorted(1)
    T.close()
    say("all reads: %d entries" % len(S))
    res = dict(metric="unitigs of one sorted k-mer table", K=K, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, entries=len(S), s={}, graph={})
    hi, lo = S.hi, S.lo
    deg = torch.zeros(len(S), dtype=torch.uint8, device=dev)
    for rnd in range(a.rounds + 1):                        # interleaved; the first pass loads every code object and is dropped
        for name, rng in RANGES:
            t, A = timed(dev, lambda: S.unitigs(rng, adjacency=True, sequences=False))
            if rnd:
                res["s"].setdefault("adjacency, " + name, []).append(t)
            t, U = timed(dev, lambda: S.unitigs(rng))
            if rnd:
                res["s"].setdefault("unitigs, " + name, []).append(t)
                res["s"].setdefault("jump rounds of it, " + name, []).append(U.tally["jump_ns"] / 1e9)
                res["s"].setdefault("number of them, " + name, []).append(U.tally["rounds"])
            g = {k: v for k, v in U.tally.items() if k != "jump_ns"}
            for k in ("keys", "isolated", "tips", "branching", "arcs"):
                assert A.tally[k] == U.tally[k], (name, k)
            if rnd == 0:
                lens = U.off[1:] - U.off[:-1]
                g["n50"] = unitig_n50(lens)
                g["nodes_sum_to_keys"] = bool(int((lens - (K - 1)).sum()) == U.tally["keys"])
                g["kc_sum"] = int(U.kc.sum())
                res["graph"][name] = g
                del lens
            else:                                          # everything but the rounds is a function of the table alone
                assert all(res["graph"][name][k] == v for k, v in g.items() if k != "rounds"), name
                res["graph"][name]["rounds"] = max(res["graph"][name]["rounds"], g["rounds"])
            U.close()
            del A, U
            t, _ = timed(dev, lambda: degrees_only(S, deg, rng))
            if rnd:
                res["s"].setdefault("het_pairs degrees, " + name, []).append(t)
        t, tally = timed(dev, lambda: S.compare(S))
        if rnd:
            res["s"].setdefault("compare", []).append(t)
        t, pos = timed(dev, lambda: S.find(hi, lo))
        assert rnd or bool((pos == torch.arange(len(S), device=dev)).all())
        del pos
        if rnd:
            res["s"].setdefault("find", []).append(t)
    best = {n: min(v) for n, v in res["s"].items()}
    res["ratio"] = {}
    for name, _ in RANGES:
        adj, whole, het = best["adjacency, " + name], best["unitigs, " + name], best["het_pairs degrees, " + name]
        r = res["graph"][name]["rounds"]
        res["ratio"][name] = {"adjacency / het_pairs degrees": adj / het, "adjacency / find": adj / best["find"],
                              "adjacency / compare": adj / best["compare"], "unitigs / adjacency": whole / adj,
                              "unitigs / compare": whole / best["compare"],
                              "s per jump round": best["jump rounds of it, " + name] / max(r, 1)}
    res["value"], res["unit"] = len(S) / best["unitigs, all"] / 1e9, "G entries/s (unitigs, whole call)"
    S.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        fmt = lambda xs: ", ".join("%d" % x if isinstance(x, int) else "%.4f" % x for x in xs)
        with open(a.out, "w") as f:
            f.write("tabunitig, the unitigs of one sorted k-mer table (cp_kmer_sorted_unitigs) on one MI355X:\n"
                    "`python scripts/unitig_bench.py`, one process; every time is in seconds, one sample per round after an\n"
                    "untimed pass, the forms interleaved, all samples given.\n\n")
            f.write("%s, K = %d: %d bases.  S = sorted(1) of all reads, %d entries.\n"
                    % (res["config"], K, res["total_bases"], res["entries"]))
            for name, _ in RANGES:
                f.write("  graph, %s: %s\n" % (name, res["graph"][name]))
            f.write("\n")
            for name in res["s"]:
                f.write("  %-36s %s\n" % (name + ":", fmt(res["s"][name])))
            f.write("\n")
            for name, _ in RANGES:
                f.write("  ratios of the best samples, %s: %s\n"
                        % (name, ", ".join("%s = %.3g" % kv for kv in res["ratio"][name].items())))
            f.write("\nNot measured: other K, tables that fit the last-level cache, hardware counters, double-buffered jumping or\n"
                    "the eight searches in lock-step (the build has one form of each), closed chains at scale (this set has\n"
                    "the ones reported above), and the tabunitig command itself (reading the .ktab files and writing the\n"
                    "FASTA on the host) on files of this scale.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

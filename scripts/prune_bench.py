"""Pruning the unitig graph of one sorted k-mer table (tabclean, cp_kmer_sorted_unitig_prune) on BASELINE configs[2]: one
JSON line, and with --out a text file that holds the summary and the line (profiles/prune_configs2.txt).

    python scripts/prune_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of 500
Mbases; S = `KmerCounts.sorted(1)` of all reads, K = 40.  After one untimed pass, --rounds samples, with the count range 5-
and without it, of one `prune` call with tips = 2K on the unitigs, where array and links of one `unitigs` call, of the same
call with bubbles = 2K-1 as well, and of the whole `clean` loop with tips = 2K (at most 10 rounds) -- and in the same process,
on the same snapshot, the yardsticks: the `unitigs` call with the where arrays, the link pass (no components; the C call,
its graph kept for the prune calls) and one streaming pass, `compare` of S with itself.  Every call is timed with a device synchronise on both sides.  The graph before
and after (unitigs, N50, tip unitigs) is that of the input and of the result of `clean`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import KmerCounts, Unitigs, _stream_of, check, unitig_n50     # noqa: E402
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


def shape(U):
    """unitigs, N50 and tip unitigs of a Unitigs made with links=True."""
    return dict(keys=U.tally["keys"], unitigs=len(U), n50=unitig_n50(U.off[1:] - U.off[:-1]) if len(U) else 0,
                tip_unitigs=U.link_tally["tip_unitigs"], isolated_unitigs=U.link_tally["isolated_unitigs"])


def links(S, U, rng):
    """The link pass without components on the unitigs and where arrays of U, as tabclean makes it; U takes the graph."""
    r = None if rng is None else (C.c_int64 * 2)(rng[0], (1 << 63) - 1)
    tally, g = (C.c_int64 * len(Unitigs.LINK_TALLY))(), C.c_void_p()
    check(S.L.cp_kmer_sorted_unitig_links(S.s, r, U.u, U.utg.data_ptr(), U.at.data_ptr(), tally, 0, _stream_of(S.device), C.byref(g)))
    U._adopt_graph(g, dict(zip(Unitigs.LINK_TALLY, tally)), False)


def prune(S, U, tips, bubbles):
    """The call with a result table, as tabclean makes it; the table is closed inside the timed region."""
    out, why, t = S.prune(U, 0, tips, bubbles)
    out.close()
    return t


def clean(S, rng):
    out, tallies = S.clean(rng, 0, 2 * K, 0)
    return out, tallies


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
    res = dict(metric="pruning the unitig graph of one sorted k-mer table", K=K, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, entries=len(S), s={}, before={}, after={}, tally={}, clean={})
    for rnd in range(a.rounds + 1):                        # the first pass loads every code object and is dropped
        for name, rng in RANGES:
            keep = lambda key, t: res["s"].setdefault(key + ", " + name, []).append(t) if rnd else None
            t, U = timed(dev, lambda: S.unitigs(rng, where=True))
            keep("unitigs with where", t)
            t, _ = timed(dev, lambda: links(S, U, rng))
            keep("links", t)
            t, tt = timed(dev, lambda: prune(S, U, 2 * K, 0))
            keep("prune, tips", t)
            t, tb = timed(dev, lambda: prune(S, U, 2 * K, 2 * K - 1))
            keep("prune, tips and bubbles", t)
            t, (out, tallies) = timed(dev, lambda: clean(S, rng))
            keep("clean, tips", t)
            if rnd == 0:
                res["before"][name] = shape(U)
                res["tally"][name] = {"tips": tt, "tips and bubbles": tb}
                res["clean"][name] = tallies
                W = out.unitigs(where=True, links=True)
                res["after"][name] = shape(W)
                W.close()
                del W
                say(name, res["before"][name], res["after"][name], len(tallies), "rounds")
            else:                                          # everything is a function of the table alone
                assert res["tally"][name] == {"tips": tt, "tips and bubbles": tb} and res["clean"][name] == tallies, name
            out.close()
            U.close()
            del U, out
        t, _ = timed(dev, lambda: S.compare(S))
        if rnd:
            res["s"].setdefault("compare", []).append(t)
    best = {n: min(v) for n, v in res["s"].items()}
    res["ratio"] = {}
    for name, _ in RANGES:
        u, lk = best["unitigs with where, " + name], best["links, " + name]
        p, pb, c = best["prune, tips, " + name], best["prune, tips and bubbles, " + name], best["clean, tips, " + name]
        res["ratio"][name] = {"prune / unitigs": p / u, "prune with bubbles / unitigs": pb / u, "prune / links": p / lk,
                              "prune / compare": p / best["compare"], "clean / (unitigs + links + prune)": c / (u + lk + p),
                              "clean / rounds": c / len(res["clean"][name])}
    res["value"], res["unit"] = res["before"]["all"]["keys"] / best["prune, tips, all"] / 1e9, "G entries/s (one prune call, tips)"
    S.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        fmt = lambda xs: ", ".join("%.4f" % x for x in xs)
        with open(a.out, "w") as f:
            f.write("tabclean, pruning the unitig graph of one sorted k-mer table (cp_kmer_sorted_unitig_prune) on one MI355X:\n"
                    "`python scripts/prune_bench.py`, one process; every time is in seconds, one sample per round after an\n"
                    "untimed pass, all samples given (%d each).  tips = 2K = %d bases, bubbles = 2K-1 = %d bases.\n\n" % (a.rounds, 2 * K, 2 * K - 1))
            f.write("%s, K = %d: %d bases.  S = sorted(1) of all reads, %d entries.\n"
                    % (res["config"], K, res["total_bases"], res["entries"]))
            for name, _ in RANGES:
                f.write("  graph before, %s: %s\n" % (name, res["before"][name]))
                f.write("  one call, tips, %s: %s\n" % (name, res["tally"][name]["tips"]))
                f.write("  one call, tips and bubbles, %s: %s\n" % (name, res["tally"][name]["tips and bubbles"]))
                for r, t in enumerate(res["clean"][name]):
                    f.write("  clean (tips), %s, round %d: %s\n" % (name, r + 1, t))
                f.write("  graph after clean (tips), %s: %s\n" % (name, res["after"][name]))
            f.write("\n")
            for name in res["s"]:
                f.write("  %-46s %s\n" % (name + ":", fmt(res["s"][name])))
            f.write("\n")
            for name, _ in RANGES:
                f.write("  ratios of the best samples, %s: %s\n"
                        % (name, ", ".join("%s = %.3g" % kv for kv in res["ratio"][name].items())))
            f.write("\nA prune figure includes its allocations,\n"
                    "the mark per unitig, the pass over the entries, the scan, the result table and its release; a clean figure\n"
                    "every round's unitigs call, link pass, prune call and the host's waits.\n")
            f.write("\nNot measured: hardware counters, the registers and occupancy of the rule kernel under load, the rule's\n"
                    "loads one candidate after the other (the build has one form: in groups), other K and limits, islands, a\n"
                    "weight array, and the tabclean command itself (reading and writing the .ktab files on the host) on files\n"
                    "of this scale.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

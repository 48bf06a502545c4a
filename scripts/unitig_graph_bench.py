"""The links and components of the unitig graph of one sorted k-mer table (tabgraph, cp_kmer_sorted_unitig_links) on
BASELINE configs[2]: one JSON line, and with --out a text file that holds the summary and the line
(profiles/unitig_graph_configs2.txt).

    python scripts/unitig_graph_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of 500
Mbases; S = `KmerCounts.sorted(1)` of all reads, K = 40.  After one untimed pass, --rounds samples, with the count range 5-
and without it, of `cp_kmer_sorted_unitig_links` in two forms on the unitigs and where arrays of one `unitigs` call -- the
link pass alone (want_comp = 0: look-ups, scan, write) and with the components (want_comp = 1); the component pass is the
difference of the two -- and in the same process, on the same snapshot, the yardsticks from before this call existed: the
adjacency pass of `unitigs`, the whole `unitigs` call with the where arrays that the links read, and `S.find` of S's own
keys.  Every call is timed with a device synchronise on both sides.  The label rounds come from the call's own tally."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import KmerCounts, Unitigs, _stream_of, check      # noqa: E402
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


def links(S, U, rng, want_comp):
    """The call with a result object, as tabgraph makes it; the object is destroyed inside the timed region, as it would be
    in any use.  Returns the tally."""
    r = None if rng is None else (C.c_int64 * 2)(rng[0], (1 << 63) - 1)
    tally, g = (C.c_int64 * len(Unitigs.LINK_TALLY))(), C.c_void_p()
    check(S.L.cp_kmer_sorted_unitig_links(S.s, r, U.u, U.utg.data_ptr(), U.at.data_ptr(), tally, want_comp,
                                          _stream_of(S.device), C.byref(g)))
    S.L.cp_unitig_graph_destroy(g)
    return dict(zip(Unitigs.LINK_TALLY, tally))


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
    res = dict(metric="links and components of the unitig graph of one sorted k-mer table", K=K, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, entries=len(S), s={}, graph={})
    hi, lo = S.hi, S.lo
    for rnd in range(a.rounds + 1):                        # the first pass loads every code object and is dropped
        for name, rng in RANGES:
            t, A = timed(dev, lambda: S.unitigs(rng, adjacency=True, sequences=False))
            if rnd:
                res["s"].setdefault("adjacency, " + name, []).append(t)
            t, U = timed(dev, lambda: S.unitigs(rng, where=True))
            if rnd:
                res["s"].setdefault("unitigs with where, " + name, []).append(t)
            t0, g0 = timed(dev, lambda: links(S, U, rng, 0))
            t1, g1 = timed(dev, lambda: links(S, U, rng, 1))
            if rnd:
                res["s"].setdefault("links, " + name, []).append(t0)
                res["s"].setdefault("links and components, " + name, []).append(t1)
                res["s"].setdefault("components (difference), " + name, []).append(t1 - t0)
                res["s"].setdefault("label rounds, " + name, []).append(g1["rounds"])
            assert all(g0[k] == g1[k] for k in ("links", "dead_ends", "tip_unitigs", "isolated_unitigs", "self")), name
            assert g1["links"] == U.tally["arcs"] - 2 * (U.tally["keys"] - U.tally["unitigs"]), name
            g = dict({k: v for k, v in g1.items() if k != "rounds"}, unitigs=len(U), keys=U.tally["keys"])
            if rnd == 0:
                res["graph"][name] = g
            else:                                          # everything but the rounds is a function of the table alone
                assert res["graph"][name] == g, name
            U.close()
            del A, U
        t, pos = timed(dev, lambda: S.find(hi, lo))
        del pos
        if rnd:
            res["s"].setdefault("find", []).append(t)
    best = {n: min(v) for n, v in res["s"].items()}
    res["ratio"] = {}
    for name, _ in RANGES:
        lk, both, adj = best["links, " + name], best["links and components, " + name], best["adjacency, " + name]
        res["ratio"][name] = {"links / adjacency": lk / adj, "links / find": lk / best["find"],
                              "links and components / adjacency": both / adj,
                              "links and components / unitigs with where": both / best["unitigs with where, " + name],
                              "s per label round": (both - lk) / max(best["label rounds, " + name], 1)}
    res["value"], res["unit"] = res["graph"]["all"]["unitigs"] / best["links and components, all"] / 1e6, "M unitigs/s (links and components)"
    S.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        fmt = lambda xs: ", ".join("%d" % x if isinstance(x, int) else "%.4f" % x for x in xs)
        with open(a.out, "w") as f:
            f.write("tabgraph, the links and components of the unitig graph of one sorted k-mer table\n"
                    "(cp_kmer_sorted_unitig_links) on one MI355X: `python scripts/unitig_graph_bench.py`, one process; every\n"
                    "time is in seconds, one sample per round after an untimed pass, all samples given (%d each).\n\n" % a.rounds)
            f.write("%s, K = %d: %d bases.  S = sorted(1) of all reads, %d entries.\n"
                    % (res["config"], K, res["total_bases"], res["entries"]))
            for name, _ in RANGES:
                f.write("  graph, %s: %s\n" % (name, res["graph"][name]))
            f.write("\n")
            for name in res["s"]:
                f.write("  %-40s %s\n" % (name + ":", fmt(res["s"][name])))
            f.write("\n")
            for name, _ in RANGES:
                f.write("  ratios of the best samples, %s: %s\n"
                        % (name, ", ".join("%s = %.3g" % kv for kv in res["ratio"][name].items())))
            f.write("\nThe link pass makes 8 look-ups per unitig where the adjacency pass makes 8 per k-mer; both figures above\n"
                    "include their allocations, the link pass also the scan, the write and the host's waits.\n")
            f.write("\nNot measured: the four searches of an end in lock-step (the build has one form: one after the other),\n"
                    "other K, closed chains at scale (this set has none), hardware counters, and the tabgraph command itself\n"
                    "(reading the .ktab files and writing the GFA on the host) on files of this scale.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

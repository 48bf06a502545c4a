"""The heterozygous k-mer pairs of one sorted k-mer table (tabhet, cp_kmer_sorted_het_pairs) on BASELINE configs[2]: one JSON
line, and with --out a text file that holds the summary and the line (profiles/hetpairs_configs2.txt).

    python scripts/hetpairs_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of 500
Mbases; S = `KmerCounts.sorted(1)` of all reads, K = 40.  After one untimed pass, --rounds samples, interleaved, of
`het_pairs` in four forms -- the matrix only, with the degrees, with the result table, with the count range 5- -- and of the
matrix only with CLASSPRO_HET_LDS=0 (every cell straight to device memory by a 64-bit atomic) and of the matrix and the
table with CLASSPRO_HET_STAGE=1 (a block's tile in LDS; every other form runs with it set to 0); and in the same process, on
the same snapshot, the two yardsticks: `S.compare(S)`, one streaming pass over the entries (the floor), and `S.find` of S's
own keys, one bucket search per key.  Every call is timed with a device synchronise on both sides.  The two forms of the
matrix must agree.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import KmerCounts          # noqa: E402
from classpro_amd.synth_dev import DeviceSynth   # noqa: E402

K = 40
XMAX = YMAX = 300
KNOB = "CLASSPRO_HET_LDS"
STAGE = "CLASSPRO_HET_STAGE"


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
    os.environ.pop(KNOB, None)
    os.environ.pop(STAGE, None)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    T = KmerCounts(K, device=str(dev))
    for first, count in ds.plan_batches(int(a.batch_mbases * 1e6)):
        rd = ds.reads(first, count)
        T.add_tensors(rd["seq"], rd["seq_off"])
        del rd
    S = T.sorted(1)
    T.close()
    say("all reads: %d entries" % len(S))
    res = dict(metric="heterozygous k-mer pairs of one sorted k-mer table", K=K, xmax=XMAX, ymax=YMAX, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, entries=len(S), s={})
    FORMS = [("matrix", {}, {}), ("matrix + degrees", dict(degrees=True), {}), ("matrix + table", dict(table=True), {}),
             ("matrix, range 5-", dict(count_range=(5, None)), {}), ("matrix, %s=0" % KNOB, {}, {KNOB: "0"}),
             ("matrix, %s=1" % STAGE, {}, {STAGE: "1"}), ("matrix + table, %s=1" % STAGE, dict(table=True), {STAGE: "1"})]
    keep = {}
    hi, lo = S.hi, S.lo
    for rnd in range(a.rounds + 1):                        # interleaved; the first pass loads every code object and is dropped
        for name, kw, env in FORMS:
            os.environ.pop(KNOB, None)
            os.environ[STAGE] = "0"
            os.environ.update(env)
            t, out = timed(dev, lambda: S.het_pairs(XMAX, YMAX, True, **kw))
            os.environ.pop(KNOB, None)
            os.environ.pop(STAGE, None)
            if len(out) > 2 and not isinstance(out[2], torch.Tensor):
                res["out_entries"] = len(out[2])
                out[2].close()
            assert name not in keep or (np.array_equal(keep[name][0], out[0]) and keep[name][1] == out[1]), name
            keep[name] = out[:2]
            del out
            if rnd:
                res["s"].setdefault(name, []).append(t)
        t, tally = timed(dev, lambda: S.compare(S))
        if rnd:
            res["s"].setdefault("compare", []).append(t)
        t, pos = timed(dev, lambda: S.find(hi, lo))
        assert rnd or bool((pos == torch.arange(len(S), device=dev)).all())
        del pos
        if rnd:
            res["s"].setdefault("find", []).append(t)
    mat, tal = keep["matrix"]
    res["tally"] = tal
    res["tally_range_5"] = keep["matrix, range 5-"][1]
    res["forms_agree"] = bool(np.array_equal(mat, keep["matrix, %s=0" % KNOB][0]) and np.array_equal(mat, keep["matrix + table"][0])
                              and np.array_equal(mat, keep["matrix, %s=1" % STAGE][0])
                              and np.array_equal(mat, keep["matrix + degrees"][0]))
    res["matrix_sums_to_unique"] = bool(int(mat.sum()) == tal["unique"])
    res["largest_cells"] = [[int(i) // (YMAX + 1), int(i) % (YMAX + 1), int(mat.reshape(-1)[i])]
                            for i in np.argsort(mat.reshape(-1))[::-1][:6]]
    m5 = keep["matrix, range 5-"][0]
    res["largest_cells_range_5"] = [[int(i) // (YMAX + 1), int(i) % (YMAX + 1), int(m5.reshape(-1)[i])]
                                    for i in np.argsort(m5.reshape(-1))[::-1][:6]]
    res["pairs_in_corner"] = int(mat[:32, :96].sum())
    best = {n: min(v) for n, v in res["s"].items()}
    res["ratio_to_compare"] = {n: best[n] / best["compare"] for n in best if n not in ("compare", "find")}
    res["ratio_to_find"] = {n: best[n] / best["find"] for n in best if n not in ("compare", "find")}
    res["value"], res["unit"] = len(S) / best["matrix"] / 1e9, "G entries/s (het_pairs, matrix only)"
    S.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        fmt = lambda xs: ", ".join("%.4f" % x for x in xs)
        with open(a.out, "w") as f:
            f.write("tabhet, the heterozygous k-mer pairs of one sorted k-mer table (cp_kmer_sorted_het_pairs) on one MI355X:\n"
                    "`python scripts/hetpairs_bench.py`, one process; every time is in seconds, one sample per round after an\n"
                    "untimed pass, the forms interleaved, all samples given.\n\n")
            f.write("%s, K = %d: %d bases.  S = sorted(1) of all reads, %d entries.  xmax = ymax = %d, unique pairs.\n"
                    % (res["config"], K, res["total_bases"], res["entries"], XMAX))
            f.write("  tally: %s\n  tally with range 5-: %s\n" % (tal, res["tally_range_5"]))
            f.write("  the matrix sums to the unique pairs: %s; pairs in the on-chip corner (a < 32, b < 96): %d\n"
                    % (res["matrix_sums_to_unique"], res["pairs_in_corner"]))
            f.write("  largest cells (a, b, pairs): %s\n  largest cells with range 5-: %s\n"
                    % (res["largest_cells"], res["largest_cells_range_5"]))
            f.write("  entries of the result table: %s; every form gives the same matrix: %s\n\n"
                    % (res.get("out_entries"), res["forms_agree"]))
            for name in [n for n in res["s"] if n not in ("compare", "find")]:
                f.write("  het_pairs %-28s %s   best / best compare = %.2f, / best find = %.2f\n"
                        % (name + ":", fmt(res["s"][name]), res["ratio_to_compare"][name], res["ratio_to_find"][name]))
            f.write("  compare(S, S), one streaming pass:     %s\n" % fmt(res["s"]["compare"]))
            f.write("  find of S's own keys:                  %s\n" % fmt(res["s"]["find"]))
            f.write("\nNot measured: other K, tables that fit the last-level cache, hardware counters, and the tabhet command\n"
                    "itself (reading the .ktab files on the host) on files of this scale.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

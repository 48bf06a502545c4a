"""The 2-D count comparison of two sorted k-mer tables (tabcmp, cp_kmer_sorted_compare_hist) on BASELINE configs[2]: one JSON
line, and with --out a text file that holds the summary and the line (profiles/cmphist_configs2.txt).

    python scripts/cmphist_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of 500
Mbases; A = `KmerCounts.sorted(1)` of the first half of the sub-batches, B = that of the second half, K = 40, the pair
"halves" of scripts/setop_bench.py.  After one untimed pass, --rounds samples, interleaved, of: `compare_hist` with weight
"keys" and with weight "a" at xmax = ymax = 300; the same two with CLASSPRO_CMP_LDS=0 (every cell straight to device memory
by a 64-bit atomic); and the tally-only `A.compare(B)`, the yardstick: it reads the same bytes and does the same searches.
Every call is timed with a device synchronise on both sides.  The two forms must give the same matrices, and column 0, row
0 and the rest of the keys matrix must be the tally.
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


def sorted_of(ds, dev, batches):
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
    for name in ("CLASSPRO_CMP_LDS", "CLASSPRO_CMP_GRID"):
        os.environ.pop(name, None)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    half = len(batches) // 2
    A = sorted_of(ds, dev, batches[:half])
    say("first half: %d entries" % len(A))
    B = sorted_of(ds, dev, batches[half:])
    say("second half: %d entries" % len(B))
    res = dict(metric="2-D count comparison of two sorted k-mer tables", K=K, xmax=XMAX, ymax=YMAX, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, a_entries=len(A), b_entries=len(B),
               s={})
    KNOBS = ("CLASSPRO_CMP_LDS",)
    FORMS = [("keys", "keys", {}), ("a", "a", {}), ("keys, CLASSPRO_CMP_LDS=0", "keys", {"CLASSPRO_CMP_LDS": "0"}),
             ("a, CLASSPRO_CMP_LDS=0", "a", {"CLASSPRO_CMP_LDS": "0"})]
    mats = {}
    for rnd in range(a.rounds + 1):                        # interleaved; the first pass loads every code object and is dropped
        for name, w, env in FORMS:
            for kn in KNOBS:
                os.environ.pop(kn, None)
            os.environ.update(env)
            t, m = timed(dev, lambda: A.compare_hist(B, XMAX, YMAX, w))
            assert w not in mats or np.array_equal(mats[w], m), name
            mats[w] = m
            mats[name] = m
            if rnd:
                res["s"].setdefault(name, []).append(t)
        for kn in KNOBS:
            os.environ.pop(kn, None)
        t, tally = timed(dev, lambda: A.compare(B))
        if rnd:
            res["s"].setdefault("compare", []).append(t)
    keys = mats["keys"]
    res["tally"] = list(tally)
    res["forms_agree"] = bool(np.array_equal(keys, mats["keys, CLASSPRO_CMP_LDS=0"])
                              and np.array_equal(mats["a"], mats["a, CLASSPRO_CMP_LDS=0"]))
    res["keys_matrix_is_tally"] = bool((int(keys[:, 0].sum()), int(keys[0, :].sum()), int(keys[1:, 1:].sum())) == tuple(tally))
    res["nonzero_cells"] = int((keys != 0).sum())
    res["largest_cells"] = [[int(i) // (YMAX + 1), int(i) % (YMAX + 1), int(keys.reshape(-1)[i])]
                            for i in np.argsort(keys.reshape(-1))[::-1][:6]]
    res["keys_in_corner"] = int(keys[:32, :96].sum())
    res["a_weight_total"] = int(mats["a"].sum())
    best = {n: min(v) for n, v in res["s"].items()}
    res["ratio_to_compare"] = {n: best[n] / best["compare"] for n in best if n != "compare"}
    res["value"], res["unit"] = (len(A) + len(B)) / best["keys"] / 1e9, "G operand entries/s (compare_hist, keys)"
    A.close()
    B.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        fmt = lambda xs: ", ".join("%.4f" % x for x in xs)
        with open(a.out, "w") as f:
            f.write("tabcmp, the 2-D count comparison of two sorted k-mer tables (cp_kmer_sorted_compare_hist) on one MI355X:\n"
                    "`python scripts/cmphist_bench.py`, one process; every time is in seconds, one sample per round after an\n"
                    "untimed pass, the forms interleaved, all samples given.\n\n")
            f.write("%s, K = %d: %d bases.  A = sorted(1) of the first half of the reads, %d entries; B = that of the second\n"
                    "half, %d entries.  xmax = ymax = %d.\n" % (res["config"], K, res["total_bases"], res["a_entries"],
                                                                 res["b_entries"], XMAX))
            f.write("  only in A / only in B / in both: %s; the keys matrix sums to it: %s\n"
                    % (" / ".join(str(x) for x in tally), res["keys_matrix_is_tally"]))
            f.write("  non-zero cells %d; keys in the on-chip corner (x < 32, y < 96): %d of %d; largest cells (x, y, keys): %s\n"
                    % (res["nonzero_cells"], res["keys_in_corner"], int(keys.sum()), res["largest_cells"]))
            f.write("  both forms give the same matrices: %s\n\n" % res["forms_agree"])
            for name in [n for n in res["s"] if n != "compare"]:
                f.write("  compare_hist %-26s %s   best / best compare = %.2f\n"
                        % (name + ":", fmt(res["s"][name]), res["ratio_to_compare"][name]))
            f.write("  compare (tally only):                   %s\n" % fmt(res["s"]["compare"]))
            f.write("\nNot measured: other shapes of the matrix and of the on-chip corner, other grids, tables that fit the\n"
                    "last-level cache, K <= 31 (the form without hi[]), an assembly against reads, and the tabcmp command\n"
                    "itself (reading the .ktab files on the host) on files of this scale.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

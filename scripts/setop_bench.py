"""Set algebra on sorted k-mer tables (tabop, cp_kmer_sorted_combine / cp_kmer_sorted_hist) on BASELINE configs[2]: one
JSON line, and with --out a text file that holds the summary and the line (profiles/setop_configs2.txt).

    python scripts/setop_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) in sub-batches of
500 Mbases.  Pair "halves": A = `KmerCounts.sorted(1)` of the first half of the sub-batches, B = that of the second half
(mostly shared: the genome's k-mers are in both, the error k-mers in one).  Pair "genome": A = `sorted(2)` of all reads, B =
`sorted(1)` of the synthesiser's two haplotypes (mostly shared as well, with the surviving error k-mers on A's side only).
Pair "disjoint": A = the k-mers seen once in the first half (`halves.A` with the range 1-1), B = the genome's table
(mostly disjoint).  For each pair, after one untimed pass, --rounds samples of: every set_op with LEFT, OR with SUM,
`compare` alone, `hist` of A; each call timed with a device synchronise on both sides.  Beside them three yardsticks taken
in the same process: (1) cp_kmer_counts_sort(1) of the tables the operands came from, (2) cp_kmer_sorted_find of all of A's
keys in B, which is what AND and SUB membership costs with the calls that existed before, (3) the bytes the two passes read
and write (24 per operand entry twice, 24 per result entry once) divided by the rate of a plain device-to-device copy.
The identity `or/sum of the two halves == sorted(1) of the whole` is checked on keys, counts and index.  K = 40 has hi bits,
so the hi-free form of the kernels (2K <= 63) is timed on a pair of K = 31 tables of the first two sub-batches, against the
general form forced by CLASSPRO_SETOP_HI=1, and the two forms of the result's bucket counters (CLASSPRO_SETOP_ATOMICS=run|entry)
on or/sum of the halves.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import KmerCounts          # noqa: E402
from classpro_amd.synth_dev import DeviceSynth   # noqa: E402

K = 40
CASES = (("and", "left"), ("or", "left"), ("sub", "left"), ("xor", "left"), ("or", "sum"))


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


def table_of(ds, dev, batches, k):
    T = KmerCounts(k, device=str(dev))
    for first, count in batches:
        rd = ds.reads(first, count)
        T.add_tensors(rd["seq"], rd["seq_off"])
        del rd
    return T


def genome_table(ds, dev, k, piece=100_000_000):
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    T = KmerCounts(k, device=str(dev))
    for shift in (0, 2):
        h = acgt[((ds.gen >> shift) & 3).long()]
        for s in range(0, h.numel() - (k - 1), piece):
            x = h[s:s + piece + k - 1]
            T.add_tensors(x, torch.tensor([0, x.numel()], dtype=torch.int64, device=dev))
        del h
    return T


def measure(dev, name, A, B, rounds, copy_rate, a_range=None):
    """The samples of one pair; every result is closed as soon as it is timed."""
    out = dict(pair=name, a_entries=len(A), b_entries=len(B), a_range=a_range, ops={}, compare_s=[], hist_s=[], find_s=[])
    for rnd in range(rounds + 1):                          # the first pass loads every code object and is dropped
        for op, rule in CASES:
            t, r = timed(dev, lambda: A.combine(B, op, rule, a_range))
            cell = out["ops"].setdefault("%s/%s" % (op, rule), dict(s=[], tally=list(r.tally)))
            nbytes = 48 * (len(A) + len(B)) + 24 * len(r)
            cell["bytes"], cell["copy_floor_s"] = nbytes, nbytes / copy_rate
            r.close()
            if rnd:
                cell["s"].append(t)
        t, tally = timed(dev, lambda: A.compare(B, a_range))
        out["compare_tally"] = list(tally)
        t2, _ = timed(dev, lambda: A.hist())
        t3, pos = timed(dev, lambda: B.find(A.hi, A.lo))
        out["find_hits"] = int((pos >= 0).sum())
        del pos
        if rnd:
            out["compare_s"].append(t)
            out["hist_s"].append(t2)
            out["find_s"].append(t3)
    say(name, json.dumps(out))
    return out


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    os.environ.pop("CLASSPRO_SETOP_HI", None)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    half = len(batches) // 2
    res = dict(metric="set algebra on sorted k-mer tables", K=K, rounds=a.rounds,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=ds.total_bases, batches=len(batches), sort_s={}, pairs=[])

    # the rate of a plain device-to-device copy: bytes read plus bytes written per second
    buf = torch.empty(1 << 30, dtype=torch.int64, device=dev)
    dst = torch.empty_like(buf)
    dst.copy_(buf)
    res["copy_s"] = [timed(dev, lambda: dst.copy_(buf))[0] for _ in range(3)]
    copy_rate = 2 * buf.numel() * 8 / min(res["copy_s"])
    res["copy_bytes_per_s"] = copy_rate
    del buf, dst
    say("device-to-device copy: %.0f GB/s read + written" % (copy_rate / 1e9))

    def snapshot(name, T, min_count=1):
        T.sorted(min_count).close()                        # untimed: the code objects and the allocator
        ts = []
        for _ in range(a.rounds):
            t, s = timed(dev, lambda: T.sorted(min_count))
            ts.append(t)
            if len(ts) < a.rounds:
                s.close()
        res["sort_s"][name] = dict(entries=len(s), s=ts)
        say("sorted %s: %d entries, %s s" % (name, len(s), ts))
        return s

    T = table_of(ds, dev, batches[:half], K)
    A = snapshot("first half", T)
    T.close()
    T = table_of(ds, dev, batches[half:], K)
    B = snapshot("second half", T)
    T.close()
    res["pairs"].append(measure(dev, "halves", A, B, a.rounds, copy_rate))
    atom = dict(run=[], entry=[])                          # the bucket counters: per run of a bucket in a tile, or per entry
    for rnd in range(a.rounds + 1):                        # interleaved; the first pass is dropped
        for form in atom:
            os.environ["CLASSPRO_SETOP_ATOMICS"] = form
            t, r = timed(dev, lambda: A.combine(B, "or", "sum"))
            r.close()
            if rnd:
                atom[form].append(t)
    os.environ.pop("CLASSPRO_SETOP_ATOMICS", None)
    res["bucket_atomics_or_sum_halves_s"] = atom
    say("bucket atomics:", json.dumps(atom))
    T = table_of(ds, dev, batches, K)
    W = snapshot("all reads", T)
    W2 = snapshot("all reads, min_count 2", T, 2)
    T.close()
    u = A.combine(B, "or", "sum")
    (_, iu), (_, iw) = u.ktab(0, 0), W.ktab(0, 0)
    res["identity_or_sum_of_halves_is_whole"] = bool(len(u) == len(W) and torch.equal(u.hi, W.hi) and torch.equal(u.lo, W.lo)
                                                     and torch.equal(u.counts, W.counts) and torch.equal(iu, iw))
    say("or/sum of the halves == sorted(1) of the whole:", res["identity_or_sum_of_halves_is_whole"])
    u.close()
    W.close()
    del iu, iw
    T = genome_table(ds, dev, K)
    G = snapshot("genome", T)
    T.close()
    res["pairs"].append(measure(dev, "genome", W2, G, a.rounds, copy_rate))
    res["pairs"].append(measure(dev, "disjoint", A, G, a.rounds, copy_rate, a_range=(1, 1)))
    for s in (A, B, W2, G):
        s.close()

    # the hi-free form against the general one, K = 31
    T = table_of(ds, dev, batches[:1], 31)
    A31 = T.sorted(1)
    T.close()
    T = table_of(ds, dev, batches[1:2], 31)
    B31 = T.sorted(1)
    T.close()
    forms = dict(a_entries=len(A31), b_entries=len(B31), lo_only_s=[], with_hi_s=[], lo_only_compare_s=[], with_hi_compare_s=[])
    for rnd in range(a.rounds + 2):                        # interleaved; the first pass is dropped
        for form, knob in (("lo_only", "0"), ("with_hi", "1")):
            os.environ["CLASSPRO_SETOP_HI"] = knob
            t, r = timed(dev, lambda: A31.combine(B31, "or", "sum"))
            forms["out_entries"] = len(r)
            r.close()
            t2, _ = timed(dev, lambda: A31.compare(B31))
            if rnd:
                forms[form + "_s"].append(t)
                forms[form + "_compare_s"].append(t2)
    os.environ.pop("CLASSPRO_SETOP_HI", None)
    res["k31_forms"] = forms
    say("K = 31 forms:", json.dumps(forms))
    A31.close()
    B31.close()

    halves = res["pairs"][0]
    res["value"], res["unit"] = (halves["a_entries"] + halves["b_entries"]) / min(halves["ops"]["or/sum"]["s"]) / 1e9, \
        "G operand entries/s (or/sum of the halves)"
    line = json.dumps(res)
    print(line)
    if a.out:
        fmt = lambda xs: ", ".join("%.4f" % x for x in xs)
        with open(a.out, "w") as f:
            f.write("tabop, set algebra on sorted k-mer tables (cp_kmer_sorted_combine, cp_kmer_sorted_hist) on one MI355X:\n"
                    "`python scripts/setop_bench.py`, one process; every time is in seconds, one sample per round after an\n"
                    "untimed pass, all samples given.\n\n")
            f.write("%s, K = %d: %d bases in %d sub-batches.\n" % (res["config"], K, res["total_bases"], len(batches)))
            f.write("  device-to-device copy of 8 GiB: %s s -> %.0f GB/s read + written\n" % (fmt(res["copy_s"]), copy_rate / 1e9))
            for name, srt in res["sort_s"].items():
                f.write("  cp_kmer_counts_sort, %-24s %d entries: %s\n" % (name + ":", srt["entries"], fmt(srt["s"])))
            f.write("  or/sum of the two halves == sorted(1) of all reads (keys, counts, index): %s\n"
                    % res["identity_or_sum_of_halves_is_whole"])
            for p in res["pairs"]:
                f.write("\npair %s: A %d entries%s, B %d entries; only in A / only in B / in both: %s\n"
                        % (p["pair"], p["a_entries"], " (count range %d-%d)" % tuple(p["a_range"]) if p["a_range"] else "",
                           p["b_entries"], " / ".join(str(x) for x in p["compare_tally"])))
                for op, c in p["ops"].items():
                    f.write("  %-9s %s   out %d entries, %d bytes moved, at the copy's rate %.4f\n"
                            % (op, fmt(c["s"]), c["tally"][3], c["bytes"], c["copy_floor_s"]))
                f.write("  compare   %s   (first pass alone: reads 24 bytes per operand entry, at the copy's rate %.4f)\n"
                        % (fmt(p["compare_s"]), 24 * (p["a_entries"] + p["b_entries"]) / copy_rate))
                f.write("  hist of A %s\n" % fmt(p["hist_s"]))
                f.write("  cp_kmer_sorted_find of A's keys in B: %s   (%d found)\n" % (fmt(p["find_s"]), p["find_hits"]))
            f.write("\nbucket counters of the result, or/sum of the halves: per run of a bucket in a tile %s   per entry %s\n"
                    % (fmt(res["bucket_atomics_or_sum_halves_s"]["run"]), fmt(res["bucket_atomics_or_sum_halves_s"]["entry"])))
            k = res["k31_forms"]
            f.write("\nK = 31, first sub-batch against the second (%d and %d entries, or/sum gives %d):\n"
                    "  hi-free form   combine %s   compare %s\n  general form   combine %s   compare %s\n"
                    % (k["a_entries"], k["b_entries"], k["out_entries"], fmt(k["lo_only_s"]), fmt(k["lo_only_compare_s"]),
                       fmt(k["with_hi_s"]), fmt(k["with_hi_compare_s"])))
            f.write("\nNot measured: the tabop command itself (reading and writing the .ktab files on the host), tables\n"
                    "larger than one GPU's memory, more than one GPU, other tile sizes, the cuts found inside the tile\n"
                    "kernel instead of a kernel of their own, a one-pass form that keeps 24 bytes per operand entry.\n")
            f.write("\nRaw JSON line:\n" + line + "\n")


if __name__ == "__main__":
    main()

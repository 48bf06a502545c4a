"""Lookups in a sorted k-mer table (tab2prof, cp_kmer_sorted_profiles / cp_kmer_sorted_load_*) on BASELINE configs[2]:
one JSON line, and with --out a text file that holds the summary and the line (profiles/tabprof_configs2.txt).

    python scripts/tabprof_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--rounds 2] [--out FILE]

One process.  The 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) and added to a
count table in sub-batches of 500 Mbases; `KmerCounts.sorted(1)` is the snapshot.  Then, batch by batch and --rounds times
over all batches, the same batch goes through cp_kmer_counts_profiles on the hash table the snapshot came from and through
cp_kmer_sorted_profiles on the snapshot in four forms -- 1, 2 and 4 searches of a lane in lock-step
(CLASSPRO_TABPROF_LOCKSTEP), and one search at a time with interpolated first probes (CLASSPRO_TABPROF_INTERP) -- one
after the other, each call timed with a device synchronise on both sides; the cells of every form are compared with the
hash table's.  Reported per round: Gbases/s of each.  Load: the snapshot's records are encoded and brought to the host,
then `SortedKmers.from_records` is timed from host memory (upload in pieces of 4 M entries, decode, check) and from
device memory (decode and check alone); the loaded arrays are compared with the snapshot's.  Device bytes of the table and
of the snapshot come from their own statistics.
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
from classpro_amd.synth_dev import DeviceSynth                # noqa: E402

K = 40
KNOBS = ("CLASSPRO_TABPROF_LOCKSTEP", "CLASSPRO_TABPROF_INTERP")
VARIANTS = {"lockstep1": (1, 0), "lockstep1_interp": (1, 1), "lockstep2": (2, 0), "lockstep4": (4, 0)}


def choose(name):
    for knob, v in zip(KNOBS, VARIANTS[name]):
        os.environ[knob] = str(v)


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
    for knob in KNOBS:
        os.environ.pop(knob, None)
    ds = DeviceSynth(genome_len=int(a.genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    batches = ds.plan_batches(int(a.batch_mbases * 1e6))
    T = KmerCounts(K, device=str(dev))
    bases = 0
    for first, count in batches:
        b = Batch.from_device(ds.reads(first, count))
        T.add(b)
        bases += b.total_bases
        del b
    st = T.stats()
    t_sort, s = timed(dev, lambda: T.sorted(1))
    say("table built: %d distinct keys, sorted in %.3f s" % (st["n_distinct"], t_sort))
    res = dict(metric="profiles relative to a sorted k-mer table", K=K,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome,
               total_bases=bases, batches=len(batches), distinct=st["n_distinct"], entries=len(s), slots=st["slots"],
               table_bytes=st["bytes"], snapshot_bytes=s.nbytes, sort_s=t_sort, rounds=[])

    # ---- profiles: the hash table and the snapshot on the same batches ----
    for rnd in range(a.rounds):
        t_hash, t_var, cells, same = 0.0, {g: 0.0 for g in VARIANTS}, 0, True
        tally = torch.zeros(3, dtype=torch.int64, device=dev)
        for first, count in batches:
            b = Batch.from_device(ds.reads(first, count))
            if rnd == 0 and first == 0:                    # every code object loaded before anything is timed
                T.profiles(b)
                for g in VARIANTS:
                    choose(g)
                    s.profiles(b)
            t, p = timed(dev, lambda: T.profiles(b))
            t_hash += t
            want = p.view(torch.int16).clone()
            for g in VARIANTS:
                choose(g)
                t, p = timed(dev, lambda: s.profiles(b, tally=tally if g == "lockstep1" else None))
                t_var[g] += t
                same = same and torch.equal(p.view(torch.int16), want)
            cells += b.total_kmers
            del b, want, p
        leg = dict(hash_s=t_hash, hash_gbases_per_s=bases / t_hash / 1e9, cells=cells, cells_equal=same,
                   tally=tally.tolist())
        for g in VARIANTS:
            leg["sorted_%s_s" % g] = t_var[g]
            leg["sorted_%s_gbases_per_s" % g] = bases / t_var[g] / 1e9
        res["rounds"].append(leg)
        say("round %d: %s" % (rnd, leg))
    for knob in KNOBS:                                     # the load and whatever follows run the build's own form
        os.environ.pop(knob, None)

    # ---- load: the snapshot's own records ----
    rec, idx = s.ktab()
    pbyte = rec.numel() // max(len(s), 1)
    h_rec, h_idx = rec.cpu().numpy(), idx.cpu().numpy()
    load = dict(record_bytes=pbyte, records_total_bytes=int(rec.numel()), piece_entries=1 << 22)
    for name, src in (("host", h_rec), ("device", rec)):
        t, L = timed(dev, lambda: SortedKmers.from_records(K, h_idx, src, device=str(dev), piece=1 << 22))
        ok = len(L) == len(s) and torch.equal(L.hi, s.hi) and torch.equal(L.lo, s.lo) \
            and torch.equal(L.counts, s.counts.clamp(max=32767))
        load["from_%s_s" % name] = t
        load["from_%s_entries_per_s" % name] = len(s) / t
        load["from_%s_equal" % name] = ok
        L.close()
        say("load from %s memory: %.3f s, equal %s" % (name, t, ok))
    res["load"] = load
    best = max(VARIANTS, key=lambda g: min(r["sorted_%s_gbases_per_s" % g] for r in res["rounds"]))
    res["value"], res["unit"], res["variant"] = min(r["sorted_%s_gbases_per_s" % best] for r in res["rounds"]), "Gbases/s", best
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("tab2prof, lookups in a sorted k-mer table (cp_kmer_sorted_profiles, cp_kmer_sorted_load_*) on one MI355X:\n"
                    "`python scripts/tabprof_bench.py`, one process, %d round(s) over all batches; every figure below is one\n"
                    "sample per round.\n\n" % a.rounds)
            f.write("%s, K = %d: %d bases in %d sub-batches, %d distinct k-mers.\n" % (res["config"], K, bases, len(batches),
                                                                                       st["n_distinct"]))
            f.write("  device bytes      hash table %d (%d slots), sorted snapshot %d (%d entries)\n"
                    % (st["bytes"], st["slots"], s.nbytes, len(s)))
            for i, r in enumerate(res["rounds"]):
                f.write("  round %d           cp_kmer_counts_profiles %.2f Gbases/s; cp_kmer_sorted_profiles %s Gbases/s;\n"
                        "                    cells equal to the hash table's: %s\n"
                        % (i, r["hash_gbases_per_s"],
                           ", ".join("%s: %.2f" % (g, r["sorted_%s_gbases_per_s" % g]) for g in VARIANTS),
                           r["cells_equal"]))
            f.write("  load              %d records of %d bytes (%d bytes): from host memory %.3f s (upload in pieces of %d\n"
                    "                    entries, decode, check), from device memory %.3f s (decode and check); loaded\n"
                    "                    arrays equal to the snapshot's: %s, %s\n"
                    % (len(s), pbyte, rec.numel(), load["from_host_s"], 1 << 22, load["from_device_s"],
                       load["from_host_equal"], load["from_device_equal"]))
            f.write("\nRaw JSON line:\n" + line + "\n")
    s.close()
    T.close()


if __name__ == "__main__":
    main()

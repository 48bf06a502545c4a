"""Sorted k-mer table (kprof -t, cp_kmer_counts_sort / cp_kmer_sorted_ktab) on BASELINE configs[2]: one JSON line.

    python scripts/ktab_bench.py [--genome 200e6] [--cov 40] [--batch-mbases 500] [--cli-genome 25e6]
                                 [--parent-kprof PATH] [--workdir DIR] [--no-cli]

Library leg: the 8-Gbase configs[2] set is generated on the device (DeviceSynth, the set of bench.py) and added to a
count table in sub-batches of 500 Mbases.  Reported: the sort (cp_kmer_counts_sort, min_count 1 and 2) in entries/s and
seconds, the snapshot's device bytes, and the encode (cp_kmer_sorted_ktab over the whole snapshot in ranges of 16 M
entries through one buffer, the index with the first range) in entries/s; the order of the snapshot is checked on the
device (every key above the one before it) and its size against the table's statistics.

Oversize leg: 2^20 k-mers behind one 12-base prefix against 2^20 k-mers with random prefixes: what the path for a bucket
larger than a tile costs (see oversize_leg).

Command leg: a set of the same generator (--cli-genome, by default 25 Mbp at the same coverage: 1 Gbase -- the whole
configs[2] set as a FASTA file, its profiles and its table are tens of gigabytes of scratch files) is written as FASTA
under --workdir, and `kprof` runs on it three times in this process's GPU call: the kprof binary named by
--parent-kprof (a build of the parent commit; skipped when not given), this build without -t, and this build with
-t1.  Reported: the wall seconds of each, what -t1 adds over either, and the bytes of the table files.  The .hist and
.prof* files of the three runs are compared byte for byte.
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from classpro_amd.api import Batch, KmerCounts                # noqa: E402
from classpro_amd.synth_dev import DeviceSynth                # noqa: E402

K = 40
RANGE = 16 << 20


def parse():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--genome", type=float, default=200e6)
    ap.add_argument("--cov", type=float, default=40)
    ap.add_argument("--read-len", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--batch-mbases", type=float, default=500)
    ap.add_argument("--cli-genome", type=float, default=25e6)
    ap.add_argument("--parent-kprof", default=None)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--no-cli", action="store_true")
    return ap.parse_args()


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(dev, fn):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def library_leg(a, dev):
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
    hist = T.hist()[4]
    say("table built: %d distinct keys" % st["n_distinct"])
    out = dict(total_bases=bases, distinct=st["n_distinct"], slots=st["slots"], table_bytes=st["bytes"])
    for minc in (1, 2):
        t, s = timed(dev, lambda: T.sorted(minc))
        n = len(s)
        want = st["n_distinct"] - (int(hist[0]) if minc == 2 else 0)
        ordered = bool(((s.hi[1:] > s.hi[:-1]) | ((s.hi[1:] == s.hi[:-1]) & (s.lo[1:] > s.lo[:-1]))).all()) if n > 1 else True
        leg = dict(min_count=minc, entries=n, entries_expected=want, ordered=ordered, sort_s=t, sort_entries_per_s=n / t,
                   snapshot_bytes=s.nbytes)
        if minc == 1:
            pbyte = ((K + 3) >> 2) - 3 + 2
            rec = torch.empty(RANGE * pbyte, dtype=torch.uint8, device=dev)
            idx = torch.empty(1 << 24, dtype=torch.int64, device=dev)
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def encode():
                for e in range(0, n, RANGE):
                    rc = s.L.cp_kmer_sorted_ktab(s.s, e, min(RANGE, n - e), rec.data_ptr(), idx.data_ptr() if e == 0 else None,
                                                 stream)
                    assert rc == 0, rc
            t, _ = timed(dev, encode)
            leg.update(encode_s=t, encode_entries_per_s=n / t, record_bytes=pbyte, records_total_bytes=n * pbyte,
                       index_last=int(idx[-1].item()))
            del rec, idx
        s.close()
        out["min_count_%d" % minc] = leg
        say("min_count %d: %s" % (minc, leg))
    T.close()
    del ds
    torch.cuda.empty_cache()
    return out


def oversize_leg(dev, log2_entries=20):
    """The path for buckets larger than a tile: 2^20 reads of one 40-mer each, once all behind the prefix A x 12 (one
    bucket of 2^20 entries, sorted in device memory with one launch per step of the network) and once with random
    prefixes (the tile path alone); the sort of each, in seconds."""
    n = 1 << log2_entries
    acgt = torch.tensor([ord(c) for c in "ACGT"], dtype=torch.uint8, device=dev)
    off = torch.arange(n + 1, dtype=torch.int64, device=dev) * K
    out = dict(reads=n)
    for name in ("one_bucket", "random_prefixes"):
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        seq = acgt[torch.randint(0, 4, (n, K), device=dev, generator=g)]
        if name == "one_bucket":
            seq[:, :12] = ord("A")
            seq[:, -1] = ord("C")                          # the forward strand is the canonical one
        T = KmerCounts(K, device=str(dev))
        T.add_tensors(seq.reshape(-1).contiguous(), off)
        t, s = timed(dev, lambda: T.sorted())
        m = len(s)
        ordered = bool(((s.hi[1:] > s.hi[:-1]) | ((s.hi[1:] == s.hi[:-1]) & (s.lo[1:] > s.lo[:-1]))).all())
        first_bucket = int(s.ktab(0, 0)[1][0].item())
        out[name] = dict(entries=m, entries_in_first_bucket=first_bucket, ordered=ordered, sort_s=t, sort_entries_per_s=m / t)
        say("%s: %s" % (name, out[name]))
        s.close()
        T.close()
    return out


def write_fasta(a, dev, path):
    ds = DeviceSynth(genome_len=int(a.cli_genome), cov=a.cov, read_len=a.read_len, K=K, seed=a.seed, device=str(dev))
    bases = 0
    with open(path, "wb") as f:
        for first, count in ds.plan_batches(int(a.batch_mbases * 1e6)):
            rd = ds.reads(first, count)
            seq, off = rd["seq"].cpu().numpy(), rd["seq_off_h"]
            for r in range(count):
                f.write(b">r%d\n" % (first + r))
                f.write(seq[off[r]:off[r + 1]].tobytes())
                f.write(b"\n")
            bases += rd["total_bases"]
            del rd
    del ds
    torch.cuda.empty_cache()
    return bases


def outputs(d, root):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.startswith(root + ".") or f.startswith("." + root + "."):
            out[f] = os.path.join(d, f)
    return out


def same_file(p, q):
    if os.path.getsize(p) != os.path.getsize(q):
        return False
    with open(p, "rb") as f, open(q, "rb") as g:
        while True:
            x, y = f.read(1 << 24), g.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def command_leg(a, dev):
    work = tempfile.mkdtemp(prefix="ktab_bench_", dir=a.workdir)
    try:
        src = os.path.join(work, "reads.fasta")
        bases = write_fasta(a, dev, src)
        say("wrote %s: %d bases" % (src, bases))
        runs = [("this_build", os.path.join(ROOT, "classpro_amd", "kprof"), []),
                ("this_build_t1", os.path.join(ROOT, "classpro_amd", "kprof"), ["-t1"])]
        if a.parent_kprof:
            runs.insert(0, ("parent_build", a.parent_kprof, []))
        out = dict(total_bases=bases, fasta_bytes=os.path.getsize(src))
        files = {}
        for name, exe, flags in runs:
            d = os.path.join(work, name)
            os.mkdir(d)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-v"] + flags + ["-N" + os.path.join(d, "reads"), src], capture_output=True, text=True)
            out[name + "_s"] = time.perf_counter() - t0
            say("%s: %.1f s" % (name, out[name + "_s"]))
            if r.returncode != 0:
                raise RuntimeError("%s failed: %s" % (name, r.stderr))
            out[name + "_stderr"] = r.stderr.strip().split("\n")[-1]
            files[name] = outputs(d, "reads")
        tab = {f: p for f, p in files["this_build_t1"].items() if "ktab" in f}
        out["ktab_files"] = len(tab)
        out["ktab_bytes"] = sum(os.path.getsize(p) for p in tab.values())
        rest = {f: p for f, p in files["this_build_t1"].items() if "ktab" not in f}
        for name in files:
            if name != "this_build_t1":
                other = files[name]
                out["other_files_equal_" + name] = (sorted(other) == sorted(rest)
                                                    and all(same_file(other[f], rest[f]) for f in rest))
                out["t1_adds_over_%s_s" % name] = out["this_build_t1_s"] - out[name + "_s"]
        return out
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    a = parse()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = dict(metric="kprof sorted k-mer table", K=K,
               config="configs[2]" if int(a.genome) == 200_000_000 else "genome %d" % a.genome)
    res["library"] = library_leg(a, dev)
    res["oversize"] = oversize_leg(dev)
    if not a.no_cli:
        res["command"] = command_leg(a, dev)
        res["command"]["config"] = "genome %d, cov %g" % (a.cli_genome, a.cov)
    res["value"], res["unit"] = res["library"]["min_count_1"]["sort_entries_per_s"], "entries/s"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

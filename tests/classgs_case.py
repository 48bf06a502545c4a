"""Scenarios for the ClassGS tests: the evaluation scenario of tests/eval_case.py (with and without its 8-base read) as
reads.fasta, reads.fasta.gz, a Dazzler .db and a .dam, the threshold sets and the error-contract cases.  Shared by
scripts/gen_classgs_golden.py (which runs the reference's own ClassGS on them) and tests/test_classgs_host.py /
tests/test_gpu_classgs.py (which run ours), so that golden and tests are made from the same inputs."""
import gzip
import hashlib
import os

import numpy as np

import eval_case

K = eval_case.K
KINDS = ["fasta", "fasta.gz", "db", "dam"]
THRESHOLDS = [("8", "25", "60"), ("30", "10", "50"), ("0", "0", "0"), ("8", "25", "70000")]
FILES = [(7, "cell_a.fasta", "m64011_a"), (None, "cell_b.fasta", "m64011_b")]     # the .db's two source files

# (name, arguments after the program; {dir} = the error directory, which holds long.fasta + long.prof only)
ERROR_CASES = [
    ("four_arguments", ["{dir}/long", "8", "25"]),
    ("illegal_option", ["-q", "{dir}/long", "8", "25", "60"]),
    ("missing_source", ["{dir}/nope", "8", "25", "60"]),
    ("negative_threshold", ["{dir}/long", "-1", "25", "60"]),
    ("read_of_60001_bases", ["{dir}/long", "8", "25", "60"]),
    ("threshold_strings", ["{dir}/nope", "70000", "x", "12y"]),
]


def scenario_id(kind, tiny):
    return "%s_%s" % (kind.replace(".", "_"), "tiny" if tiny else "notiny")


def case_id(kind, tiny, thres):
    return "%s_%s" % (scenario_id(kind, tiny), "_".join(thres))


def build_scenario(d, kind, tiny):
    """Writes <d>/reads.<kind> (+ hidden files), reads.prof, truth.prof; returns dict(headers, seqs, profiles,
    rel_profiles): the header line ClassGS prints for every read, its bases and its counts."""
    from classpro_amd import dazz
    c = eval_case.build_case(d, lambda seqs, profs, hist: [b"N" * len(s) for s in seqs], tiny)
    names, seqs, comments = c["names"], c["seqs"], c["comments"]
    fasta = os.path.join(d, "reads.fasta")
    os.remove(os.path.join(d, "est.class"))
    if kind == "fasta" or kind == "fasta.gz":
        headers, last = [], "(null)"                     # kseq keeps the previous record's comment; none yet: "(null)"
        for n, cm in zip(names, comments):
            last = cm if cm else last
            headers.append("@%s %s" % (n, last))
        if kind == "fasta.gz":
            with open(fasta, "rb") as f, gzip.GzipFile(fasta + ".gz", "wb", mtime=0) as g:
                g.write(f.read())
            os.remove(fasta)
    else:
        os.remove(fasta)
        files = [(FILES[0][0], FILES[0][1], FILES[0][2]), (len(seqs) - FILES[0][0], FILES[1][1], FILES[1][2])]
        dam = kind == "dam"
        hdr_lines = [">%s scaffold %d" % (n, i) for i, n in enumerate(names)] if dam else None
        recs = dazz.write_db(d, "reads", seqs, files, dam=dam, hdr_lines=hdr_lines)
        headers = dazz.db_headers(files, recs, dam=dam, hdr_lines=hdr_lines)
    return dict(headers=headers, seqs=seqs, profiles=c["profiles"], rel_profiles=c["rel_profiles"])


def build_error_dir(d):
    """long.fasta: one read of 60001 bases (one more than the reference takes from a FASTX file), and its profile."""
    from classpro_amd import fastk
    rng = np.random.default_rng(60001)
    seq = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 60001)])
    with open(os.path.join(d, "long.fasta"), "wb") as f:
        f.write(b">long\n" + seq + b"\n")
    prof = rng.integers(1, 80, 60001 - K + 1).astype(np.uint16)
    h = np.zeros(32767, np.int64)
    fastk.write_fastk(d, "long", K, [prof], (1, 32767, 0, 0, h), nparts=1)


def chain_labels(counts, thres):
    """src/ClassGS.c:236-245 restated: E if c < t0, else H if c < t1, else D if c < t2, else R (plain integers)."""
    c = np.asarray(counts).astype(np.int64)
    t = [int(x) for x in thres]
    out = np.full(len(c), ord("R"), np.uint8)
    out[c < t[2]] = ord("D")
    out[c < t[1]] = ord("H")
    out[c < t[0]] = ord("E")
    return out


def parse_thresholds(strs):
    """(int)strtol(s, 0, 10) for the strings the tests use: an optional sign and leading digits, else 0."""
    out = []
    for s in strs:
        i = 1 if s[:1] in "+-" else 0
        j = i
        while j < len(s) and s[j].isdigit():
            j += 1
        v = int(s[:j]) if j > i else 0
        out.append((v + 2 ** 31) % 2 ** 32 - 2 ** 31)
    return out


def expected_class(sc, thres):
    """The bytes of reads.GS.class for a scenario by the restated chain, and the per-label character counts."""
    t = parse_thresholds(thres)
    out, counts = [], dict.fromkeys("EHDRN", 0)
    for h, s, p in zip(sc["headers"], sc["seqs"], sc["profiles"]):
        lab = np.concatenate([np.full(min(K - 1, len(s)), ord("N"), np.uint8), chain_labels(p, t)]).tobytes()
        assert len(lab) == len(s)
        for ch in "EHDRN":
            counts[ch] += lab.count(ch.encode())
        out.append(h.encode() + b"\n" + s + b"\n+\n" + lab + b"\n")
    return b"".join(out), counts


def input_sha(d):
    """sha256 over the names and contents of every file of a scenario directory (a .gz by its decompressed content,
    which does not depend on the zlib at hand); outputs (*.class) are left out."""
    h = hashlib.sha256()
    for name in sorted(os.listdir(d)):
        if name.endswith(".class"):
            continue
        h.update(name.encode() + b"\0")
        p = os.path.join(d, name)
        h.update((gzip.open(p, "rb") if name.endswith(".gz") else open(p, "rb")).read())
    return h.hexdigest()

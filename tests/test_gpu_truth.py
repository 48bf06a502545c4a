"""Relative labels (cp_kmer_counts_rel_labels, KmerCounts.rel_labels, genome2class) on a real MI355X (`-m gpu`), against
the brute-force restatement in tests/truth_oracle.py: characters, packed bytes, relative profile and counts, independence
of order and batching on either side, an empty table, growth, key and input edges, the argument contract, a 150-Mbase set
against a torch-side oracle, and the command line against the oracle, prof2class and class2acc.  Everything is integers
and bytes: the tolerance is zero."""
import gzip
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import kprof_oracle as O
import truth_oracle as TO
from conftest import ROOT

pytestmark = pytest.mark.gpu
K = 40
TOOLS = os.path.join(ROOT, "classpro_amd")
REF = os.path.join(ROOT, "oracle", "_ref")
G2C = os.path.join(TOOLS, "genome2class")


@pytest.fixture(scope="module")
def torch_dev(built):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def oracle_of(genome, seqs, k):
    rel = TO.rel_profiles(genome, seqs, k)
    labs = [TO.labels(r, len(s), k) for r, s in zip(rel, seqs)]
    return dict(rel=rel, labels=labs, counts=TO.label_counts(labs))


@pytest.fixture(scope="module")
def case(torch_dev):
    c = TO.make_case(5, K=K)
    c["want"] = oracle_of(c["genome"], c["seqs"], K)
    assert min(c["want"]["counts"]) >= 1000
    return c


def flat(torch, seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    x = b"".join(seqs)
    dev = torch.device("cuda:0")
    seq = torch.from_numpy(np.frombuffer(x, np.uint8).copy() if x else np.zeros(1, np.uint8)).to(dev)
    return seq, torch.from_numpy(off).to(dev)


def split(x, lens):
    """A flat device tensor as per-read numpy arrays."""
    p = x.cpu().numpy()
    out, o = [], 0
    for n in lens:
        out.append(p[o:o + n])
        o += n
    assert o == len(p)
    return out


def table(torch, genome_batches, k, **kw):
    from classpro_amd.api import KmerCounts
    T = KmerCounts(k, **kw)
    for b in genome_batches:
        T.add_tensors(*flat(torch, [TO.fold(g) for g in b]))
    return T


def label_reads(torch, T, seqs, k, batches=None, packed=False, counts=None):
    """Labels (bytes per read), relative profiles (arrays per read) and the counts tensor, the reads going through in
    `batches` (lists of indices; default: all at once)."""
    from classpro_amd.api import unpack_labels
    labs, prof = [None] * len(seqs), [None] * len(seqs)
    for idx in batches or [list(range(len(seqs)))]:
        b = [seqs[i] for i in idx]
        lens = [len(s) for s in b]
        out, p, counts = T.rel_labels(flat(torch, b), packed=packed, profiles=True, counts=counts)
        if packed:
            pk, pko = out
            chars = unpack_labels(pk.cpu().numpy(), pko.cpu().numpy(), lens, k)
            o = np.zeros(len(b) + 1, np.int64)
            np.cumsum(lens, out=o[1:])
            got = [chars[o[i]:o[i + 1]].tobytes() for i in range(len(b))]
        else:
            got = [x.tobytes() for x in split(out, lens)]
        pp = split(p, [max(n - (k - 1), 0) for n in lens])
        for j, i in enumerate(idx):
            labs[i], prof[i] = got[j], pp[j]
    return labs, prof, counts


def check(got, want):
    labs, prof, counts = got
    assert labs == want["labels"]
    assert len(prof) == len(want["rel"]) and all(np.array_equal(a, b) for a, b in zip(prof, want["rel"]))
    assert counts.cpu().tolist() == want["counts"]


def test_library_matches_oracle(torch_dev, case):
    from classpro_amd.api import Batch
    torch = torch_dev
    seqs, want = case["seqs"], case["want"]
    T = table(torch, [case["genome"]], K)
    before = (T.stats(), T.hist())
    check(label_reads(torch, T, seqs, K), want)
    check(label_reads(torch, T, seqs, K, packed=True), want)
    lab, cnt = T.rel_labels(flat(torch, seqs))                       # labels alone
    assert lab.cpu().numpy().tobytes() == b"".join(want["labels"]) and cnt.cpu().tolist() == want["counts"]
    b = Batch.from_seqs(seqs, K)                                     # the Batch form fills b.prof in place
    lab2, prof, cnt2 = T.rel_labels(b, profiles=True)
    assert prof.dtype == torch.uint16 and prof.data_ptr() == b.prof.data_ptr() and prof.numel() == b.total_kmers
    assert torch.equal(lab, lab2) and torch.equal(cnt, cnt2)
    assert np.array_equal(prof.cpu().numpy(), np.concatenate(want["rel"]))
    after = (T.stats(), T.hist())
    assert before[0] == after[0] and before[1][:4] == after[1][:4] and np.array_equal(before[1][4], after[1][4])
    cnt_g = TO.genome_counter(case["genome"], K)
    assert after[0]["n_kmers"] == sum(cnt_g.values()) and after[0]["n_distinct"] == len(cnt_g)
    T.close()


def _rc(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@pytest.mark.parametrize("k", [2, 21, 63])
def test_key_and_input_edges(torch_dev, k):
    rng = random.Random(k)
    rnd = lambda n, alpha=b"ACGT": bytes(rng.choice(alpha) for _ in range(n))
    seqs = [b"A" * (k + 20), b"T" * (k + 20), b"A" * (k - 1), b"", b"C" * k, b"G"]
    seqs.append(rnd(3 * k) + b"N" + rnd(2 * k))
    seqs.append(rnd(2 * k) + b"a" + rnd(k) + b"\0" + rnd(k + 1))
    seqs.append(rnd(4 * k, b"ACGTacgtN"))
    seqs.append(rnd(5 * k + 3))
    seqs.append(_rc(seqs[-1]))
    seqs.append(b"")
    seqs.append(b"ACGT" * 40)                                        # its own reverse complement at even K
    seqs.append(rnd(7 * k))                                          # not in the genome
    genome = [seqs[0], seqs[4], seqs[6], seqs[7], seqs[8], seqs[9], seqs[9][k:3 * k + 1], seqs[12], b"", b"G" * (k - 1)]
    want = oracle_of(genome, seqs, k)
    assert (k == 2 or all(want["counts"])) and want["labels"][2] == b"N" * (k - 1) and want["labels"][3] == b""
    T = table(torch_dev, [genome], k)
    check(label_reads(torch_dev, T, seqs, k), want)
    check(label_reads(torch_dev, T, seqs, k, packed=True), want)
    check(label_reads(torch_dev, T, seqs, k, batches=[[i] for i in range(len(seqs))], packed=True), want)
    T.close()


def test_genome_order_and_batching(torch_dev, case):
    genome, seqs, want = case["genome"], case["seqs"], case["want"]
    sh = list(genome)
    random.Random(7).shuffle(sh)
    pieces = [p for g in genome for p in TO.cut(g, 1000, K)]
    for batches in ([genome], [[g] for g in genome], [sh], [pieces[:7], pieces[7:]]):
        T = table(torch_dev, batches, K)
        check(label_reads(torch_dev, T, seqs, K, packed=True), want)
        T.close()


def test_read_order_and_batching(torch_dev, case):
    torch = torch_dev
    seqs, want = case["seqs"], case["want"]
    n = len(seqs)
    T = table(torch, [case["genome"]], K)
    idx = list(range(n))
    check(label_reads(torch, T, seqs, K, batches=[idx[:5], idx[5:40], idx[40:]]), want)
    check(label_reads(torch, T, seqs, K, batches=[[i] for i in idx], packed=True), want)
    random.Random(3).shuffle(idx)
    check(label_reads(torch, T, seqs, K, batches=[idx], packed=True), want)
    _, _, counts = label_reads(torch, T, seqs, K)                    # a counts tensor passed in is added to
    _, _, again = label_reads(torch, T, seqs, K, counts=counts)
    assert again.data_ptr() == counts.data_ptr() and again.cpu().tolist() == [2 * c for c in want["counts"]]
    T.close()


def test_empty_table_is_no_error(torch_dev, case):
    from classpro_amd.api import KmerCounts
    seqs = case["seqs"][:20]
    T = KmerCounts(K)
    before = (T.stats(), T.hist())
    for _ in range(3):
        labs, prof, counts = label_reads(torch_dev, T, seqs, K)
    assert labs == [b"N" * min(K - 1, len(s)) + b"E" * max(len(s) - (K - 1), 0) for s in seqs]
    assert all(not p.any() for p in prof)
    assert counts.cpu().tolist() == [sum(max(len(s) - (K - 1), 0) for s in seqs), 0, 0, 0]
    after = (T.stats(), T.hist())                                    # stats() does not raise: absent is no error
    assert before[0] == after[0] and before[1][:4] == after[1][:4] and np.array_equal(before[1][4], after[1][4])
    assert after[0]["n_kmers"] == 0 and after[0]["n_distinct"] == 0
    T.close()


def test_growth(torch_dev, case):
    T = table(torch_dev, [[g] for g in case["genome"]], K, initial_slots=64)
    assert T.stats()["growths"] > 0
    check(label_reads(torch_dev, T, case["seqs"], K, packed=True), case["want"])
    T.close()


def test_argument_contract(torch_dev, case):
    import ctypes as C
    torch = torch_dev
    from classpro_amd._lib import lib
    T = table(torch, [case["genome"][:1]], K)
    seqs = case["seqs"][:4]
    seq, off = flat(torch, seqs)
    n, total = len(seqs), int(off[-1].item())
    buf = torch.zeros(2 * total + 64, dtype=torch.uint8, device=seq.device)
    aux = torch.zeros(n + 1, dtype=torch.int64, device=seq.device)
    cnt = torch.zeros(4, dtype=torch.int64, device=seq.device)
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda prof, poff, lab, pk, pko, c: L.cp_kmer_counts_rel_labels(
        T.t, seq.data_ptr(), off.data_ptr(), n, total, prof, poff, lab, pk, pko, c, st)
    b, a = buf.data_ptr(), aux.data_ptr()
    assert call(None, None, None, None, None, None) == -1             # CP_EINVAL: no output
    assert call(b, None, b, None, None, None) == -1                  # half a pair
    assert call(None, a, b, None, None, None) == -1
    assert call(None, None, b, b, None, None) == -1
    assert call(None, None, None, None, a, cnt.data_ptr()) == -1
    assert L.cp_kmer_counts_rel_labels(None, seq.data_ptr(), off.data_ptr(), n, total, None, None, b, None, None, None, st) == -1
    assert call(None, None, None, None, None, cnt.data_ptr()) == 0   # the counts alone are an output
    torch.cuda.synchronize()
    want = oracle_of(case["genome"][:1], seqs, K)
    assert cnt.cpu().tolist() == want["counts"]
    T.stats()
    T.close()


def test_labels_go_straight_into_label_accuracy(torch_dev, case):
    from classpro_amd.api import LabelAccuracy
    torch = torch_dev
    seqs, want = case["seqs"], case["want"]
    T = table(torch, [case["genome"]], K)
    seq, off = flat(torch, seqs)
    lab, _ = T.rel_labels((seq, off))
    truth = torch.from_numpy(np.frombuffer(b"".join(want["labels"]), np.uint8).copy()).to(seq.device)
    A = LabelAccuracy(K)
    A.add(lab, truth, off)
    s = A.stats()
    e, h, d, r = want["counts"]
    assert [s["cfm"][i][i] for i in range(4)] == [e, r, h, d]        # order E R H D
    assert sum(sum(row) for row in s["cfm"]) == e + h + d + r and s["ncor"] == s["ntot"] == e + h + d + r
    A.close()
    T.close()


def test_scale_against_torch_oracle(torch_dev):
    """A 3-Mbp diploid genome and 150 Mbases of reads sliced from it with substitutions, K = 31: labels, relative profile
    and counts against canonical keys packed into int64, torch.unique and searchsorted on the device."""
    torch = torch_dev
    from classpro_amd.api import KmerCounts
    k, G, n, L = 31, 3_000_000, 15000, 10000
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    A = torch.randint(0, 4, (G,), device=dev, generator=g)
    A[1_000_000:1_050_000] = A[200_000:250_000]                      # a repeat
    A[2_000_000:2_050_000] = A[200_000:250_000]
    snp = torch.rand(G, device=dev, generator=g) < 0.01
    snp[500_000:900_000] = False
    B = torch.where(snp, (A + torch.randint(1, 4, (G,), device=dev, generator=g)) & 3, A)
    hap = torch.stack([A, B])                                        # [2, G]: two contigs
    start = torch.randint(0, G - L, (n,), device=dev, generator=g) + G * torch.randint(0, 2, (n,), device=dev, generator=g)
    reads = hap.reshape(-1)[start[:, None] + torch.arange(L, device=dev)[None, :]]
    sub = torch.rand(n, L, device=dev, generator=g) < 0.005
    reads = torch.where(sub, (reads + torch.randint(1, 4, (n, L), device=dev, generator=g)) & 3, reads)
    rcm = torch.rand(n, device=dev, generator=g) < 0.5
    reads = torch.where(rcm[:, None], 3 - reads.flip(1), reads)
    del sub
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)

    def keys(x):                                                     # [m, len] codes -> [m, len-k+1] canonical keys
        w = x.shape[1] - k + 1
        fw = torch.zeros((x.shape[0], w), dtype=torch.int64, device=dev)
        rc = torch.zeros_like(fw)
        for j in range(k):
            bj = x[:, j:j + w]
            fw = fw * 4 + bj
            rc = rc + ((3 - bj) << (2 * j))
        return torch.minimum(fw, rc)

    T = KmerCounts(k)
    gseq = lut[hap.reshape(-1)]
    goff = torch.tensor([0, G, 2 * G], dtype=torch.int64, device=dev)
    T.add_tensors(gseq[:G], goff[:2])                                # a contig at a time
    T.add_tensors(gseq[G:], goff[:2])
    u, c = torch.unique(keys(hap).reshape(-1), return_counts=True)
    s = T.stats()
    assert s["n_distinct"] == u.numel() and s["n_kmers"] == 2 * (G - k + 1)
    rseq = lut[reads.reshape(-1)]
    roff = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    lab, prof, cnt = T.rel_labels((rseq, roff), profiles=True)
    (pk, pko), cnt2 = T.rel_labels((rseq, roff), packed=True)
    assert s == T.stats()
    T.close()
    rk = keys(reads)
    del reads
    i = torch.searchsorted(u, rk).clamp(max=u.numel() - 1)
    want = torch.where(u[i] == rk, c[i], torch.zeros_like(rk))
    del rk, i
    assert torch.equal(prof.view(torch.int16).long().reshape(n, L - k + 1), want.clamp(max=32767))
    x = want.clamp(max=3)
    wc = torch.bincount(x.reshape(-1), minlength=4)
    assert min(wc.tolist()) > 100000
    assert cnt.tolist() == wc.tolist() == cnt2.tolist()
    lab = lab.reshape(n, L)
    assert bool((lab[:, :k - 1] == ord("N")).all())
    assert torch.equal(lab[:, k - 1:], torch.tensor(list(b"EHDR"), dtype=torch.uint8, device=dev)[x])
    # the packed bytes: four labels per byte from the start of each read, N and E 0, R 1, H 2, D 3
    code = torch.tensor([0, 2, 3, 1], dtype=torch.uint8, device=dev)[x]
    full = torch.cat([torch.zeros((n, k - 1), dtype=torch.uint8, device=dev), code], 1).reshape(n, L // 4, 4)
    wpk = (full[:, :, 0] << 6) | (full[:, :, 1] << 4) | (full[:, :, 2] << 2) | full[:, :, 3]
    assert pko.tolist() == [r * (L // 4) for r in range(n + 1)] and torch.equal(pk.reshape(n, L // 4), wpk)


# ---------------------------------------------------------------------------------------------------------------------
# the command

def _write_genome(d, case, name="genome.fasta"):
    path = os.path.join(d, name)
    with open(path, "wb") as f:
        for n, s in zip(case["genome_names"], case["genome"]):
            f.write(b">" + n.encode() + b" assembled\n")
            for o in range(0, len(s), 100):                          # multi-line, as assemblies are
                f.write(s[o:o + 100] + b"\n")
    return path


def _write_source(d, kind, names, seqs):
    if kind == "fastq":
        path = os.path.join(d, "reads.fastq")
        with open(path, "wb") as f:
            for n, s in zip(names, seqs):
                f.write(b"@" + n.encode() + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
        return path
    path = os.path.join(d, "reads.fasta.gz" if kind == "fasta.gz" else "reads.fasta")
    with (gzip.open if kind == "fasta.gz" else open)(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n.encode() + b"\n" + s + b"\n")
    return path


def _tool(name):
    p = os.path.join(REF, name)
    return p if os.access(p, os.X_OK) else os.path.join(TOOLS, name)


def _run(*a):
    return subprocess.run(list(a), capture_output=True, text=True)


@pytest.mark.parametrize("kind", ["fasta", "fasta.gz", "fastq", "dam"])
def test_command(case, tmp_path, kind):
    from classpro_amd import dazz, fastk
    d = str(tmp_path)
    gen = _write_genome(d, case)
    names, seqs, want, headers = case["names"], case["seqs"], case["want"], None
    if kind == "dam":                                                # a database holds A C G T only
        seqs = [s.replace(b"N", b"A") for s in seqs]
        want = oracle_of(case["genome"], seqs, K)
        hdr = [">%s of the test" % n for n in names]
        recs = dazz.write_db(d, "reads", seqs, [(len(seqs), "reads.fasta", "reads")], dam=True, hdr_lines=hdr)
        headers = dazz.db_headers([(len(seqs), "reads.fasta", "reads")], recs, dam=True, hdr_lines=hdr)
        src = os.path.join(d, "reads.dam")
    else:
        src = _write_source(d, kind, names, seqs)
    text = TO.class_text(names, seqs, want["labels"], headers=headers)
    r = _run(G2C, "-v", "-p", "-T3", gen, os.path.join(d, "reads"))
    assert r.returncode == 0 and r.stdout == "", r.stderr
    out = os.path.join(d, "reads.truth.class")
    assert open(out, "rb").read() == text
    cnt_g = TO.genome_counter(case["genome"], K)
    skipped = sum(1 for g in case["genome"] for x in O.kmers(TO.fold(g), K) if x is None)
    line = [l for l in r.stderr.splitlines() if " contigs, " in l]
    assert len(line) == 1
    e, h, dd, rr = want["counts"]
    assert line[0] == ("4 contigs, %d genome bases, 4 pieces, %d k-mers counted, %d distinct, %d skipped, %d reads, %d bases, "
                       "E %d, H %d, D %d, R %d" % (sum(len(g) for g in case["genome"]), sum(cnt_g.values()), len(cnt_g),
                                                   skipped, len(seqs), sum(len(s) for s in seqs), e, h, dd, rr))
    rskip = sum(1 for s in seqs for x in O.kmers(s, K) if x is None)
    assert ("k-mer positions of the reads" in r.stderr) == (rskip > 0)
    if rskip:
        assert "genome2class: %d k-mer positions of the reads" % rskip in r.stderr
    # the -p files: kprof's layout, the oracle's codes, no histogram
    kk, codes = fastk.read_fastk_codes(d, "reads.truth")
    assert kk == K and codes == [fastk.encode_profile(p) for p in want["rel"]]
    assert not os.path.exists(os.path.join(d, "reads.truth.hist"))
    assert sorted(x for x in os.listdir(d) if "truth" in x) == sorted(
        ["reads.truth.class", "reads.truth.prof"] + [".reads.truth.%s.%d" % (w, p) for w in ("pidx", "prof") for p in (1, 2, 3)])
    # prof2class on those files writes the same path
    aside = os.path.join(d, "ours.class")
    shutil.copy(out, aside)
    os.remove(out)
    r = _run(_tool("prof2class"), os.path.join(d, "reads.truth.prof"), src)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(aside, "rb").read() == text


def test_command_pieces(case, tmp_path):
    """-b: contigs cut into overlapping pieces (and the reads into many batches) give the same bytes."""
    d = str(tmp_path)
    gen = _write_genome(d, case)
    _write_source(d, "fasta", case["names"], case["seqs"])
    text = TO.class_text(case["names"], case["seqs"], case["want"]["labels"])
    total = sum(TO.genome_counter(case["genome"], K).values())
    for b in (1000, 64):
        r = _run(G2C, "-v", "-b%d" % b, "-N" + os.path.join(d, "b%d" % b), gen, os.path.join(d, "reads.fasta"))
        assert r.returncode == 0 and r.stdout == "", r.stderr
        assert open(os.path.join(d, "b%d.class" % b), "rb").read() == text
        line = [l for l in r.stderr.splitlines() if " contigs, " in l][0].split(", ")
        npieces = sum(len(TO.cut(g, b, K)) for g in case["genome"])
        assert line[0] == "4 contigs" and line[2] == "%d pieces" % npieces and npieces > 4
        assert line[3] == "%d k-mers counted" % total
        assert not os.path.exists(os.path.join(d, "b%d.prof" % b))


def test_command_options(case, tmp_path):
    """-k and -N: another K, another root."""
    d = str(tmp_path)
    gen = _write_genome(d, case)
    names, seqs = case["names"][:40], case["seqs"][:40]
    src = _write_source(d, "fastq", names, seqs)
    os.mkdir(os.path.join(d, "sub"))
    root = os.path.join(d, "sub", "other")
    r = _run(G2C, "-k21", "-T2", "-N" + root, os.path.join(d, "genome"), src)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    want = oracle_of(case["genome"], seqs, 21)
    assert open(root + ".class", "rb").read() == TO.class_text(names, seqs, want["labels"])
    assert os.listdir(os.path.join(d, "sub")) == ["other.class"]


def test_command_long_fastx_read_is_refused(tmp_path):
    d = str(tmp_path)
    rng = random.Random(1)
    s = bytes(rng.choice(b"ACGT") for _ in range(60001))
    with open(os.path.join(d, "genome.fa"), "wb") as f:
        f.write(b">g\n" + s[:5000] + b"\n")
    src = _write_source(d, "fasta", ["a", "b"], [s[:300], s])
    r = _run(G2C, os.path.join(d, "genome"), src)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.endswith("rlen (60001) > rlen_max (60000)\n")
    want = oracle_of([s[:5000]], [s[:300]], K)
    assert open(os.path.join(d, "reads.truth.class"), "rb").read() == TO.class_text(["a"], [s[:300]], want["labels"])


def test_command_accuracy(torch_dev, tmp_path):
    """-A with an estimate made by ClassPro on kprof's files of the same reads: stdout is class2acc's."""
    from classpro_amd import synth
    ds = synth.make_dataset(genome_len=60000, cov=30, read_len=6000, seed=11)
    seqs = [bytes(s) for s in ds["seqs"]]
    d = str(tmp_path)
    src = _write_source(d, "fasta", ds["names"], seqs)
    with open(os.path.join(d, "genome.fa"), "wb") as f:              # some of the reads stand in for an assembly
        for i, s in enumerate(seqs[::3]):
            f.write(b">c%d\n" % i + s + b"\n")
    r = _run(os.path.join(TOOLS, "kprof"), "-T4", src)
    assert r.returncode == 0, r.stderr
    r = _run(os.path.join(TOOLS, "ClassPro"), "-T4", "-P" + d, src)
    assert r.returncode == 0, r.stderr
    est = os.path.join(d, "reads.class")
    out = os.path.join(d, "reads.truth.class")
    r = _run(G2C, "-A" + est, os.path.join(d, "genome"), os.path.join(d, "reads"))
    assert r.returncode == 0, r.stderr
    want = oracle_of(seqs[::3], seqs, K)
    assert open(out, "rb").read() == TO.class_text(ds["names"], seqs, want["labels"])
    assert min(want["counts"]) > 0
    tools = [os.path.join(TOOLS, "class2acc")] + ([os.path.join(REF, "class2acc")] if os.access(os.path.join(REF, "class2acc"), os.X_OK) else [])
    for t in tools:
        c = _run(t, est, out)
        assert c.returncode == 0 and c.stdout == r.stdout and "Confusion Matrix" in r.stdout, t
    # an estimate with a renamed read, and one a record short: class2acc's messages
    recs = open(est, "rb").read().split(b"\n@")
    bad = os.path.join(d, "renamed.class")
    with open(bad, "wb") as f:
        f.write(b"\n@".join(recs[:5] + [b"other " + recs[5].split(b" ", 1)[1]] + recs[6:]))
    short = os.path.join(d, "short.class")
    with open(short, "wb") as f:
        f.write(b"\n@".join(recs[:-1]) + b"\n")
    for path in (bad, short):
        r = _run(G2C, "-A" + path, "-N" + os.path.join(d, "again"), os.path.join(d, "genome"), os.path.join(d, "reads"))
        c = _run(os.path.join(TOOLS, "class2acc"), path, out)
        assert r.returncode == c.returncode == 1 and r.stdout == ""
        assert r.stderr == c.stderr.replace(out, os.path.join(d, "again.class")) and r.stderr
    assert "inconsistent names: other (estimate) vs %s (truth)" % ds["names"][5] in _run(
        G2C, "-A" + bad, "-N" + os.path.join(d, "again"), os.path.join(d, "genome"), os.path.join(d, "reads")).stderr

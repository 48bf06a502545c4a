"""The batch loop over a .class file that class2cns and class2ktab share (csrc/host/class_record.h for_class_batches),
driven on the CPU by tests/class_batch_check.cpp with heap buffers of exactly the size asked for, under AddressSanitizer
and UBSan: the records come back byte for byte, plain and gzipped, and the batches end where the flush rule says, at
capacities that put a boundary at every record, records longer than a batch included.  A record longer than the batch
capacity makes the loop grow the sequence buffers; it must not give the offsets buffer back with them (h_off[0], set
to 0 by the flush before, would be lost): the 65- and 200-base records at capacity 64 are that case."""
import gzip
import os
import subprocess

import pytest

from conftest import ROOT, build_if_changed

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")       # the checker frees its buffers; a tool that dies does not

LENGTHS = [0, 1, 63, 64, 65, 200, 3, 3, 3, 3, 3, 64, 1, 0, 0, 0, 0, 70]
CAPACITIES = [(64, 4), (64, 100), (1000, 2), (1, 1), (10**6, 1 << 16)]


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "class_batch_check.cpp")
    out = os.path.join(ROOT, "tests", "_class_batch_check")
    deps = [src] + [os.path.join(ROOT, "classpro_amd", "csrc", "host", f) for f in ("class_record.h", "host_io.h")]
    return build_if_changed(out, ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                  "-o", out, src, "-lz"], deps)


def _class_text():
    out = []
    for i, n in enumerate(LENGTHS):
        header = b"@r%d" % i + (b" comment %d of two in three" % i if i % 3 != 2 else b"")
        seq = bytes(b"ACGT"[(i + j) % 4] for j in range(n))
        lab = bytes(b"EHDR"[(i + j // 3) % 4] for j in range(n))
        out.append(header + b"\n" + seq + b"\n+\n" + lab + b"\n")
    return b"".join(out)


@pytest.fixture(scope="module")
def class_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("class_batch")
    text = _class_text()
    plain, gz = d / "est.class", d / "est.class.gz"
    plain.write_bytes(text)
    with gzip.open(gz, "wb") as f:
        f.write(text)
    return text, [str(plain), str(gz)]


def _model(batch_bases, batch_reads):
    """The flush rule: a batch ends before a record that would not fit the bases or the offsets; then the base capacity
    grows to a record longer than it."""
    cap_bases, cap_reads = batch_bases, batch_reads + 1
    batches, nreads, nbases = [], 0, 0
    for n in LENGTHS:
        if nbases + n > cap_bases or nreads + 1 >= cap_reads:
            if nreads:
                batches.append((nreads, nbases))
            nreads = nbases = 0
        if n > cap_bases:
            cap_bases = n
        nreads, nbases = nreads + 1, nbases + n
    if nreads:
        batches.append((nreads, nbases))
    return batches


def test_model_restates_the_known_case():
    assert _model(64, 4) == [(3, 64), (1, 64), (1, 65), (1, 200), (4, 12), (4, 68), (4, 70)]
    assert _model(10**6, 1 << 16) == [(len(LENGTHS), sum(LENGTHS))]


@pytest.mark.parametrize("batch_bases,batch_reads", CAPACITIES)
def test_batches_and_records(checker, class_files, batch_bases, batch_reads):
    text, paths = class_files
    for path in paths:
        run = subprocess.run([checker, path, str(batch_bases), str(batch_reads)], capture_output=True, env=ENV)
        assert run.returncode == 0 and run.stderr == b"", (path, run.returncode, run.stderr.decode(errors="replace")[-2000:])
        lines = run.stdout.split(b"\n")
        assert lines[-1] == b""
        batches, records, at = [], [], 0
        while at < len(lines) - 1:
            tag, nreads, nbases = lines[at].split()
            assert tag == b"B"
            batches.append((int(nreads), int(nbases)))
            records += lines[at + 1:at + 1 + 4 * int(nreads)]
            at += 1 + 4 * int(nreads)
        print(path, (batch_bases, batch_reads), batches)
        assert b"".join(l + b"\n" for l in records) == text
        assert batches == _model(batch_bases, batch_reads)


def test_record_without_labels(checker, tmp_path):
    p = tmp_path / "reads.fasta"
    p.write_bytes(b">a\nACGT\n")
    run = subprocess.run([checker, str(p), "64", "4"], capture_output=True, env=ENV)
    assert run.returncode == 1
    assert run.stdout == b""
    assert run.stderr == b"class_batch_check: record a of %s carries no labels\n" % str(p).encode()

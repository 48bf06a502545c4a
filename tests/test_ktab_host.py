"""The FASTK k-mer table files without a GPU: fastk.write_fastk_ktab / read_fastk_ktab against the byte-level oracle of
tests/ktab_oracle.py, and the written files through the reference's own readers (Open_Kmer_Stream, Load_Kmer_Table,
Find_Kmer of libfastk.c, compiled into oracle/_ref).  Everything is bytes and integers: the tolerance is zero."""
import os
import random

import numpy as np
import pytest

import ktab_oracle as KO

KS = [5, 8, 9, 12, 13, 16, 21, 31, 32, 40, 63]


def reads_for(K, seed=0):
    """A few hundred k-mers: random reads, a repeated one (counts above 1), poly-A and the first and last bucket."""
    rng = random.Random(1000 * K + seed)
    rnd = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    seqs = [rnd(K + 60) for _ in range(4)]
    seqs += [seqs[0][:K + 20]] * 2 + [b"A" * (K + 3), b"T" * 12 + rnd(max(K - 24, 0)) + b"A" * 12 if K >= 24 else rnd(K)]
    return seqs


def test_ibyte():
    from classpro_amd import fastk
    assert [fastk.ktab_ibyte(k) for k in (2, 4, 5, 8, 9, 12, 13, 40, 63)] == [0, 0, 1, 1, 2, 2, 3, 3, 3]
    assert all(fastk.ktab_ibyte(k) == KO.ibyte_of(k) for k in range(2, 64))
    with pytest.raises(ValueError):
        fastk.write_fastk_ktab("/nonexistent", "x", 4, 1, [], [])


@pytest.mark.parametrize("K", KS)
def test_round_trip_and_bytes(tmp_path, K):
    from classpro_amd import fastk
    ents = KO.table(reads_for(K), K)
    assert len(ents) > 100 or K < 8
    assert any(c > 1 for _, c in ents)
    if K in (32, 40, 63):
        assert any(k >> 63 for k, _ in ents)               # keys that reach into hi
    if K == 63:
        assert max(k for k, _ in ents).bit_length() > 120
    assert KO.records_fast(ents, K) == KO.records(ents, K)
    for minc in (1, 2):
        sub = [(k, c) for k, c in ents if c >= minc]
        for nparts in (1, 3, len(sub) + 2) if minc == 1 else (2,):
            d = str(tmp_path / ("m%d_p%d" % (minc, nparts)))
            fastk.write_fastk_ktab(d, "tab", K, minc, [k for k, _ in sub], [c for _, c in sub], nparts)
            assert KO.read_files(d, "tab", nparts) == KO.files(sub, K, minc, nparts)
            assert len(os.listdir(d)) == nparts + 1
            k, m, ib, keys, counts = fastk.read_fastk_ktab(d, "tab")
            assert (k, m, ib) == (K, minc, KO.ibyte_of(K))
            assert keys == [x for x, _ in sub] and counts.tolist() == [c for _, c in sub]


@pytest.mark.parametrize("K", [5, 9, 12, 21, 31])
def test_numpy_form_of_the_oracle(K):
    """The vectorised restatement that the large GPU cases use gives what the brute-force one gives."""
    rng = random.Random(K)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (K + 200, K - 1, 3 * K, K)] + [b"A" * (K + 40000)]
    seqs += [seqs[0][20:K + 90]] * 2
    for minc in (1, 2):
        ents = KO.table(seqs, K, minc)
        keys, counts = KO.table_np(seqs, K, minc)
        assert keys.tolist() == [k for k, _ in ents] and counts.tolist() == [c for _, c in ents]
        assert counts.max() > KO.MAXC
        assert KO.records_np(keys, counts, K) == KO.records(ents, K)
        assert np.array_equal(KO.index_np(keys, K), KO.index(ents, K))


def test_clamp_and_pad_bits(tmp_path):
    from classpro_amd import fastk
    K = 21                                                 # 42 bits in 6 bytes: the last 6 bits of a record's key are 0
    keys = [0, 5, (1 << 42) - 1]
    fastk.write_fastk_ktab(str(tmp_path), "t", K, 1, keys, [40000, 32767, 7], 1)
    want = KO.files(list(zip(keys, [40000, 32767, 7])), K, 1, 1)
    assert KO.read_files(str(tmp_path), "t", 1) == want
    rec = want[1][12:]
    assert len(rec) == 3 * 5 and rec[0:5] == b"\0\0\0\xff\x7f" and rec[10:15] == b"\xff\xff\xc0\x07\x00"
    assert fastk.read_fastk_ktab(str(tmp_path), "t")[4].tolist() == [32767, 32767, 7]
    with pytest.raises(ValueError):
        fastk.write_fastk_ktab(str(tmp_path), "u", K, 1, [5, 5], [1, 1], 1)


@pytest.mark.parametrize("K", [5, 12, 40])
def test_empty_table(tmp_path, K):
    """Python reader only: the reference's Open_Kmer_Stream walks off the index of a table without entries."""
    from classpro_amd import fastk
    fastk.write_fastk_ktab(str(tmp_path), "e", K, 3, [], [], 1)
    assert KO.read_files(str(tmp_path), "e", 1) == KO.files([], K, 3, 1)
    k, m, ib, keys, counts = fastk.read_fastk_ktab(str(tmp_path), "e")
    assert (k, m, ib, keys, len(counts)) == (K, 3, KO.ibyte_of(K), [], 0)


def check_through_reference(L, d, root, K, minval, ents, absent):
    """The files under d/root against the oracle's entries, through the reference's stream and loaded table."""
    path = os.path.join(d, root)
    k, m, got = KO.ref_stream(L, path)
    assert (k, m) == (K, minval)
    assert got == [(KO.text_of(x, K), min(c, KO.MAXC)) for x, c in ents]
    T = KO.RefTable(L, path)
    assert (T.K, T.minval, T.nels) == (K, minval, len(ents))
    for i, (x, _) in enumerate(ents):
        assert T.find(KO.text_of(x, K)) == i
    assert T.find(KO.text_of(ents[-1][0], K).upper()) == len(ents) - 1
    rc = bytes.maketrans(b"acgt", b"tgca")
    t0 = KO.text_of(ents[0][0], K)
    assert T.find(t0.encode().translate(rc)[::-1].decode()) == 0          # the other strand finds the same entry
    have = {x for x, _ in ents}
    for x in absent:
        if x not in have:
            assert T.find(KO.text_of(x, K)) < 0
    T.close()
    cut = minval + 1
    sub = [(x, c) for x, c in ents if c >= cut]
    if sub:
        T = KO.RefTable(L, path, cut)
        assert (T.minval, T.nels) == (cut, len(sub))
        assert [T.fetch(i) for i in range(len(sub))] == [KO.text_of(x, K) for x, _ in sub]
        for i, (x, _) in enumerate(sub):
            assert T.find(KO.text_of(x, K)) == i
        gone = [x for x, c in ents if c < cut][:20]
        assert all(T.find(KO.text_of(x, K)) < 0 for x in gone)
        T.close()


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_through_the_reference_readers(tmp_path, K, nparts):
    from classpro_amd import fastk
    L = KO.ref_lib()
    if L is None:
        pytest.skip("the reference's own readers (oracle/_ref) are not built here")
    ents = KO.table(reads_for(K, 1), K)
    rng = random.Random(K)
    absent = [KO.key_of(KO.O.canon(KO.text_of(rng.getrandbits(2 * K), K).upper().encode())) for _ in range(50)]
    fastk.write_fastk_ktab(str(tmp_path), "tab", K, 1, [k for k, _ in ents], [c for _, c in ents], nparts)
    check_through_reference(L, str(tmp_path), "tab", K, 1, ents, absent)

"""Inputs and the CPU comparison shared by tests/test_rel_anchor_cells.py and tests/test_gpu_rel_grp_stream.py: reads whose
classify_rel DP looks an anchor up on a stand-in (see test_rel_anchor_cells.py), found with tests/rel_anchor_probe.cpp."""
import ctypes as C
import os

import numpy as np
from conftest import ROOT, build_if_changed
from oracle.oracle import INTVL_DTYPE

K, HC, DC = 40, 20, 40
MAX_PLEN = 65535          # GRP_MAX_PLEN of kernels.hip: the pairs are 16 + 16 bits
vp = C.c_void_p


def load_probe():
    """tests/rel_anchor_probe.cpp, compiled for the host."""
    src = os.path.join(ROOT, "tests", "rel_anchor_probe.cpp")
    out = os.path.join(ROOT, "tests", "_rel_anchor_probe.so")
    csrc = os.path.join(ROOT, "classpro_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    build_if_changed(out, ["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src], deps)
    R = C.CDLL(out)
    R.rap_params_new.restype = vp
    return R


def reliable_intervals(H, P, s, p):
    """The reliable intervals of a read, from the product's scalar functions (tests/host_harness.cpp)."""
    rlen = len(s)
    cap = rlen + 2
    lab = np.zeros(rlen, np.uint8)
    iv, riv = np.zeros(cap, INTVL_DTYPE), np.zeros(cap, INTVL_DTYPE)
    fw, bw = np.zeros(cap, np.int8), np.zeros(cap, np.int8)
    M = C.c_int()
    sb = np.frombuffer(s, np.uint8)
    H.hh_classify_read(vp(P), sb.ctypes.data_as(vp), rlen, p.ctypes.data_as(vp), lab.ctypes.data_as(vp),
                       iv.ctypes.data_as(vp), cap, C.byref(M), riv.ctypes.data_as(vp), fw.ctypes.data_as(vp),
                       bw.ctypes.data_as(vp))
    return riv[:M.value].copy()


def run_direction(R, P, riv, plen, F, anchored):
    M = len(riv)
    a_dp, a = np.zeros(M, np.int8), np.zeros(M, np.int8)
    par, rp = np.zeros(4 * M, np.int8), np.zeros(M, np.uint8)
    hb, n = C.c_uint64(), C.c_longlong(0)
    rerun = R.rap_direction(vp(P), riv.ctypes.data_as(vp), M, plen, F, anchored, a_dp.ctypes.data_as(vp),
                            a.ctypes.data_as(vp), par.ctypes.data_as(vp), rp.ctypes.data_as(vp), C.byref(hb), C.byref(n))
    return dict(asgn_dp=a_dp, asgn=a, parent=par, rpos=rp, hdrr_bits=hb.value, rerun=rerun), n.value


def input_reads():
    from adversarial import adversarial_reads
    from classpro_amd import synth
    seqs, profs = adversarial_reads(7, n=150)
    out = [("adversarial(7) read %d" % j, s, p) for j, (s, p) in enumerate(zip(seqs, profs))]
    ds = synth.make_dataset(genome_len=200000, cov=40, read_len=10000, seed=5)
    out += [("10-kb set read %d" % j, ds["seqs"][j], ds["profiles"][j]) for j in range(150)]
    return out


def standin_reads(harness, probe):
    """[(name, seq, prof, M, look-ups fw, look-ups bw)] of the input reads with M > 0, after checking each of them."""
    P = probe.rap_params_new(K, 20000, HC, DC)
    assert P
    rows = []
    for name, s, p in input_reads():
        p = np.ascontiguousarray(p, np.uint16)
        if len(s) < K or len(p) > MAX_PLEN:
            continue
        riv = reliable_intervals(harness, P, s, p)
        if len(riv) == 0:
            continue
        n = [0, 0]
        for F in (1, 0):
            want, n[1 - F] = run_direction(probe, P, riv, len(p), F, 0)
            got, _ = run_direction(probe, P, riv, len(p), F, 1)
            where = "%s (M = %d), %s" % (name, len(riv), "forward" if F else "backward")
            for k in ("asgn_dp", "asgn", "parent", "rpos"):
                assert np.array_equal(got[k], want[k]), "%s: %s" % (where, k)
            assert got["rerun"] == want["rerun"] and got["hdrr_bits"] == want["hdrr_bits"], where
        rows.append((name, s, p, len(riv), n[0], n[1]))
    probe.rap_params_free(vp(P))
    return rows

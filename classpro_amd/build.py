"""Build libclasspro_amd.so in-tree: hipcc cross-compiles gfx950 without a GPU.

    python -m classpro_amd.build [--force]
"""
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
OUT = os.path.join(_HERE, "libclasspro_amd.so")
SYNTH = os.path.join(_HERE, "libcp_synth.so")  # device-side synthetic read sets: test / bench infrastructure (csrc/synth/)
CLI = os.path.join(_HERE, "ClassPro")          # drop-in command line (csrc/host/classpro_main.cpp)
CNS = os.path.join(_HERE, "class2cns")         # per-k-mer label consensus (csrc/host/class2cns.cpp; its flags use the GPU)
GS = os.path.join(_HERE, "ClassGS")             # global-threshold labels and their accuracy (csrc/host/classgs.cpp; uses the GPU)
KPROF = os.path.join(_HERE, "kprof")           # count profiles and histogram from reads (csrc/host/kprof.cpp; uses the GPU)
G2C = os.path.join(_HERE, "genome2class")      # ground-truth labels from a genome (csrc/host/genome2class.cpp; uses the GPU)
C2K = os.path.join(_HERE, "class2ktab")        # per-class k-mer tables of a .class (csrc/host/class2ktab.cpp; uses the GPU)
T2P = os.path.join(_HERE, "tab2prof")          # profiles relative to a k-mer table (csrc/host/tab2prof.cpp; uses the GPU)
TOP = os.path.join(_HERE, "tabop")             # set algebra on two k-mer tables (csrc/host/tabop.cpp; uses the GPU)
TBIN = os.path.join(_HERE, "tabbin")           # per-read hits and switches in two k-mer tables (csrc/host/tabbin.cpp; uses the GPU)
TCMP = os.path.join(_HERE, "tabcmp")           # 2-D count comparison of two k-mer tables, QV (csrc/host/tabcmp.cpp; uses the GPU)
TTRK = os.path.join(_HERE, "tabtrack")         # runs of k-mer states along sequences, QV, phase blocks (csrc/host/tabtrack.cpp; uses the GPU)
THET = os.path.join(_HERE, "tabhet")           # heterozygous k-mer pairs of one k-mer table (csrc/host/tabhet.cpp; uses the GPU)
TUTG = os.path.join(_HERE, "tabunitig")        # unitigs of one k-mer table's de Bruijn graph (csrc/host/tabunitig.cpp; uses the GPU)
TGRF = os.path.join(_HERE, "tabgraph")         # links and components of that graph, as GFA (csrc/host/tabgraph.cpp; uses the GPU)
TPTH = os.path.join(_HERE, "tabpath")          # reads threaded through that graph, as GAF (csrc/host/tabpath.cpp; uses the GPU)
TCLN = os.path.join(_HERE, "tabclean")         # tips, bubbles and islands of that graph removed (csrc/host/tabclean.cpp; uses the GPU)
TFIX = os.path.join(_HERE, "tabfix")             # read errors a table can name, fixed on the device (csrc/host/tabfix.cpp; uses the GPU)
TPHS = os.path.join(_HERE, "tabphase")         # heterozygous pairs phased from reads into two marker tables (csrc/host/tabphase.cpp; uses the GPU)
TOOLS = {"prof2class": "prof2class.cpp", "class2acc": "class2acc.cpp"}   # host-only evaluation tools
# -ffp-contract=off: the decision path compares doubles against thresholds and truncates them to
# ints (class_rel.c:449,483); fused multiply-adds would change those values.
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17"]


# CP_SANITIZE=1 (scripts/sanitize.sh): the host-only tools are built with AddressSanitizer + UBSan.  The HIP objects never
# are (GPU sanitizers are not available on this pool); the scalar device functions are covered through
# tests/host_harness.cpp, which compiles the same headers for the host.
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if os.environ.get("CP_SANITIZE") == "1" else []


def _src_key(extra):
    """Hash of the CONTENT of every source the outputs are built from (+ the flags): after a fresh checkout, or on a
    snapshot copied to another box, every mtime is the copy time and says nothing (same rule as tests/conftest.py)."""
    import hashlib
    h = hashlib.sha1(" ".join(extra).encode())
    files = [os.path.join(_HERE, "..", "include", "classpro_amd.h")]
    for root, _d, names in os.walk(CSRC):
        files += [os.path.join(root, f) for f in names]
    for f in sorted(files):
        h.update(os.path.relpath(f, _HERE).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def _fresh(outs, side, key, force):
    return (not force and all(os.path.exists(o) for o in outs)
            and os.path.exists(side) and open(side).read().strip() == key)


def _run(cmd, verbose):
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)


def build(force=False, verbose=False):
    # the HIP objects: library, command line, synthetic-set generator
    outs, side, key = [OUT, CLI, CNS, GS, KPROF, G2C, C2K, T2P, TOP, TBIN, TTRK, TCMP, THET, TUTG, TGRF, TPTH, TCLN, TFIX, TPHS, SYNTH], os.path.join(_HERE, ".build.srchash"), _src_key(FLAGS)
    if not _fresh(outs, side, key, force):
        if os.path.exists(side):
            os.remove(side)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        _run([hipcc] + FLAGS + [os.path.join(CSRC, "capi.hip"), "-o", OUT], verbose)
        for src, out, pthread in (("classpro_main.cpp", CLI, True), ("class2cns.cpp", CNS, False), ("classgs.cpp", GS, False),
                                  ("kprof.cpp", KPROF, True), ("genome2class.cpp", G2C, True), ("class2ktab.cpp", C2K, False),
                                  ("tab2prof.cpp", T2P, True), ("tabop.cpp", TOP, False), ("tabbin.cpp", TBIN, False),
                                  ("tabtrack.cpp", TTRK, False),
                                  ("tabcmp.cpp", TCMP, False), ("tabhet.cpp", THET, False),
                                  ("tabunitig.cpp", TUTG, False), ("tabgraph.cpp", TGRF, False),
                                  ("tabpath.cpp", TPTH, False), ("tabclean.cpp", TCLN, False),
                                  ("tabfix.cpp", TFIX, False), ("tabphase.cpp", TPHS, False)):
            _run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(CSRC, "host", src), "-o", out,
                  "-L" + _HERE, "-lclasspro_amd", "-lz"] + ["-lpthread"] * pthread + ["-Wl,-rpath,$ORIGIN"], verbose)
        _run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17",
              os.path.join(CSRC, "synth", "synth_gen.hip"), "-o", SYNTH], verbose)
        with open(side, "w") as f:
            f.write(key + "\n")
    # the host-only evaluation tools
    outs, side, key = [os.path.join(_HERE, t) for t in TOOLS], os.path.join(_HERE, ".tools.srchash"), _src_key(["tools"] + SAN)
    if not _fresh(outs, side, key, force):
        if os.path.exists(side):
            os.remove(side)
        for tool, src in TOOLS.items():
            _run([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off"] + SAN
                 + [os.path.join(CSRC, "host", src), "-o", os.path.join(_HERE, tool), "-lz"], verbose)
        with open(side, "w") as f:
            f.write(key + "\n")
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

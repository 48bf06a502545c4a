#!/usr/bin/env python3
"""Diagnostic: where k_wall_tasks and k_find_wall spend their cycles on the WHOLE-PATH call (compact records, find_rel inside the emission loop) (needs build_diag/lib_walk.so, built
with -DCP_PROF_WALK; run with CLASSPRO_AMD_LIB=build_diag/lib_walk.so on the GPU box)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from classpro_amd import synth
from classpro_amd.api import Classifier, Batch, hist_covs, STAGE_REL
from classpro_amd._lib import lib

if len(sys.argv) > 1 and sys.argv[1] == "python-synth":
    ds = synth.make_dataset(genome_len=5_000_000, cov=40, read_len=20000, K=40, het=0.001, n_repeats=62, min_len=3000, seed=1)
    low, high, il, ih, h = ds["hist"]
    hc, dc = hist_covs(h, low, high, il, ih, 0)
    b = Batch.from_reads(ds["seqs"], ds["profiles"])
else:                                                     # the bench's generator: one 800-Mbase sub-batch
    from classpro_amd.synth_dev import DeviceSynth
    sy = DeviceSynth(genome_len=20_000_000, cov=40, read_len=20000, seed=1)
    low, high, il, ih, h = sy.hist
    hc, dc = hist_covs(h, low, high, il, ih, 0)
    b = Batch.from_device(sy.reads(0, sy.n_reads))
clf = Classifier(40, 20000, hc, dc)
ph = (C.c_ulonglong * 36)()
lv = (C.c_ulonglong * 8)()
em = (C.c_ulonglong * 8)()
ur = (C.c_ulonglong * 12)()
rp = (C.c_ulonglong * 13)()
fw = (C.c_ulonglong * 12)()
clf.classify(b)
lib().cp_debug_unrel_prof(ur)
lib().cp_debug_phase_prof(ph)
lib().cp_debug_live_prof(lv)
lib().cp_debug_emit_prof(em)
lib().cp_debug_fw_prof(fw)
clf.classify(b)
lib().cp_debug_phase_prof(ph)
lib().cp_debug_live_prof(lv)
lib().cp_debug_emit_prof(em)
lib().cp_debug_unrel_prof(ur)
lib().cp_debug_fw_prof(fw)
lib().cp_debug_rel_prof(rp)
pn = {0: "k_wall_tasks: candidate list", 7: "k_wall_tasks: prelude + filters", 6: "k_wall_tasks: live tasks",
      1: "k_find_wall: replay", 2: "unwall/sort/olist", 3: "multi-error search", 4: "merge + sorts",
      8: "components + boundaries", 5: "records + find_rel"}
print("phase                          max over reads (ticks)   mean      argmax read / its ncand   (100 MHz ticks)")
for k in (0, 7, 6, 1, 2, 3, 4, 8, 5):
    print("  %-34s %12d %12.1f      %d / %d" % (pn[k], ph[k], ph[12 + k] / b.nreads, ph[24 + k] >> 32, ph[24 + k] & 0xffffffff))
print("replay chunks %d (%.1f tasks each): dependency rounds per chunk %.2f with the hashed table, %.2f with exact key comparisons"
      % (lv[2], lv[3] / max(1, lv[2]), lv[0] / max(1, lv[2]), lv[1] / max(1, lv[2])))
print("k_find_wall, ticks per read (mean over all reads): head up to the first chunk %.1f (%d reads on the lane-parallel replay), chunk heads %.1f "
      "(%d chunks, %.1f ticks each)" % (fw[0] / b.nreads, fw[3], fw[1] / b.nreads, fw[2], fw[1] / max(1, fw[2])))
print("k_find_wall, emission loop, ticks per read: boundaries %.1f, cp_make_interval %.1f, find_rel %.1f, compaction and record stores %.1f"
      % (fw[4] / b.nreads, fw[5] / b.nreads, fw[6] / b.nreads, fw[7] / b.nreads))
print("E-interval lists of at most 64 (the wave-parallel forms): before the un-wall %d reads (mean length %.1f), before the merge %d (%.1f), before the components %d (%.1f)"
      % (em[0], em[1] / b.nreads, em[2], em[3] / b.nreads, em[4], em[5] / b.nreads))
print("classify_unrel (main class): %.1f non-fixed intervals per read, %.1f speculation rounds in the first sweep (eight slots per round: UNREL_SMALL_G = 2 reads per wave, UNREL_LPS = 4 lanes per slot), %.1f in the second"
      % (ph[12 + 10] / max(1, ph[12 + 11]), ph[12 + 9] / max(1, ph[12 + 11]), ph[9] / max(1, ph[12 + 11])))
print("classify_unrel (rare class, sixteen slots per round): %d reads, %.1f non-fixed intervals per read, %.1f rounds in the first sweep, %.1f in the second"
      % (ur[11], ur[10] / max(1, ur[11]), ur[8] / max(1, ur[11]), ur[9] / max(1, ur[11])))
nw, tot = max(1, ur[3]), max(1, ur[2])
print("classify_unrel (main class): %d waves, %.1f ticks per wave" % (ur[3], ur[2] / nw))
for name, v in (("interval load before the rounds", ur[5]), ("sort of the non-fixed intervals", ur[6]),
                ("round: up to the first global load issued", ur[1]), ("round: waiting for the loads and using them", ur[4]),
                ("round: committing the slots", ur[0]), ("head and final write", ur[2] - ur[0] - ur[1] - ur[4] - ur[5] - ur[6])):
    print("    %-46s %9.1f ticks per wave  %5.1f %%" % (name, v / nw, 100.0 * v / tot))
print("classify_rel: %d of %d (read, direction) passes are repeated with adjusted coverages (class_rel.c:629-650); %d of %d waves run the DP a second time"
      % (em[6] & 0xffffffff, em[6] >> 32, em[7] & 0xffffffff, em[7] >> 32))
if rp[9]:
    names = ["step: start to the return of its loads", "step: from there to the tr values", "step: state phase", "step: syncs",
             "traceback", "cp_rel_post1", "cp_rel_post2", "fw / bw compare"]
    order = [10, 0, 12, 1, 2, 3, 4, 5, 6, 7, 11]
    label = dict(zip(range(8), names)); label[10] = "init of a pass"; label[11] = "final write"
    label[12] = "  of which the head, up to the load addresses"
    print("classify_rel (main class): %d groups of eight reads, %.1f ticks per group (stamped: every stamp drains the wave's memory operations)" % (rp[9], rp[8] / rp[9]))
    for k in order:
        v = rp[0] + rp[12] if k == 0 else rp[k]            # (the stamp of [12] splits what [0] was)
        print("    %-42s %9.1f ticks per group  %5.1f %%" % (label[k], v / rp[9], 100.0 * v / rp[8]))
print("reads %d: memo on chip %d, flags on chip to the end %d, sent their flags to the arrays after the replay (more off-list SELF walls than slots) %d, flags on chip after the walk %d" %
      (b.nreads, lv[4], lv[5], lv[6], lv[7]))

"""Inputs of tests/test_find_wall_handoff_inputs.py and tests/test_gpu_find_wall_handoff.py: small reads at the edges of
the task record that k_wall_tasks hands to k_find_wall (classpro_amd/csrc/kernels.hip: task_res) and of the replay's
chunks of 64 tasks.

The record carries the candidate's position, its pass (SELF / OTHERS), its wall type and its row in the candidate list,
the low-complexity partner's position and the best high-complexity partner as a signed offset; k_find_wall loads a
chunk's records at tb+lane and nothing else.  What the reads are for:

  * task counts around one and two chunks (63, 64, 65, 127, 128, 129), the latter three with OTHERS tasks among them so
    that the memo stays on chip and the chunks are replayed a lane per task;
  * a pair of tasks of ONE candidate (its SELF and its OTHERS task) as the last of a chunk and the first of the next;
  * a pairing across the chunk's end in either direction: the last task of chunk 0 accepts the candidate of the first
    task of chunk 1 (a tooth), and the first task of chunk 1 accepts the candidate of the last task of chunk 0 (`REV`:
    the DROP pairs off the candidates, the GAIN behind it then pairs with the DROP);
  * the high-complexity partner at the largest offset on either side: K-1+CP_MAX_N_HC = K+4 positions to the right of a
    DROP (a tooth of K+4 positions) and to the left of a GAIN (`REV`);
  * low-complexity partners beyond either end of the read (lc_j = 0 and lc_j = plen);
  * a position beyond 16 bits, a row beyond 8 bits;
  * the memo rules' edges: 124 | 125 SELF tasks, 28 | 29 OTHERS tasks (the larger of each takes the one-lane replay);
  * a read with no k-mer, a read with no candidate.

The motifs are those of wall_path_inputs, plus
  DUAL   60 at 80, K at 65, 60 at 80   the two inner walls change a count beyond cmax by less than the haploid coverage:
                                       each is a SELF task AND an OTHERS task; the outer walls are a SELF task each
  REV    K at 1, 4 at 3                a DROP, and K+4 positions on a GAIN (1 -> 3 is no candidate)
Seeds are chosen so that the account (wall_path_inputs.account) has the numbers asserted in
tests/test_find_wall_handoff_inputs.py and the reference accepts the read.
"""
import functools

import numpy as np

import wall_path_inputs as W
import wall_load_inputs as L
from wall_path_inputs import Read, K, READ_LEN, HCOV, DCOV, motif_read, TO_3, _read

WAVE = 64
CP_MAX_N_HC = 5
TOOTH = [(K, 1), (80, DCOV)]
DUAL = [(60, 80), (K, 65), (60, 80), (90, DCOV)]
REV = [(K, 1), (4, 3), (100, DCOV)]
WIDE = [(K + CP_MAX_N_HC - 1, 1), (90, DCOV)]             # the GAIN is the DROP's last high-complexity partner
FROM_3 = [(60, 3)]                                         # a read that begins at 3: one candidate, one SELF task


def candidates(r):
    """The candidate positions of a read by the scan rule, in order (row k of the kernel's candidate list)."""
    p = r.prof.astype(np.int64)
    repeat = L.tables().cov[1]
    i = np.arange(1, len(p))
    return i[(np.minimum(p[:-1], p[1:]) < repeat) & (np.abs(p[:-1] - p[1:]) >= 3)]


@functools.lru_cache(maxsize=None)
def reads():
    R = [motif_read("hf_nt63", 501, tooth=31, end=TO_3), motif_read("hf_nt64", 502, tooth=32),
         motif_read("hf_nt65", 503, tooth=32, end=TO_3),
         motif_read("hf_nt127", 504, tooth=56, o_tooth=7, end=TO_3), motif_read("hf_nt128", 505, tooth=57, o_tooth=7),
         motif_read("hf_nt129", 506, tooth=57, o_tooth=7, end=TO_3)]
    R += [_read("hf_same_cand_63_64", [(90, DCOV)] + TOOTH * 31 + DUAL, 511),
          _read("hf_pair_63_to_64", FROM_3 + [(90, DCOV)] + TOOTH * 32, 512),
          _read("hf_pair_64_to_63", FROM_3 + [(90, DCOV)] + TOOTH * 31 + REV, 513),
          # (two teeth in front: a read of fewer than four candidates has no room for its E-intervals on chip and keeps its flags in the arrays)
          _read("hf_hc_right", [(90, DCOV)] + TOOTH * 2 + WIDE, 514), _read("hf_hc_left", [(90, DCOV)] + TOOTH * 2 + REV, 515)]
    R += [L.edge_read("hf_boundaries", 520, 20, 20), W.long_comb("hf_plen66300", 66300, 521),
          motif_read("hf_row256", 522, tooth=50, plateau=78, end=TO_3)]
    R += [motif_read("hf_self124", 531, tooth=62), motif_read("hf_self125", 532, tooth=62, end=TO_3),
          motif_read("hf_others28", 533, tooth=5, o_tooth=14), motif_read("hf_others29", 536, tooth=5, o_tooth=14, o_plat=1)]
    rng = np.random.default_rng(540)
    R += [Read("hf_no_kmer", bytes(b"ACGT"[v] for v in rng.integers(0, 4, K - 1)), np.zeros(0, np.uint16)),
          _read("hf_no_candidate", [(200, DCOV)], 541)]
    names = [r.name for r in R]
    assert len(set(names)) == len(names)
    return tuple(R)


@functools.lru_cache(maxsize=None)
def expected():
    """Per read of reads(), the oracle's dict(wall, rel, lab) as wall_path_inputs.expected() (None: the reference aborts).
    A read shorter than K has no k-mer and so no position to call find_wall on: its labels are the oracle's
    (classify_read: the N's the reference prints, ClassPro.c:209-226), its interval records are empty by definition."""
    O = L.tables().O
    out, empty = [], None
    for r in reads():
        if len(r.prof) == 0:
            out.append(O.classify_read(r.seq, r.prof))
            continue
        l, rc = O.seq_context(r.seq)
        try:
            iv = O.find_wall(r.prof, l, rc)
        except RuntimeError:
            out.append(None)
            continue
        rel = O.find_rel_intvl(iv, r.prof, l, rc)
        empty = dict(wall=iv[:0], rel=(rel[0][:0], rel[1][:0]))
        out.append(dict(wall=iv, rel=rel, lab=O.classify_read(r.seq, r.prof)))
    return tuple(dict(empty, lab=e) if isinstance(e, bytes) else e for e in out)

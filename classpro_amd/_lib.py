"""Loader for the C-ABI library (classpro_amd/libclasspro_amd.so, built from csrc/ by build.py).

Fails loudly when the library is missing: there is no CPU or PyTorch fallback for the hot path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CLASSPRO_AMD_LIB") or os.path.join(_HERE, "libclasspro_amd.so")   # env: diagnostic builds only

# every symbol include/classpro_amd.h declares
SYMBOLS = [
    "cp_last_error", "cp_version", "cp_hist_covs", "cp_params_create", "cp_params_destroy",
    "cp_params_export", "cp_decode_profile", "cp_workspace_create", "cp_workspace_destroy",
    "cp_workspace_bytes", "cp_classify_batch", "cp_workspace_check", "cp_run_stages", "cp_get_counts",
    "cp_get_intervals", "cp_get_rel_asgn", "cp_get_bitmap", "cp_seq_context", "cp_scan_candidates",
    "cp_encode_profile", "cp_decode_profiles", "cp_params_create_model", "cp_params_create_pe", "cp_load_error_model", "cp_unpack_bases",
    "cp_find_seeds_batch", "cp_get_rep_masks", "cp_rep_masks_capacity", "cp_params_tables", "cp_pack_bases", "cp_pack_labels", "cp_unpack_labels", "cp_math_eval", "cp_pack_bases_batch",
    "cp_label_runs", "cp_label_runs_capacity", "cp_expand_label_runs",
    "cp_kmer_table_create", "cp_kmer_table_destroy", "cp_kmer_table_add", "cp_kmer_table_stats",
    "cp_kmer_table_consensus", "cp_kmer_table_export",
    "cp_kmer_counts_create", "cp_kmer_counts_destroy", "cp_kmer_counts_add", "cp_kmer_counts_profiles",
    "cp_kmer_counts_hist", "cp_kmer_counts_stats", "cp_kmer_counts_rel_labels",
    "cp_kmer_counts_create_filtered", "cp_kmer_counts_mark", "cp_kmer_counts_filter_stats",
    "cp_kmer_counts_sort", "cp_kmer_sorted_destroy", "cp_kmer_sorted_size", "cp_kmer_sorted_bytes",
    "cp_kmer_sorted_arrays", "cp_kmer_sorted_ktab", "cp_ktab_ibyte", "cp_ktab_tile",
    "cp_kmer_table_sort", "cp_kmer_table_class_hist",
    "cp_kmer_sorted_load_begin", "cp_kmer_sorted_load_records", "cp_kmer_sorted_load_end", "cp_kmer_sorted_find",
    "cp_kmer_sorted_profiles",
    "cp_kmer_sorted_combine", "cp_kmer_sorted_hist",
    "cp_kmer_sorted_read_hits", "cp_bin_call",
    "cp_kmer_sorted_read_runs", "cp_run_blocks",
    "cp_kmer_sorted_read_fixes", "cp_apply_fixes",
    "cp_kmer_sorted_compare_hist", "cp_kmer_qv",
    "cp_kmer_sorted_het_pairs",
    "cp_kmer_counts_add_keys", "cp_kmer_sorted_het_sites", "cp_kmer_sorted_read_links", "cp_phase_forest",
    "cp_kmer_sorted_phase_split",
    "cp_kmer_sorted_unitigs", "cp_unitigs_count", "cp_unitigs_bases", "cp_unitigs_arrays", "cp_unitigs_destroy", "cp_unitig_n50",
    "cp_kmer_sorted_unitig_links", "cp_unitig_graph_links", "cp_unitig_graph_arrays", "cp_unitig_graph_destroy",
    "cp_kmer_sorted_read_paths", "cp_count_nonzero",
    "cp_kmer_sorted_unitig_prune",
    "cp_threshold_labels", "cp_acc_create", "cp_acc_destroy", "cp_acc_add", "cp_acc_read",
]

_lib = None


class KmerStats(C.Structure):
    """cp_kmer_stats of include/classpro_amd.h."""
    _fields_ = [("n_kmers", C.c_int64), ("n_skipped", C.c_int64), ("n_distinct", C.c_int64), ("n_unanimous", C.c_int64),
                ("label_total", C.c_int64 * 4), ("cns_total", C.c_int64 * 4), ("s_fixed_hi", C.c_uint64),
                ("s_fixed_lo", C.c_uint64), ("consistency", C.c_double), ("slots", C.c_int64), ("bytes", C.c_int64),
                ("growths", C.c_int64)]


class KmerCountStats(C.Structure):
    """cp_kmer_count_stats of include/classpro_amd.h."""
    _fields_ = [("n_kmers", C.c_int64), ("n_skipped", C.c_int64), ("n_distinct", C.c_int64), ("slots", C.c_int64),
                ("bytes", C.c_int64), ("growths", C.c_int64)]


class KmerFilterStats(C.Structure):
    """cp_kmer_filter_stats of include/classpro_amd.h."""
    _fields_ = [("filter_bits", C.c_int64), ("filter_bytes", C.c_int64), ("n_marked", C.c_int64),
                ("n_counted", C.c_int64), ("n_table_keys", C.c_int64), ("n_outside", C.c_int64), ("n_false", C.c_int64)]


class AccStats(C.Structure):
    """cp_acc_stats of include/classpro_amd.h."""
    _fields_ = [("cfm", (C.c_int64 * 4) * 4), ("ntot", C.c_int64), ("ncor", C.c_int64), ("nfne", C.c_int64),
                ("ntot_normal", C.c_int64), ("ncor_normal", C.c_int64), ("nfne_normal", C.c_int64),
                ("ntot_repeat", C.c_int64), ("ncor_repeat", C.c_int64), ("nfne_repeat", C.c_int64),
                ("n_reads", C.c_int64), ("n_reads_filtered", C.c_int64), ("n_invalid", C.c_int64)]


# the error codes of include/classpro_amd.h
CP_OK, CP_EINVAL, CP_ENOPEAK, CP_ERCOV, CP_EHIP, CP_EOVERFLOW, CP_ENOMEM = 0, -1, -2, -3, -4, -5, -6


class ClassProError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("classpro_amd error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "classpro_amd: %s not found. Build it with `python -m classpro_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    # The Python layer shares device memory and streams with torch, so both must sit on ONE HIP runtime: torch's
    # (it ships its own libamdhip64) has to be in the process first -- loaded after ours, it comes up as a second
    # runtime and every later HIP call of this library answers "no ROCm-capable device".
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.cp_last_error.restype = C.c_char_p
    L.cp_version.restype = C.c_char_p
    L.cp_hist_covs.argtypes = [vp, i32, i32, i64, i64, i32, C.POINTER(i32), C.POINTER(i32)]
    L.cp_params_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.cp_params_create_model.argtypes = [i32, i32, i32, i32, C.c_char_p, C.POINTER(vp)]
    L.cp_load_error_model.argtypes = [C.c_char_p, vp]
    L.cp_params_create_pe.argtypes = [i32, i32, i32, i32, vp, C.POINTER(vp)]
    L.cp_params_destroy.argtypes = [vp]
    L.cp_params_destroy.restype = None
    L.cp_params_export.argtypes = [vp] + [vp] * 7
    L.cp_params_tables.argtypes = [vp, vp, vp, vp]
    L.cp_math_eval.argtypes = [i32, vp, vp, vp, i64, vp]
    L.cp_label_runs.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.cp_label_runs_capacity.argtypes = [vp]
    L.cp_label_runs_capacity.restype = i64
    L.cp_expand_label_runs.argtypes = [vp, vp, i32, i32, i32, vp]
    L.cp_pack_bases.argtypes = [vp, i32, vp]
    L.cp_pack_bases_batch.argtypes = [vp, vp, i32, vp, vp, i32]
    L.cp_pack_labels.argtypes = [vp, vp, vp, i32, vp, vp]
    L.cp_unpack_labels.argtypes = [vp, i32, i32, vp]
    L.cp_decode_profile.argtypes = [vp, i64, vp, i32]
    L.cp_workspace_create.argtypes = [C.POINTER(vp)]
    L.cp_workspace_destroy.argtypes = [vp]
    L.cp_workspace_destroy.restype = None
    L.cp_workspace_bytes.argtypes = [vp]
    L.cp_workspace_bytes.restype = C.c_size_t
    L.cp_classify_batch.argtypes = [vp, vp, vp, vp, vp, vp, i32, i64, i64, vp, vp]
    L.cp_workspace_check.argtypes = [vp]
    L.cp_run_stages.argtypes = [vp, vp, vp, vp, vp, vp, i32, i64, i64, vp, i32, vp]
    L.cp_get_counts.argtypes = [vp, vp, vp, vp, vp]
    L.cp_get_intervals.argtypes = [vp, vp, vp, i64]
    L.cp_get_rel_asgn.argtypes = [vp, vp, vp, i64]
    L.cp_get_bitmap.argtypes = [vp, vp, i64]
    L.cp_seq_context.argtypes = [vp, vp, i32, i64, vp, vp, vp]
    L.cp_scan_candidates.argtypes = [vp, vp, i64, vp, vp]
    L.cp_encode_profile.argtypes = [vp, i32, vp, i64]
    L.cp_encode_profile.restype = i64
    L.cp_decode_profiles.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.cp_unpack_bases.argtypes = [vp, vp, vp, i32, vp, vp]
    L.cp_find_seeds_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i64, i64, vp, vp]
    L.cp_get_rep_masks.argtypes = [vp, vp, vp, vp, i64]
    L.cp_rep_masks_capacity.argtypes = [vp]
    L.cp_rep_masks_capacity.restype = i64
    L.cp_kmer_table_create.argtypes = [i32, i32, i64, C.POINTER(vp)]
    L.cp_kmer_table_destroy.argtypes = [vp]
    L.cp_kmer_table_destroy.restype = None
    L.cp_kmer_table_add.argtypes = [vp, vp, vp, vp, i32, i64, vp]
    L.cp_kmer_table_stats.argtypes = [vp, C.POINTER(KmerStats)]
    L.cp_kmer_table_consensus.argtypes = [vp, vp, vp, i32, i64, vp, vp]
    L.cp_kmer_table_export.argtypes = [vp, vp, vp, vp, i64]
    L.cp_kmer_table_export.restype = i64
    L.cp_kmer_counts_create.argtypes = [i32, i64, C.POINTER(vp)]
    L.cp_kmer_counts_destroy.argtypes = [vp]
    L.cp_kmer_counts_destroy.restype = None
    L.cp_kmer_counts_add.argtypes = [vp, vp, vp, i32, i64, vp]
    L.cp_kmer_counts_profiles.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp]
    L.cp_kmer_counts_hist.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.cp_kmer_counts_stats.argtypes = [vp, C.POINTER(KmerCountStats)]
    L.cp_kmer_counts_rel_labels.argtypes = [vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]
    L.cp_kmer_counts_create_filtered.argtypes = [i32, i64, i64, C.POINTER(vp)]
    L.cp_kmer_counts_mark.argtypes = [vp, vp, vp, i32, i64, vp]
    L.cp_kmer_counts_filter_stats.argtypes = [vp, C.POINTER(KmerFilterStats)]
    L.cp_kmer_counts_sort.argtypes = [vp, i64, vp, C.POINTER(vp)]
    L.cp_kmer_sorted_destroy.argtypes = [vp]
    L.cp_kmer_sorted_destroy.restype = None
    L.cp_kmer_sorted_size.argtypes = [vp]
    L.cp_kmer_sorted_size.restype = i64
    L.cp_kmer_sorted_bytes.argtypes = [vp]
    L.cp_kmer_sorted_bytes.restype = i64
    L.cp_kmer_sorted_arrays.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.cp_kmer_sorted_ktab.argtypes = [vp, i64, i64, vp, vp, vp]
    L.cp_ktab_ibyte.argtypes = [i32]
    L.cp_ktab_tile.argtypes = []
    L.cp_kmer_table_sort.argtypes = [vp, i32, i64, i32, vp, C.POINTER(vp)]
    L.cp_kmer_table_class_hist.argtypes = [vp, vp, vp, vp]
    L.cp_kmer_sorted_load_begin.argtypes = [i32, vp, C.POINTER(vp)]
    L.cp_kmer_sorted_load_records.argtypes = [vp, i64, vp, vp]
    L.cp_kmer_sorted_load_end.argtypes = [vp, vp]
    L.cp_kmer_sorted_find.argtypes = [vp, vp, vp, i64, vp, vp]
    L.cp_kmer_sorted_profiles.argtypes = [vp, i32, vp, vp, vp, i32, i64, vp, vp, vp]
    L.cp_kmer_sorted_combine.argtypes = [vp, vp, i32, i32, vp, vp, vp, C.POINTER(vp)]
    L.cp_kmer_sorted_hist.argtypes = [vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.cp_kmer_sorted_read_hits.argtypes = [vp, vp, i32, vp, vp, vp, i32, i64, vp, vp]
    L.cp_bin_call.argtypes = [vp, i64, i64, i64, i32]
    L.cp_kmer_sorted_read_runs.argtypes = [vp, vp, i32, vp, C.c_uint, C.c_uint, vp, vp, i32, i64, vp, i64, vp, C.POINTER(i64), vp]
    L.cp_run_blocks.argtypes = [vp, i64, i64, vp, C.POINTER(i64)]
    L.cp_run_blocks.restype = i64
    L.cp_kmer_sorted_read_fixes.argtypes = [vp, i32, vp, i32, vp, vp, i32, i64, vp, i64, vp, C.POINTER(i64), vp, vp]
    L.cp_apply_fixes.argtypes = [vp, vp, i32, i64, i32, vp, vp, vp, i64, vp, C.POINTER(i64), vp]
    L.cp_kmer_sorted_compare_hist.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.cp_kmer_qv.argtypes = [i32, i64, i64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.cp_kmer_sorted_het_pairs.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, C.POINTER(vp)]
    L.cp_kmer_counts_add_keys.argtypes = [vp, vp, vp, i64, vp]
    L.cp_kmer_sorted_het_sites.argtypes = [vp, vp, vp, C.POINTER(i64), vp, vp]
    L.cp_kmer_sorted_read_links.argtypes = [vp, vp, i32, vp, vp, i32, i64, vp, i64, C.POINTER(i64), vp, vp]
    L.cp_phase_forest.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    L.cp_kmer_sorted_phase_split.argtypes = [vp, vp, vp, vp, i64, i32, vp, C.POINTER(vp)]
    L.cp_kmer_sorted_unitigs.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.cp_unitigs_count.argtypes = [vp]
    L.cp_unitigs_count.restype = i64
    L.cp_unitigs_bases.argtypes = [vp]
    L.cp_unitigs_bases.restype = i64
    L.cp_unitigs_arrays.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.cp_unitigs_destroy.argtypes = [vp]
    L.cp_unitigs_destroy.restype = None
    L.cp_unitig_n50.argtypes = [vp, i64]
    L.cp_unitig_n50.restype = i64
    L.cp_kmer_sorted_unitig_links.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(vp)]
    L.cp_unitig_graph_links.argtypes = [vp]
    L.cp_unitig_graph_links.restype = i64
    L.cp_unitig_graph_arrays.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.cp_unitig_graph_destroy.argtypes = [vp]
    L.cp_unitig_graph_destroy.restype = None
    L.cp_kmer_sorted_read_paths.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i64, vp, i64, vp, vp, vp, vp, C.POINTER(i64), vp]
    L.cp_count_nonzero.argtypes = [vp, i64, C.POINTER(i64), vp]
    L.cp_kmer_sorted_unitig_prune.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.cp_threshold_labels.argtypes =[i32, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp]
    L.cp_acc_create.argtypes = [i32, C.c_double, C.c_double, C.POINTER(vp)]
    L.cp_acc_destroy.argtypes = [vp]
    L.cp_acc_destroy.restype = None
    L.cp_acc_add.argtypes = [vp, vp, vp, vp, i32, i64, vp]
    L.cp_acc_read.argtypes = [vp, C.POINTER(AccStats)]
    _lib = L
    return L


def check(rc):
    if rc < 0:
        raise ClassProError(rc, lib().cp_last_error().decode(errors="replace"))
    return rc

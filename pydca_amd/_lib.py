"""ctypes binding of libdca_hip.so (include/dca_hip.h).

The product has no CPU fallback: if the shared library is missing or no gfx950 device
is visible, every compute entry point raises -- it never routes to another
implementation.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DCA_LIB_PATH: an alternative build of the SAME library (kernel experiments); never a different backend
LIB_PATH = os.environ.get("DCA_LIB_PATH") or os.path.join(_HERE, "lib", "libdca_hip.so")

DCA_OK = 0
DCA_ERR_ARG, DCA_ERR_IO, DCA_ERR_RESIDUE = -1, -2, -3
DCA_ERR_NOMEM, DCA_ERR_HIP, DCA_ERR_NO_DEVICE, DCA_ERR_NOT_SPD, DCA_ERR_STATE = -4, -5, -6, -7, -8
DCA_F32, DCA_F64 = 32, 64
DCA_BIOMOLECULE_PROTEIN, DCA_BIOMOLECULE_RNA = 1, 2
CARRY_EXACT, CARRY_CHUNKED, CARRY_SERIAL = 0, 1, 2
PROTEIN, RNA = 1, 2


class DcaBackendError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libdca_hip error %d: %s" % (code, msg))
        self.code = code


class PlmStats(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("evaluations", C.c_int), ("finished", C.c_int),
                ("fx", C.c_double), ("xnorm", C.c_double), ("gnorm", C.c_double), ("step", C.c_double),
                ("seconds", C.c_double)]


class BmArgs(C.Structure):
    """dca_bm_args (include/dca_hip.h)"""
    _fields_ = [("chains", C.c_int), ("sweeps", C.c_int), ("equilibration_sweeps", C.c_int), ("seed", C.c_uint64),
                ("eta_h", C.c_double), ("eta_J", C.c_double), ("mu_h", C.c_double), ("mu_J", C.c_double),
                ("pseudocount", C.c_double), ("initial", C.c_void_p)]


class BmDecimation(C.Structure):
    """dca_bm_decimation (include/dca_hip.h)"""
    _fields_ = [("active_before", C.c_longlong), ("removed", C.c_longlong), ("active_after", C.c_longlong),
                ("threshold", C.c_double), ("removed_sum", C.c_double)]


class AisArgs(C.Structure):
    """dca_ais_args (include/dca_hip.h)"""
    _fields_ = [("chains", C.c_int), ("temperatures", C.c_int), ("betas", C.c_void_p), ("sweeps_per_temperature", C.c_int),
                ("seed", C.c_uint64), ("first_chain", C.c_uint64), ("base_fields", C.c_void_p)]


class PtArgs(C.Structure):
    """dca_pt_args (include/dca_hip.h)"""
    _fields_ = [("ladders", C.c_int), ("levels", C.c_int), ("betas", C.c_void_p), ("sweeps", C.c_int), ("swap_interval", C.c_int),
                ("seed", C.c_uint64), ("first_ladder", C.c_uint64), ("first_sweep", C.c_uint64), ("initial", C.c_void_p),
                ("initial_levels", C.c_void_p)]


class ArStats(C.Structure):
    """dca_ar_stats (include/dca_hip.h)"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("evaluations", C.c_int), ("fx", C.c_double), ("gnorm", C.c_double),
                ("seconds", C.c_double)]


class SetComparison(C.Structure):
    """dca_set_comparison (include/dca_hip.h): one entry per quantity, [0] f_i, [1] f_ij, [2] c_ij"""
    _fields_ = [(k, C.c_double * 3) for k in ("pearson", "slope", "max_abs_diff", "sxx", "syy", "sxy", "terms")]


class FilterInfo(C.Structure):
    """dca_filter_info (include/dca_hip.h)"""
    _fields_ = [("kept", C.c_int32), ("blocks", C.c_int32), ("block_rows", C.c_int32), ("tile_pairs", C.c_int64)]


class ClusterInfo(C.Structure):
    """dca_cluster_info (include/dca_hip.h)"""
    _fields_ = [("clusters", C.c_int32), ("largest", C.c_int32), ("rounds", C.c_int32), ("stored_bits", C.c_int32)]


class HopfieldArgs(C.Structure):
    """dca_hopfield_args (include/dca_hip.h)"""
    _fields_ = [("selection", C.c_int32), ("num_patterns", C.c_int32), ("num_attractive", C.c_int32), ("num_repulsive", C.c_int32),
                ("max_iterations", C.c_int32), ("tol", C.c_double), ("seed", C.c_uint64)]


class HopfieldInfo(C.Structure):
    """dca_hopfield_info (include/dca_hip.h)"""
    _fields_ = [("num_attractive", C.c_int32), ("num_repulsive", C.c_int32), ("iterations", C.c_int32 * 2), ("converged", C.c_int32 * 2)]


HOPFIELD_EXPLICIT, HOPFIELD_LIKELIHOOD = 0, 1
MF_MODEL_NONE, MF_MODEL_MEAN_FIELD, MF_MODEL_HOPFIELD = 0, 1, 2
HOPFIELD_MAX_PER_END = 64

AR_CONVERGED, AR_MAX_ITERATIONS, AR_LINE_SEARCH_FAILED = 0, 1, 2

COMM_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int)
COMM_ALL_REDUCE, COMM_REDUCE_SCATTER, COMM_ALL_GATHER = 0, 1, 2
REDUCE_HOOK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)


def build(verbose=False):
    """Compile libdca_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j", str(min(8, os.cpu_count() or 1))]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DcaBackendError(-100, "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(pydca_amd has no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i, d, sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
    sig = {
        "dca_last_error": (C.c_char_p, []),
        "dca_version": (C.c_char_p, []),
        "dca_device_count": (i, []),
        "dca_release_cached_memory": (sz, []),
        "dca_device_blocks_in_use": (sz, []),
        "dca_read_msa": (i, [C.c_char_p, i, i, vp, i, C.POINTER(i)]),
        "dca_count_msa_lines": (i, [C.c_char_p]),
        "dca_fasta_shape": (i, [C.c_char_p, C.POINTER(i), C.POINTER(i)]),
        "dca_read_fasta": (i, [C.c_char_p, i, i, vp, i, C.POINTER(i)]),
        "dca_read_fasta_alloc": (i, [C.c_char_p, i, C.POINTER(vp), C.POINTER(i), C.POINTER(i)]),
        "dca_host_free": (None, [vp]),
        "dca_read_msa_alloc": (i, [C.c_char_p, i, i, C.POINTER(vp), C.POINTER(i)]),
        "dca_create": (i, [C.POINTER(vp), i, i]),
        "dca_destroy": (None, [vp]),
        "dca_set_msa": (i, [vp, vp, i, i, i]),
        "dca_compute_weights": (i, [vp, d, i]),
        "dca_weights_work": (i, [vp, vp]),
        "dca_compute_weights_sharded": (i, [vp, d, i]),
        "dca_weights_partial_counts": (i, [vp, d, i, i, i, vp]),
        "dca_set_weight_counts": (i, [vp, vp]),
        "dca_comm_unique_id": (i, [C.c_char_p, vp]),
        "dca_comm_init": (i, [vp, C.c_char_p, vp, i, i]),
        "dca_comm_destroy": (i, [vp]),
        "dca_comm_info": (i, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "dca_plm_set_native_comm": (i, [vp, i]),
        "dca_mf_set_native_comm": (i, [vp, i]),
        "dca_set_weights": (i, [vp, vp]),
        "dca_get_weights": (i, [vp, vp]),
        "dca_get_weight_counts": (i, [vp, vp]),
        "dca_get_meff": (i, [vp, C.POINTER(d)]),
        "dca_plm_configure": (i, [vp, d, d, i, i, i, i, i]),
        "dca_plm_configure_strips": (i, [vp, d, d, i, i, i]),
        "dca_plm_num_params": (sz, [i, i]),
        "dca_plm_init_x": (i, [vp]),
        "dca_plm_set_x": (i, [vp, vp, i]),
        "dca_plm_get_x": (i, [vp, vp, i]),
        "dca_plm_release": (i, [vp]),
        "dca_plm_gradient": (i, [vp, C.POINTER(d)]),
        "dca_plm_get_g": (i, [vp, vp, i]),
        "dca_plm_set_reduce_hook": (i, [vp, REDUCE_HOOK, vp]),
        "dca_mf_set_reduce_hook": (i, [vp, REDUCE_HOOK, vp]),
        "dca_di_from_arrays": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "dca_di_from_fields": (i, [vp, vp, i, vp, vp, i, i, vp]),
        "dca_plm_set_vector_sharding": (i, [vp, i, i, COMM_HOOK, vp]),
        "dca_plm_lbfgs_begin": (i, [vp, i, i]),
        "dca_plm_lbfgs_iterate": (i, [vp, i, C.POINTER(PlmStats)]),
        "dca_plm_lbfgs_end": (i, [vp]),
        "dca_mf_set_row_window": (i, [vp, i, i]),
        "dca_comm_allgather_host": (i, [vp, vp, i, vp]),
        "dca_plm_scores": (i, [vp, i, vp]),
        "dca_plm_di_scores": (i, [vp, vp, i, vp]),
        "dca_mf_di_scores": (i, [vp, i, vp]),
        "dca_plm_pair_couplings": (i, [vp, vp, i, i, vp]),
        "dca_mf_fields": (i, [vp, vp]),
        "dca_encode_sequences": (i, [C.c_char_p, vp, i, i, i, i, vp, C.POINTER(i)]),
        "dca_plm_energies": (i, [vp, vp, i, vp]),
        "dca_plm_mutation_scan": (i, [vp, vp, vp]),
        "dca_mf_energies": (i, [vp, vp, i, vp]),
        "dca_mf_mutation_scan": (i, [vp, vp, vp]),
        "dca_plm_pseudo_likelihood": (i, [vp, vp, i, vp, vp, vp]),
        "dca_mf_pseudo_likelihood": (i, [vp, vp, i, vp, vp, vp]),
        "dca_plm_sample": (i, [vp, i, i, C.c_uint64, C.c_uint64, C.c_uint64, d, vp, vp]),
        "dca_mf_sample": (i, [vp, i, i, C.c_uint64, C.c_uint64, C.c_uint64, d, vp, vp]),
        "dca_plm_sample_conditional": (i, [vp, i, i, C.c_uint64, C.c_uint64, C.c_uint64, d, vp, i, vp, i, vp]),
        "dca_mf_sample_conditional": (i, [vp, i, i, C.c_uint64, C.c_uint64, C.c_uint64, d, vp, i, vp, i, vp]),
        "dca_plm_sample_tempered": (i, [vp, C.POINTER(PtArgs), vp, vp, vp, vp, vp, vp, C.POINTER(i)]),
        "dca_mf_sample_tempered": (i, [vp, C.POINTER(PtArgs), vp, vp, vp, vp, vp, vp, C.POINTER(i)]),
        "dca_plm_ascend": (i, [vp, vp, i, vp, i, i, d, vp, vp, vp, vp, vp, vp]),
        "dca_mf_ascend": (i, [vp, vp, i, vp, i, i, d, vp, vp, vp, vp, vp, vp]),
        "dca_philox4x32_10": (i, [vp, vp, vp]),
        "dca_plm_interaction_energies": (i, [vp, i, vp, i, vp, i, vp, vp, i, i, vp]),
        "dca_mf_interaction_energies": (i, [vp, i, vp, i, vp, i, vp, vp, i, i, vp]),
        "dca_assign_partners": (i, [vp, i, i, vp, vp, vp]),
        "dca_ar_configure": (i, [vp, d, d]),
        "dca_ar_num_params": (sz, [i, i]),
        "dca_ar_init_x": (i, [vp]),
        "dca_ar_set_x": (i, [vp, vp]),
        "dca_ar_get_x": (i, [vp, vp]),
        "dca_ar_gradient": (i, [vp, C.POINTER(d)]),
        "dca_ar_get_g": (i, [vp, vp]),
        "dca_ar_fit": (i, [vp, i, d, C.POINTER(ArStats)]),
        "dca_ar_log_probabilities": (i, [vp, vp, i, vp, vp, vp]),
        "dca_ar_sample": (i, [vp, i, C.c_uint64, C.c_uint64, vp]),
        "dca_ar_release": (i, [vp]),
        "dca_ar_epistasis": (i, [vp, vp, vp, vp]),
        "dca_ar_epistatic_scores": (i, [vp, vp, i, vp]),
        "dca_plm_bm_begin": (i, [vp, C.POINTER(BmArgs)]),
        "dca_plm_bm_iterate": (i, [vp, i, vp]),
        "dca_plm_bm_freqs": (i, [vp, i, vp, vp]),
        "dca_plm_bm_chains": (i, [vp, vp]),
        "dca_plm_bm_end": (i, [vp]),
        "dca_plm_bm_set_mask": (i, [vp, vp]),
        "dca_plm_bm_get_mask": (i, [vp, vp]),
        "dca_plm_bm_decimate": (i, [vp, C.c_longlong, vp, C.POINTER(BmDecimation)]),
        "dca_plm_zero_sum_gauge": (i, [vp]),
        "dca_hamming_nearest": (i, [vp, vp, i, vp, i, i, vp, vp, vp]),
        "dca_sequence_statistics": (i, [vp, vp, i, vp, vp, C.POINTER(SetComparison)]),
        "dca_alignment_statistics": (i, [vp, vp, vp]),
        "dca_identity_filter": (i, [vp, vp, i, i, vp, vp, vp, C.POINTER(FilterInfo)]),
        "dca_identity_clusters": (i, [vp, vp, i, i, vp, vp, C.POINTER(ClusterInfo)]),
        "dca_three_site_values": (i, [vp, vp, i, vp, i, vp, vp, vp, vp]),
        "dca_three_site_scan": (i, [vp, vp, i, i, i, vp, vp, vp, C.POINTER(i)]),
        "dca_pca_fit": (i, [vp, i, d, i, C.c_uint64, vp, vp, vp, vp, C.POINTER(d), C.POINTER(i), C.POINTER(i)]),
        "dca_pca_project": (i, [vp, vp, i, i, vp, vp, vp]),
        "dca_plm_ais": (i, [vp, C.POINTER(AisArgs), vp, C.POINTER(d), vp]),
        "dca_mf_ais": (i, [vp, C.POINTER(AisArgs), vp, C.POINTER(d), vp]),
        "dca_ais_estimate": (i, [vp, i, d, C.POINTER(d), C.POINTER(d), C.POINTER(d)]),
        "dca_mf_pair_couplings": (i, [vp, vp, i, i, vp]),
        "dca_mf_single_site_freqs": (i, [vp, vp]),
        "dca_mf_pair_site_freqs": (i, [vp, vp]),
        "dca_mf_corr_mat": (i, [vp, d, vp]),
        "dca_mf_couplings": (i, [vp, vp]),
        "dca_mf_scores": (i, [vp, i, vp]),
        "dca_mf_run": (i, [vp, d, i, vp, vp]),
        "dca_mf_corr_from_freqs": (i, [vp, vp, vp, i, i, vp]),
        "dca_spd_inverse": (i, [vp, vp, i, vp]),
        "dca_mf_hopfield_fit": (i, [vp, d, C.POINTER(HopfieldArgs), vp, vp, vp, vp, vp, C.POINTER(HopfieldInfo)]),
        "dca_mf_model_kind": (i, [vp, C.POINTER(i)]),
        "dca_mf_hopfield_couplings": (i, [vp, vp]),
        "dca_hopfield_project": (i, [vp, vp, i, i, vp, vp]),
        "dca_dense_apply": (i, [vp, vp, i, i, vp, i, vp]),
        "dca_comm_abort": (i, [vp]),
        "dca_plm_run": (i, [vp, vp, i, vp]),
        "dca_scores_order": (i, [vp, vp, i]),
        "dca_sw_scores": (i, [C.c_char_p, i, C.c_char_p, vp, i, vp, i, i, vp]),
        "dca_sw_align": (i, [C.c_char_p, i, C.c_char_p, i, vp, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.c_char_p,
                             C.c_char_p, C.POINTER(i)]),
        "dca_profile_align": (i, [vp, vp, i, i, vp, vp, i, i, i, vp, vp, i, vp, vp]),
        "dca_profile_align_last_scratch": (i, [vp, C.POINTER(C.c_ulonglong)]),
        "dca_get_msa": (i, [vp, vp]),
        "dca_sw_scores_device": (i, [vp, C.c_char_p, i, C.c_char_p, vp, i, vp, i, i, vp]),
        "dca_set_profiling": (i, [vp, i]),
        "dca_set_profiling_only": (i, [vp, C.c_char_p]),
        "dca_get_kernel_time": (i, [vp, C.c_char_p, C.POINTER(d), C.POINTER(i)]),
        "dca_reset_kernel_times": (i, [vp]),
        "plmdcaBackend": (C.c_void_p, [C.c_ushort, C.c_ushort, C.c_char_p, C.c_uint, C.c_float, C.c_float, C.c_float,
                                       C.c_uint, C.c_uint, C.c_bool]),
        "freeFieldsAndCouplings": (None, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


EXPORTS = ["dca_weights_work", "dca_compute_weights_sharded", "dca_weights_partial_counts", "dca_set_weight_counts", "dca_comm_unique_id",
           "dca_comm_init", "dca_comm_destroy", "dca_comm_abort", "dca_comm_info", "dca_plm_set_native_comm", "dca_mf_set_native_comm",
           "dca_last_error", "dca_version", "dca_device_count", "dca_release_cached_memory", "dca_device_blocks_in_use", "dca_read_msa", "dca_count_msa_lines", "dca_read_msa_alloc", "dca_mf_set_row_window", "dca_comm_allgather_host", "dca_fasta_shape", "dca_read_fasta", "dca_read_fasta_alloc", "dca_host_free", "dca_create",
           "dca_destroy", "dca_set_msa", "dca_compute_weights", "dca_set_weights", "dca_get_weights",
           "dca_get_weight_counts", "dca_get_meff", "dca_plm_configure", "dca_plm_configure_strips", "dca_plm_num_params", "dca_plm_init_x",
           "dca_plm_set_x", "dca_plm_get_x", "dca_plm_release", "dca_plm_gradient", "dca_plm_get_g", "dca_plm_set_reduce_hook", "dca_mf_set_reduce_hook", "dca_di_from_arrays", "dca_di_from_fields", "dca_plm_set_vector_sharding",
           "dca_plm_lbfgs_begin", "dca_plm_lbfgs_iterate", "dca_plm_lbfgs_end", "dca_plm_scores", "dca_plm_di_scores",
           "dca_mf_di_scores", "dca_plm_pair_couplings", "dca_mf_fields", "dca_mf_pair_couplings",
           "dca_encode_sequences", "dca_plm_energies", "dca_plm_mutation_scan", "dca_mf_energies", "dca_mf_mutation_scan",
           "dca_plm_pseudo_likelihood", "dca_mf_pseudo_likelihood",
           "dca_plm_sample", "dca_mf_sample", "dca_plm_sample_conditional", "dca_mf_sample_conditional",
           "dca_plm_sample_tempered", "dca_mf_sample_tempered", "dca_plm_ascend", "dca_mf_ascend", "dca_philox4x32_10",
           "dca_plm_interaction_energies", "dca_mf_interaction_energies", "dca_assign_partners",
           "dca_ar_configure", "dca_ar_num_params", "dca_ar_init_x", "dca_ar_set_x", "dca_ar_get_x", "dca_ar_gradient", "dca_ar_get_g",
           "dca_ar_fit", "dca_ar_log_probabilities", "dca_ar_sample", "dca_ar_release",
           "dca_ar_epistasis", "dca_ar_epistatic_scores",
           "dca_plm_bm_begin", "dca_plm_bm_iterate", "dca_plm_bm_freqs", "dca_plm_bm_chains", "dca_plm_bm_end",
           "dca_plm_bm_set_mask", "dca_plm_bm_get_mask", "dca_plm_bm_decimate", "dca_plm_zero_sum_gauge",
           "dca_plm_ais", "dca_mf_ais", "dca_ais_estimate",
           "dca_hamming_nearest", "dca_sequence_statistics", "dca_alignment_statistics",
           "dca_identity_filter", "dca_identity_clusters",
           "dca_three_site_values", "dca_three_site_scan", "dca_pca_fit", "dca_pca_project",
           "dca_mf_single_site_freqs",
           "dca_mf_pair_site_freqs", "dca_mf_corr_mat", "dca_mf_couplings", "dca_mf_scores", "dca_mf_run",
           "dca_mf_corr_from_freqs", "dca_spd_inverse", "dca_mf_hopfield_fit", "dca_mf_model_kind", "dca_mf_hopfield_couplings",
           "dca_hopfield_project", "dca_dense_apply", "dca_sw_scores", "dca_sw_align", "dca_profile_align",
           "dca_profile_align_last_scratch", "dca_get_msa", "dca_sw_scores_device", "dca_scores_order", "dca_set_profiling", "dca_set_profiling_only", "dca_get_kernel_time",
           "dca_reset_kernel_times", "dca_plm_run", "plmdcaBackend", "freeFieldsAndCouplings"]


def three_site_elements(elements, L, q):
    """elements of the three-site entries -> int32[T, 6], rows (i, j, k, a, b, c) checked as dca_three_site_values checks them
    (0 <= i < j < k < L, states in 0 .. q-1); ValueError otherwise.  Needs no device."""
    try:
        raw = np.asarray(elements)
    except Exception:
        raise ValueError("elements must be an integer array of shape (T, 6)")
    if raw.dtype == object or raw.ndim != 2 or raw.shape[1] != 6 or not (np.issubdtype(raw.dtype, np.integer) or raw.dtype == np.bool_):
        raise ValueError("elements must be an integer array of shape (T, 6) with rows (i, j, k, a, b, c), not %s of shape %s"
                         % (raw.dtype, raw.shape))
    if raw.shape[0] < 1:
        raise ValueError("elements must hold at least one row")
    big = raw.astype(np.int64)
    s, st = big[:, :3], big[:, 3:]
    bad = (s[:, 0] < 0) | (s[:, 0] >= s[:, 1]) | (s[:, 1] >= s[:, 2]) | (s[:, 2] >= L)
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError("element %d names the sites %s; they must satisfy 0 <= i < j < k < %d" % (k, tuple(int(v) for v in s[k]), L))
    bad = ((st < 0) | (st >= q)).any(axis=1)
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError("element %d names the states %s; states are 0 .. %d" % (k, tuple(int(v) for v in st[k]), q - 1))
    return np.ascontiguousarray(big, dtype=np.int32)


PCA_SLAB = 1024            # DCA_PCA_SLAB (include/dca_hip.h): sequences per slab of the back-projection's fixed summation order
PCA_MAX_COMPONENTS = 64


def pca_arguments(num_components, tolerance, max_iterations, seed, L, q):
    """The arguments of dca_pca_fit, checked as the library checks them -> (k, tol, max_iterations, seed); ValueError
    otherwise.  Needs no device."""
    def integer(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer, not %r" % (name, v))
        return int(v)
    k, it, sd = integer("num_components", num_components), integer("max_iterations", max_iterations), integer("seed", seed)
    cap = min(PCA_MAX_COMPONENTS, int(L) * int(q))
    if k < 1 or k > cap:
        raise ValueError("num_components must be between 1 and min(%d, L q) = %d, not %d" % (PCA_MAX_COMPONENTS, cap, k))
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)):
        raise ValueError("tolerance must be a number, not %r" % (tolerance,))
    tol = float(tolerance)
    if not (tol > 0.0) or not np.isfinite(tol):
        raise ValueError("tolerance must be a finite number > 0, not %r" % (tolerance,))
    if it < 1:
        raise ValueError("max_iterations must be >= 1, not %d" % it)
    if sd < 0 or sd >= 1 << 64:
        raise ValueError("seed must be in 0 .. 2^64 - 1, not %d" % sd)
    return k, tol, it, sd


def hopfield_arguments(num_patterns, num_attractive, num_repulsive, tolerance, max_iterations, seed, L, q):
    """The arguments of dca_mf_hopfield_fit, checked as the library checks them -> (selection, p, a, r, tol, max_iterations, seed);
    ValueError with the reason otherwise.  Either num_patterns (the likelihood selection) or num_attractive / num_repulsive (one
    may be left None for 0)."""
    n = int(L) * (int(q) - 1)

    def count(name, v, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s must be an integer" % name)
        if not lo <= v <= hi:
            raise ValueError("%s must be between %d and %d" % (name, lo, hi))
        return int(v)

    explicit = num_attractive is not None or num_repulsive is not None
    if explicit and num_patterns is not None:
        raise ValueError("give num_patterns or num_attractive / num_repulsive, not both")
    if not explicit and num_patterns is None:
        raise ValueError("give num_patterns or num_attractive / num_repulsive")
    if explicit:
        a = count("num_attractive", 0 if num_attractive is None else num_attractive, 0, HOPFIELD_MAX_PER_END)
        r = count("num_repulsive", 0 if num_repulsive is None else num_repulsive, 0, HOPFIELD_MAX_PER_END)
        if not 1 <= a + r <= n:
            raise ValueError("num_attractive + num_repulsive must be between 1 and L (q - 1) = %d" % n)
        sel, p = HOPFIELD_EXPLICIT, 0
    else:
        p = count("num_patterns", num_patterns, 1, min(2 * HOPFIELD_MAX_PER_END, n))
        sel, a, r = HOPFIELD_LIKELIHOOD, 0, 0
    if isinstance(tolerance, (bool, str)) or not isinstance(tolerance, (int, float, np.integer, np.floating)) \
            or not (np.isfinite(tolerance) and tolerance > 0):
        raise ValueError("tolerance must be a finite number > 0")
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, (int, np.integer)) or max_iterations < 1:
        raise ValueError("max_iterations must be >= 1")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    return sel, p, a, r, float(tolerance), int(max_iterations), int(seed)


def ais_schedule(temperatures, betas=None):
    """The annealing schedule of the AIS entries: betas None -> None (the library forms k / K), else float64[K + 1], checked as
    dca_plm_ais checks it (finite, strictly increasing from 0 to 1); ValueError otherwise."""
    K = int(temperatures)
    if K < 1:
        raise ValueError("the number of temperatures must be >= 1, not %r" % (temperatures,))
    if betas is None:
        return None
    b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    if b.size != K + 1:
        raise ValueError("betas must hold K + 1 = %d values, not %d" % (K + 1, b.size))
    if not np.all(np.isfinite(b)) or b[0] != 0.0 or b[-1] != 1.0 or not np.all(np.diff(b) > 0):
        raise ValueError("betas must be finite and strictly increasing from 0 to 1")
    return b


def ais_base_fields(base_fields, L, q):
    """None -> None (the model's own fields), else float64[L, q] of finite values; ValueError otherwise."""
    if base_fields is None:
        return None
    h = np.ascontiguousarray(base_fields, dtype=np.float64)
    if h.size != L * q:
        raise ValueError("the base fields must be an L x q = %d x %d array, not of shape %s" % (L, q, h.shape))
    h = h.reshape(L, q)
    if not np.all(np.isfinite(h)):
        raise ValueError("the base fields must be finite")
    return h


def ais_estimate(log_weights, log_z0):
    """dca_ais_estimate -> (log_z, ess, stderr_log_z)"""
    w = np.ascontiguousarray(log_weights, dtype=np.float64).reshape(-1)
    lz, ess, se = C.c_double(0), C.c_double(0), C.c_double(0)
    check(lib().dca_ais_estimate(_ptr(w) if w.size else None, int(w.size), float(log_z0), C.byref(lz), C.byref(ess), C.byref(se)))
    return lz.value, ess.value, se.value


class PlmArgs(C.Structure):
    """dca_plm_args (include/dca_hip.h)"""
    _fields_ = [("biomolecule", C.c_int), ("msa_file", C.c_char_p), ("msa", C.c_void_p), ("num_seqs", C.c_int), ("seqs_len", C.c_int),
                ("seqid", C.c_float), ("lambda_h", C.c_float), ("lambda_J", C.c_float), ("max_iterations", C.c_int), ("precision", C.c_int),
                ("devices", C.POINTER(C.c_int)), ("num_devices", C.c_int), ("exchange_scheme", C.c_int), ("rccl_path", C.c_char_p),
                ("verbose", C.c_int)]


def plm_run(biomolecule, seqs_len, msa_file=None, msa=None, seqid=0.8, lambda_h=1.0, lambda_J=20.0, max_iterations=100, precision=DCA_F32,
            devices=None, exchange_scheme=0, rccl_path=None, verbose=False, dtype=np.float32):
    """dca_plm_run, the library's one-call plmDCA entry (what a C host would call) -> (x, PlmStats).  msa: uint8[N, L] codes."""
    q = 21 if biomolecule == DCA_BIOMOLECULE_PROTEIN else 5
    a = PlmArgs()
    a.biomolecule, a.seqs_len = int(biomolecule), int(seqs_len)
    a.msa_file = os.fsencode(msa_file) if msa_file else None
    keep = None
    if msa is not None:
        keep = np.ascontiguousarray(msa, dtype=np.uint8)
        a.msa, a.num_seqs = keep.ctypes.data, int(keep.shape[0])
    a.seqid, a.lambda_h, a.lambda_J = float(seqid), float(lambda_h), float(lambda_J)
    a.max_iterations, a.precision, a.exchange_scheme, a.verbose = int(max_iterations), int(precision), int(exchange_scheme), int(bool(verbose))
    devs = (C.c_int * len(devices))(*devices) if devices else None
    a.devices, a.num_devices = devs, len(devices) if devices else 0
    a.rccl_path = os.fsencode(rccl_path) if rccl_path else None
    L = int(seqs_len)
    x = np.zeros(L * q + L * (L - 1) // 2 * q * q, dtype=dtype)
    st = PlmStats()
    check(lib().dca_plm_run(C.byref(a), _ptr(x), DCA_F64 if np.dtype(dtype) == np.float64 else DCA_F32, C.byref(st)))
    del keep
    return x, st


def comm_unique_id(rccl_path=None):
    """128-byte RCCL unique id (rank 0 makes it, every rank passes it to Context.comm_init)."""
    buf = C.create_string_buffer(128)
    check(lib().dca_comm_unique_id(os.fsencode(rccl_path) if rccl_path else None, buf))
    return buf.raw


def release_cached_memory():
    """Return the library's cached device blocks (>= 1 MiB, kept across contexts) to the driver -> bytes released."""
    return int(lib().dca_release_cached_memory())


def device_blocks_in_use():
    """Device blocks the library has allocated and not yet released, over all contexts of the process."""
    return int(lib().dca_device_blocks_in_use())


def check(rc):
    if rc != DCA_OK:
        raise DcaBackendError(rc, lib().dca_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def read_msa(path, biomolecule, L):
    """Reference C++ reader semantics (plmdca_numerics.cpp:685-767) -> (uint8[N',L], raw_count)."""
    l = lib()
    rows, raw = C.c_void_p(), C.c_int(0)
    n = l.dca_read_msa_alloc(os.fsencode(path), int(biomolecule), int(L), C.byref(rows), C.byref(raw))     # one pass over the file
    try:
        if n < 0:
            check(n)
        out = np.empty((n, int(L)), dtype=np.uint8)
        if n:
            C.memmove(out.ctypes.data, rows, out.nbytes)
        return out, raw.value
    finally:
        if rows:
            l.dca_host_free(rows)


def fasta_shape(path):
    """(records with residues, their common length) of a FASTA file, natively (dca_fasta_shape)."""
    l = lib()
    n, L = C.c_int(0), C.c_int(0)
    rc = l.dca_fasta_shape(os.fsencode(path), C.byref(n), C.byref(L))
    if rc == DCA_ERR_ARG:
        raise ValueError(l.dca_last_error().decode("utf-8", "replace"))
    check(rc)
    return n.value, L.value


def read_fasta(path, biomolecule):
    """The mfDCA path's FASTA semantics (fasta_reader.py:81-163) natively -> (uint8[N', L] with 0-based codes, gap = q-1;
    number of records read).  Raises DcaBackendError(DCA_ERR_RESIDUE) for files with non-ASCII bytes (the caller then
    reads in text mode itself), ValueError for empty files / unequal lengths like the Python reader."""
    l = lib()
    rows, L, raw = C.c_void_p(), C.c_int(0), C.c_int(0)
    k = l.dca_read_fasta_alloc(os.fsencode(path), int(biomolecule), C.byref(rows), C.byref(L), C.byref(raw))     # one pass
    try:
        if k == DCA_ERR_ARG:
            raise ValueError(l.dca_last_error().decode("utf-8", "replace"))
        if k < 0:
            check(k)
        if raw.value == 0:
            raise ValueError("No sequences found in %s" % path)
        out = np.empty((k, L.value), dtype=np.uint8)
        C.memmove(out.ctypes.data, rows, out.nbytes)
    finally:
        if rows:
            l.dca_host_free(rows)
    return out, raw.value


class EncodeError(ValueError):
    """A query record that dca_encode_sequences rejected: .record is its 0-based index, .code DCA_ERR_ARG (length) or
    DCA_ERR_RESIDUE (a character the plm reader's table lacks)."""

    def __init__(self, code, record, msg):
        super().__init__(msg)
        self.code, self.record = code, record


def encode_sequences(seqs, biomolecule, L, table):
    """Aligned strings -> uint8[n, L] codes (0-based, gap = q-1), in order, duplicates kept (dca_encode_sequences).
    table 0: the plm reader's residue table, 1: the mf reader's (unknown characters are the gap)."""
    enc = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    offs = np.zeros(len(enc) + 1, dtype=np.int32)
    if enc:
        offs[1:] = np.cumsum([len(e) for e in enc])
    out = np.zeros((len(enc), int(L)), dtype=np.uint8)
    bad = C.c_int(-1)
    rc = lib().dca_encode_sequences(b"".join(enc), _ptr(offs), len(enc), int(biomolecule), int(table), int(L), _ptr(out), C.byref(bad))
    if rc in (DCA_ERR_ARG, DCA_ERR_RESIDUE) and bad.value >= 0:
        raise EncodeError(rc, bad.value, lib().dca_last_error().decode("utf-8", "replace"))
    check(rc)
    return out


def philox4x32_10(ctr, key):
    """Philox4x32-10 of the samplers on the host (dca_philox4x32_10): 4 counter words, 2 key words -> uint32[4]."""
    c = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
    out = np.zeros(4, dtype=np.uint32)
    check(lib().dca_philox4x32_10(_ptr(c), _ptr(k), _ptr(out)))
    return out


GAUGES = {"as_stored": 0, "zero_sum": 1}


def assign_partners(E):
    """Maximum-weight matching of size min(nr, nc) in the 2-D array E with gaps (dca_assign_partners; host only) ->
    (col_of_row int32[nr], -1 = unassigned; total; gaps float64[nr]: +inf where the pair cannot be replaced, 0 for an
    unassigned row).  Under exact ties any optimal matching may come back."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    if E.ndim != 2:
        raise ValueError("E must be a 2-D array")
    nr, nc = E.shape
    col = np.full(nr, -1, dtype=np.int32)
    gap = np.zeros(nr, dtype=np.float64)
    total = C.c_double(0.0)
    check(lib().dca_assign_partners(_ptr(E) if E.size else None, nr, nc, _ptr(col) if nr else None, C.byref(total),
                                    _ptr(gap) if nr else None))
    return col, total.value, gap


class Context:
    """One GPU, one stream, one alignment (include/dca_hip.h `dca_ctx`)."""

    def __init__(self, device=0, precision=DCA_F32):
        self._l = lib()
        self._h = C.c_void_p()
        check(self._l.dca_create(C.byref(self._h), int(device), int(precision)))
        self.precision = precision
        self.N = self.L = self.q = 0
        self._hook = None

    def close(self):
        if self._h:
            self._l.dca_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- alignment / weights
    def set_msa(self, X, q):
        X = np.ascontiguousarray(X, dtype=np.uint8)
        self.N, self.L, self.q = X.shape[0], X.shape[1], int(q)
        check(self._l.dca_set_msa(self._h, _ptr(X), self.N, self.L, self.q))

    def compute_weights(self, seqid, compare_precision=DCA_F32):
        check(self._l.dca_compute_weights(self._h, float(seqid), int(compare_precision)))
        return self.weights()

    def weights_work(self):
        """(wave x 32-site groups the last compute_weights launch compared, the same without the early exit, bit planes per group)"""
        out = np.zeros(3, dtype=np.uint64)
        check(self._l.dca_weights_work(self._h, _ptr(out)))
        return int(out[0]), int(out[1]), int(out[2])

    def set_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (self.N,)
        check(self._l.dca_set_weights(self._h, _ptr(w)))

    def compute_weights_sharded(self, seqid, compare_precision=DCA_F32):
        """Weights with the comparisons divided over the ranks of the context's communicator (comm_init first).
        Same default compare precision as compute_weights, so the two give the same counts at threshold ties."""
        check(self._l.dca_compute_weights_sharded(self._h, float(seqid), int(compare_precision)))
        return self.weights()

    def weights_partial_counts(self, seqid, compare_precision, part, parts):
        """Part `part` of `parts` of the identity comparisons -> partial integer counts (sum the parts, then set_weight_counts)."""
        c = np.zeros(self.N, dtype=np.uint32)
        check(self._l.dca_weights_partial_counts(self._h, float(seqid), int(compare_precision), int(part), int(parts), _ptr(c)))
        return c

    def set_weight_counts(self, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if counts.shape != (self.N,):
            raise ValueError("counts must have one entry per sequence")
        check(self._l.dca_set_weight_counts(self._h, _ptr(counts)))

    # ---- native collectives (RCCL on the context's stream)
    def comm_init(self, unique_id, world, rank, rccl_path=None):
        self._comm_id = bytes(unique_id)
        check(self._l.dca_comm_init(self._h, os.fsencode(rccl_path) if rccl_path else None, self._comm_id, int(world), int(rank)))

    def comm_destroy(self):
        check(self._l.dca_comm_destroy(self._h))

    def comm_abort(self):
        """From a watchdog thread: a peer died -- make this context's pending collectives fail (ncclCommAbort)."""
        check(self._l.dca_comm_abort(self._h))

    def comm_info(self):
        """(world, rank) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)."""
        w, r = C.c_int(0), C.c_int(0)
        check(self._l.dca_comm_info(self._h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def plm_set_native_comm(self, mode):
        """0 off, 1 all-reduce of g and fx per evaluation, 2 sharded optimiser vectors (RCCL reduce-scatter / all-gather),
        3 sharded optimiser vectors by direct exchange (grouped send / recv + rank-ordered local sum)."""
        check(self._l.dca_plm_set_native_comm(self._h, int(mode)))

    def mf_set_row_window(self, first, count):
        """Count only the sequences [first, first + count) of the (whole) alignment this context holds; count < 0: all."""
        check(self._l.dca_mf_set_row_window(self._h, int(first), int(count)))

    def comm_allgather(self, values):
        """Every rank's `values` (a few doubles) on every rank, in rank order: array [world, len(values)].  Collective."""
        mine = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        world = self.comm_info()[0]
        out = np.zeros((world, mine.size), dtype=np.float64)
        check(self._l.dca_comm_allgather_host(self._h, _ptr(mine), mine.size, _ptr(out)))
        return out

    def mf_set_native_comm(self, on=True):
        check(self._l.dca_mf_set_native_comm(self._h, int(bool(on))))

    def weights(self):
        w = np.zeros(self.N, dtype=np.float64)
        check(self._l.dca_get_weights(self._h, _ptr(w)))
        return w

    def weight_counts(self):
        c = np.zeros(self.N, dtype=np.uint32)
        check(self._l.dca_get_weight_counts(self._h, _ptr(c)))
        return c

    def meff(self):
        v = C.c_double(0)
        check(self._l.dca_get_meff(self._h, C.byref(v)))
        return v.value

    # ---- plmDCA
    def num_params(self):
        return int(self._l.dca_plm_num_params(self.L, self.q))

    def plm_configure(self, lambda_h, lambda_J, carry_mode=CARRY_CHUNKED, chunk=0, warmup=0, halo=0, add_regulariser=1):
        check(self._l.dca_plm_configure(self._h, float(lambda_h), float(lambda_J), int(carry_mode), int(chunk),
                                        int(warmup), int(halo), int(add_regulariser)))

    def plm_configure_strips(self, lambda_h, lambda_J, carry_mode=CARRY_CHUNKED, chunk=0, warmup=0):
        """Column-strip decomposition over the context's communicator (comm_init first; the context holds the whole
        alignment): this rank takes the columns of its share of the sites.  plm_get_x / plm_get_g / plm_scores are collective."""
        check(self._l.dca_plm_configure_strips(self._h, float(lambda_h), float(lambda_J), int(carry_mode), int(chunk), int(warmup)))

    def plm_init_x(self):
        check(self._l.dca_plm_init_x(self._h))

    def plm_set_x(self, x):
        x = np.ascontiguousarray(x)
        dt = DCA_F32 if x.dtype == np.float32 else DCA_F64
        if dt == DCA_F64:
            x = np.ascontiguousarray(x, dtype=np.float64)
        check(self._l.dca_plm_set_x(self._h, _ptr(x), dt))

    def plm_get_x(self, dtype=np.float32):
        x = np.zeros(self.num_params(), dtype=dtype)
        check(self._l.dca_plm_get_x(self._h, _ptr(x), DCA_F32 if x.dtype == np.float32 else DCA_F64))
        return x

    def plm_release(self):
        """Frees the plmDCA engine of this context (tables, vectors); alignment, weights and communicator stay."""
        check(self._l.dca_plm_release(self._h))

    def plm_get_g(self, dtype=np.float32):
        g = np.zeros(self.num_params(), dtype=dtype)
        check(self._l.dca_plm_get_g(self._h, _ptr(g), DCA_F32 if g.dtype == np.float32 else DCA_F64))
        return g

    def plm_gradient(self):
        fx = C.c_double(0)
        check(self._l.dca_plm_gradient(self._h, C.byref(fx)))
        return fx.value

    def plm_set_reduce_hook(self, pyfunc):
        """pyfunc(g_dev_ptr:int, count:int, dtype:int, fx_dev_ptr:int) -> 0 on success."""
        def tramp(user, g_dev, count, dtype, fx_dev):
            try:
                return int(pyfunc(g_dev, count, dtype, fx_dev) or 0)
            except Exception:   # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._hook = REDUCE_HOOK(tramp) if pyfunc is not None else C.cast(None, REDUCE_HOOK)
        check(self._l.dca_plm_set_reduce_hook(self._h, self._hook, None))

    def plm_set_vector_sharding(self, rank, world, pyfunc):
        """Shard the optimiser's P-vectors over `world` ranks; pyfunc(op, buf_dev_ptr, count, dtype) -> 0
        runs the collectives (COMM_ALL_REDUCE / COMM_REDUCE_SCATTER / COMM_ALL_GATHER, in place on
        device memory).  pyfunc=None switches back to replicated vectors."""
        def tramp(user, op, buf, count, dtype):
            try:
                return int(pyfunc(op, buf, count, dtype) or 0)
            except Exception:   # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._comm = COMM_HOOK(tramp) if pyfunc is not None else C.cast(None, COMM_HOOK)
        check(self._l.dca_plm_set_vector_sharding(self._h, int(rank), int(world), self._comm, None))

    def mf_set_reduce_hook(self, pyfunc):
        """Same hook protocol for the mfDCA pair counts: pyfunc(craw_dev_ptr, count, 64, meff_dev_ptr)."""
        def tramp(user, g_dev, count, dtype, fx_dev):
            try:
                return int(pyfunc(g_dev, count, dtype, fx_dev) or 0)
            except Exception:   # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._mf_hook = REDUCE_HOOK(tramp) if pyfunc is not None else C.cast(None, REDUCE_HOOK)
        check(self._l.dca_mf_set_reduce_hook(self._h, self._mf_hook, None))

    def plm_lbfgs_begin(self, max_iterations, verbose=False):
        check(self._l.dca_plm_lbfgs_begin(self._h, int(max_iterations), int(bool(verbose))))

    def plm_lbfgs_end(self):
        check(self._l.dca_plm_lbfgs_end(self._h))

    def plm_lbfgs_iterate(self, iterations):
        st = PlmStats()
        check(self._l.dca_plm_lbfgs_iterate(self._h, int(iterations), C.byref(st)))
        return st

    def plm_scores(self, apc=True):
        out = np.zeros(self.L * (self.L - 1) // 2, dtype=np.float64)
        check(self._l.dca_plm_scores(self._h, int(bool(apc)), _ptr(out)))
        return out

    def plm_di_scores(self, reg_fi, apc=False):
        reg_fi = np.ascontiguousarray(reg_fi, dtype=np.float64)
        if reg_fi.shape != (self.L, self.q):
            raise ValueError("reg_fi must be L x q")
        out = np.zeros(self.L * (self.L - 1) // 2, dtype=np.float64)
        check(self._l.dca_plm_di_scores(self._h, _ptr(reg_fi), int(bool(apc)), _ptr(out)))
        return out

    def di_from_arrays(self, couplings, layout, reg_fi, L, q, want_fields=False, want_di=True):
        """layout 1: n x n couplings matrix; 2: gap-stripped 1-D blocks.  -> (fields [pairs,2,q] | None, di [pairs] | None)"""
        couplings = np.ascontiguousarray(couplings, dtype=np.float64)
        reg_fi = np.ascontiguousarray(reg_fi, dtype=np.float64)
        npairs = L * (L - 1) // 2
        fields = np.zeros((npairs, 2, q), dtype=np.float64) if want_fields else None
        di = np.zeros(npairs, dtype=np.float64) if want_di else None
        check(self._l.dca_di_from_arrays(self._h, _ptr(couplings), int(layout), _ptr(reg_fi), int(L), int(q),
                                         _ptr(fields) if want_fields else None, _ptr(di) if want_di else None))
        return fields, di

    def di_from_fields(self, couplings, layout, reg_fi, fields_ij, L, q):
        """DI from the caller's two-site model fields [pairs, 2, q] (no fixed point is run)."""
        couplings = np.ascontiguousarray(couplings, dtype=np.float64)
        reg_fi = np.ascontiguousarray(reg_fi, dtype=np.float64)
        npairs = L * (L - 1) // 2
        fields_ij = np.ascontiguousarray(fields_ij, dtype=np.float64)
        if fields_ij.shape != (npairs, 2, q):
            raise ValueError("fields_ij must have shape (L(L-1)/2, 2, q)")
        di = np.zeros(npairs, dtype=np.float64)
        check(self._l.dca_di_from_fields(self._h, _ptr(couplings), int(layout), _ptr(reg_fi), _ptr(fields_ij), int(L), int(q), _ptr(di)))
        return di

    def scores_order(self):
        """Pair indices of the last score vector, best first (device radix sort, stable)."""
        out = np.zeros(self.L * (self.L - 1) // 2, dtype=np.int32)
        check(self._l.dca_scores_order(self._h, _ptr(out), int(out.size)))
        return out

    def _pair_couplings(self, fn, pairs, shift):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        qm = self.q - 1
        out = np.zeros((pairs.shape[0], qm, qm), dtype=np.float64)
        if pairs.shape[0]:
            check(fn(self._h, _ptr(pairs), int(pairs.shape[0]), int(bool(shift)), _ptr(out)))
        return out

    def plm_pair_couplings(self, pairs, shift=True):
        return self._pair_couplings(self._l.dca_plm_pair_couplings, pairs, shift)

    # ---- mfDCA
    def mf_pair_couplings(self, pairs, shift=True):
        return self._pair_couplings(self._l.dca_mf_pair_couplings, pairs, shift)

    def mf_fields(self):
        out = np.zeros((self.L, self.q - 1), dtype=np.float64)
        check(self._l.dca_mf_fields(self._h, _ptr(out)))
        return out

    # ---- Potts energies (energy.hip): X uint8[n, L] codes < q -> float64[n]; wild type uint8[L] -> float64[L, q]
    def _energies(self, fn, X):
        X = np.ascontiguousarray(X, dtype=np.uint8).reshape(-1, self.L)
        out = np.zeros(X.shape[0], dtype=np.float64)
        check(fn(self._h, _ptr(X), int(X.shape[0]), _ptr(out)))
        return out

    def _mutation_scan(self, fn, wildtype):
        w = np.ascontiguousarray(wildtype, dtype=np.uint8).reshape(-1)
        if w.size != self.L:
            raise ValueError("the wild type must have L = %d codes" % self.L)
        out = np.zeros((self.L, self.q), dtype=np.float64)
        check(fn(self._h, _ptr(w), _ptr(out)))
        return out

    def plm_energies(self, X):
        return self._energies(self._l.dca_plm_energies, X)

    def plm_mutation_scan(self, wildtype):
        return self._mutation_scan(self._l.dca_plm_mutation_scan, wildtype)

    def mf_energies(self, X):
        return self._energies(self._l.dca_mf_energies, X)

    def mf_mutation_scan(self, wildtype):
        return self._mutation_scan(self._l.dca_mf_mutation_scan, wildtype)

    # ---- site conditionals and pseudo-log-likelihoods (pll.hip): X uint8[n, L] codes < q -> pll float64[n], or a tuple with
    # site float64[n, L] and / or cond float64[n, L, q] (log P(s_i = a | s_-i))
    def _pseudo_likelihood(self, fn, X, per_site, conditionals):
        X = np.ascontiguousarray(X, dtype=np.uint8).reshape(-1, self.L)
        n = X.shape[0]
        pll = np.zeros(n, dtype=np.float64)
        site = np.zeros((n, self.L), dtype=np.float64) if per_site else None
        cond = np.zeros((n, self.L, self.q), dtype=np.float64) if conditionals else None
        check(fn(self._h, _ptr(X), int(n), _ptr(pll), None if site is None or not n else _ptr(site),
                 None if cond is None or not n else _ptr(cond)))
        if not per_site and not conditionals:
            return pll
        return (pll,) + tuple(v for v in (site, cond) if v is not None)

    def plm_pseudo_likelihood(self, X, per_site=False, conditionals=False):
        return self._pseudo_likelihood(self._l.dca_plm_pseudo_likelihood, X, per_site, conditionals)

    def mf_pseudo_likelihood(self, X, per_site=False, conditionals=False):
        return self._pseudo_likelihood(self._l.dca_mf_pseudo_likelihood, X, per_site, conditionals)

    # ---- Gibbs sampling (sample.hip): n chains, `sweeps` systematic sweeps -> uint8[n, L] codes
    def _sample(self, fn, n, sweeps, seed, beta, initial, first_chain, first_sweep):
        n = int(n)
        init = None
        if initial is not None:
            init = np.ascontiguousarray(initial, dtype=np.uint8)
            if init.shape != (n, self.L):
                raise ValueError("initial must be uint8[%d, %d]" % (n, self.L))
        out = np.zeros((max(n, 0), self.L), dtype=np.uint8)
        check(fn(self._h, n, int(sweeps), int(seed), int(first_chain), int(first_sweep), float(beta),
                 None if init is None else _ptr(init), _ptr(out)))
        return out

    def plm_sample(self, n, sweeps, seed=0, beta=1.0, initial=None, first_chain=0, first_sweep=0):
        return self._sample(self._l.dca_plm_sample, n, sweeps, seed, beta, initial, first_chain, first_sweep)

    def mf_sample(self, n, sweeps, seed=0, beta=1.0, initial=None, first_chain=0, first_sweep=0):
        return self._sample(self._l.dca_mf_sample, n, sweeps, seed, beta, initial, first_chain, first_sweep)

    # ---- conditional Gibbs sampling (sample_conditional.hip): the sites of free_sites (strictly ascending) are resampled, every
    # other site keeps the chain's own row of `initial` (uint8[n, L], required) -> uint8[n, L] codes
    def _sample_conditional(self, fn, initial, free_sites, sweeps, seed, beta, random_start, first_chain, first_sweep):
        init = np.ascontiguousarray(initial, dtype=np.uint8)
        if init.ndim != 2 or init.shape[1] != self.L:
            raise ValueError("initial must be uint8[n, %d]" % self.L)
        sites = np.ascontiguousarray(free_sites, dtype=np.int32).reshape(-1)
        n = init.shape[0]
        out = np.zeros((n, self.L), dtype=np.uint8)
        check(fn(self._h, n, int(sweeps), int(seed), int(first_chain), int(first_sweep), float(beta),
                 _ptr(sites) if sites.size else None, int(sites.size), _ptr(init) if n else None, int(bool(random_start)),
                 _ptr(out) if n else None))
        return out

    def plm_sample_conditional(self, initial, free_sites, sweeps, seed=0, beta=1.0, random_start=True, first_chain=0, first_sweep=0):
        return self._sample_conditional(self._l.dca_plm_sample_conditional, initial, free_sites, sweeps, seed, beta, random_start,
                                        first_chain, first_sweep)

    def mf_sample_conditional(self, initial, free_sites, sweeps, seed=0, beta=1.0, random_start=True, first_chain=0, first_sweep=0):
        return self._sample_conditional(self._l.dca_mf_sample_conditional, initial, free_sites, sweeps, seed, beta, random_start,
                                        first_chain, first_sweep)

    # ---- inter-protein energies (interaction.hip): sites [0, split) are protein A, the rest protein B; XA uint8[nA, split],
    # XB uint8[nB, L - split]; group g holds the rows offsets_a[g] .. offsets_a[g+1] of XA and offsets_b[g] .. offsets_b[g+1] of XB
    # -> a list of float64[nA_g, nB_g] blocks; with no offsets one dense float64[nA, nB]
    def _interaction_energies(self, fn, XA, XB, split, offsets_a, offsets_b, gauge):
        if gauge not in GAUGES:
            raise ValueError("gauge must be one of %s" % sorted(GAUGES))
        split = int(split)
        XA = np.ascontiguousarray(XA, dtype=np.uint8)
        XB = np.ascontiguousarray(XB, dtype=np.uint8)
        if XA.ndim != 2 or XB.ndim != 2 or (0 < split < self.L and (XA.shape[1] != split or XB.shape[1] != self.L - split)):
            raise ValueError("XA must be uint8[nA, %d] and XB uint8[nB, %d]" % (split, self.L - split))
        if (offsets_a is None) != (offsets_b is None):
            raise ValueError("give both offsets or neither")
        dense = offsets_a is None
        oa = np.array([0, XA.shape[0]], dtype=np.int32) if dense else np.ascontiguousarray(offsets_a, dtype=np.int32).reshape(-1)
        ob = np.array([0, XB.shape[0]], dtype=np.int32) if dense else np.ascontiguousarray(offsets_b, dtype=np.int32).reshape(-1)
        if oa.size != ob.size:
            raise ValueError("offsets_a and offsets_b must have the same length")
        G = oa.size - 1
        na, nb = np.diff(oa).astype(np.int64), np.diff(ob).astype(np.int64)
        sizes = na * nb if G >= 1 and (na >= 0).all() and (nb >= 0).all() else np.zeros(max(G, 0), dtype=np.int64)
        out = np.zeros(int(sizes.sum()), dtype=np.float64)
        check(fn(self._h, split, _ptr(XA) if XA.size else None, XA.shape[0], _ptr(XB) if XB.size else None, XB.shape[0],
                 _ptr(oa), _ptr(ob), G, GAUGES[gauge], _ptr(out) if out.size else None))
        if dense:
            return out.reshape(XA.shape[0], XB.shape[0])
        ends = np.cumsum(sizes)
        return [out[e - z:e].reshape(int(a), int(b)) for e, z, a, b in zip(ends, sizes, na, nb)]

    def plm_interaction_energies(self, XA, XB, split, offsets_a=None, offsets_b=None, gauge="zero_sum"):
        return self._interaction_energies(self._l.dca_plm_interaction_energies, XA, XB, split, offsets_a, offsets_b, gauge)

    def mf_interaction_energies(self, XA, XB, split, offsets_a=None, offsets_b=None, gauge="zero_sum"):
        return self._interaction_energies(self._l.dca_mf_interaction_energies, XA, XB, split, offsets_a, offsets_b, gauge)

    # ---- replica-exchange Gibbs sampling (tempered.hip): `ladders` ladders of len(betas) walkers, walker r of ladder m at row
    # m R + r; betas strictly increasing -> dict: codes uint8[n, L], levels int32[n], energies float64[n] (E of the final codes),
    # attempts / accepts uint64[R - 1], rounds and, with trace, trace float64[rounds, ladders, R] (E of the walker at each level
    # before every exchange round)
    def _sample_tempered(self, fn, ladders, betas, sweeps, swap_interval, seed, first_ladder, first_sweep, initial, initial_levels, trace):
        M = int(ladders)
        b = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
        R = int(b.size)
        n = max(M, 0) * R
        init = lev = None
        if initial is not None:
            init = np.ascontiguousarray(initial, dtype=np.uint8)
            if init.shape != (n, self.L):
                raise ValueError("initial must be uint8[%d, %d]" % (n, self.L))
        if initial_levels is not None:
            lev = np.ascontiguousarray(initial_levels, dtype=np.int32).reshape(-1)
            if lev.size != n:
                raise ValueError("initial_levels must hold ladders x levels = %d values, not %d" % (n, lev.size))
        sweeps, swap_interval, first_sweep = int(sweeps), int(swap_interval), int(first_sweep)
        rounds = (first_sweep + sweeps) // swap_interval - first_sweep // swap_interval if swap_interval > 0 and sweeps >= 0 else 0
        args = PtArgs(M, R, b.ctypes.data if R else None, sweeps, swap_interval, int(seed), int(first_ladder), first_sweep,
                      init.ctypes.data if init is not None and n else None, lev.ctypes.data if lev is not None and n else None)
        out = np.zeros((n, self.L), dtype=np.uint8)
        levels = np.zeros(n, dtype=np.int32)
        energies = np.zeros(n, dtype=np.float64)
        attempts = np.zeros(max(R - 1, 0), dtype=np.uint64)
        accepts = np.zeros(max(R - 1, 0), dtype=np.uint64)
        tr = np.zeros((max(rounds, 0), max(M, 0), R), dtype=np.float64) if trace else None
        done = C.c_int(0)
        check(fn(self._h, C.byref(args), _ptr(out) if n else None, _ptr(levels) if n else None, _ptr(energies) if n else None,
                 _ptr(attempts) if attempts.size else None, _ptr(accepts) if accepts.size else None,
                 _ptr(tr) if tr is not None and tr.size else None, C.byref(done)))
        res = {"codes": out, "levels": levels, "energies": energies, "attempts": attempts, "accepts": accepts, "rounds": int(done.value)}
        if trace:
            res["trace"] = tr
        return res

    def plm_sample_tempered(self, ladders, betas, sweeps, swap_interval=1, seed=0, first_ladder=0, first_sweep=0, initial=None,
                            initial_levels=None, trace=False):
        return self._sample_tempered(self._l.dca_plm_sample_tempered, ladders, betas, sweeps, swap_interval, seed, first_ladder,
                                     first_sweep, initial, initial_levels, trace)

    def mf_sample_tempered(self, ladders, betas, sweeps, swap_interval=1, seed=0, first_ladder=0, first_sweep=0, initial=None,
                           initial_levels=None, trace=False):
        return self._sample_tempered(self._l.dca_mf_sample_tempered, ladders, betas, sweeps, swap_interval, seed, first_ladder,
                                     first_sweep, initial, initial_levels, trace)

    # ---- greedy ascent to local maxima (ascent.hip): every row of X (uint8[n, L]) climbs by the best single mutation of a free
    # site (free_sites strictly ascending, every other site keeps the row's code) until none gains more than min_gain or max_steps
    # moves are made -> dict: codes uint8[n, L], steps int32[n], converged bool[n], gains float64[n] and, with paths, path
    # int32[n, max_steps, 2] (site, new state; -1 past steps) and path_gains float64[n, max_steps]
    def _ascend(self, fn, X, free_sites, max_steps, min_gain, paths):
        X = np.ascontiguousarray(X, dtype=np.uint8)
        if X.ndim != 2 or X.shape[1] != self.L:
            raise ValueError("X must be uint8[n, %d]" % self.L)
        sites = np.ascontiguousarray(free_sites, dtype=np.int32).reshape(-1)
        max_steps = 4 * int(sites.size) if max_steps is None else int(max_steps)
        n = X.shape[0]
        out = np.zeros((n, self.L), dtype=np.uint8)
        steps = np.zeros(n, dtype=np.int32)
        conv = np.zeros(n, dtype=np.uint8)
        gains = np.zeros(n, dtype=np.float64)
        path = np.zeros((n, max(max_steps, 0), 2), dtype=np.int32) if paths else None
        pgain = np.zeros((n, max(max_steps, 0)), dtype=np.float64) if paths else None
        some = n > 0
        check(fn(self._h, _ptr(X) if some else None, n, _ptr(sites) if sites.size else None, int(sites.size), max_steps, float(min_gain),
                 _ptr(out) if some else None, _ptr(steps) if some else None, _ptr(conv) if some else None, _ptr(gains) if some else None,
                 _ptr(path) if paths and path.size else None, _ptr(pgain) if paths and pgain.size else None))
        res = {"codes": out, "steps": steps, "converged": conv.astype(bool), "gains": gains}
        if paths:
            res["path"], res["path_gains"] = path, pgain
        return res

    def plm_ascend(self, X, free_sites, max_steps=None, min_gain=0.0, paths=False):
        return self._ascend(self._l.dca_plm_ascend, X, free_sites, max_steps, min_gain, paths)

    def mf_ascend(self, X, free_sites, max_steps=None, min_gain=0.0, paths=False):
        return self._ascend(self._l.dca_mf_ascend, X, free_sites, max_steps, min_gain, paths)

    # ---- autoregressive model (ardca.hip): float64 x in the plm layout, sites in the alignment's column order
    def ar_configure(self, lambda_h, lambda_J):
        check(self._l.dca_ar_configure(self._h, float(lambda_h), float(lambda_J)))

    def ar_num_params(self):
        return int(self._l.dca_ar_num_params(self.L, self.q))

    def ar_init_x(self):
        check(self._l.dca_ar_init_x(self._h))

    def ar_set_x(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.ar_num_params():
            raise ValueError("x must hold %d values, not %d" % (self.ar_num_params(), x.size))
        check(self._l.dca_ar_set_x(self._h, _ptr(x)))

    def ar_get_x(self):
        x = np.zeros(self.ar_num_params(), dtype=np.float64)
        check(self._l.dca_ar_get_x(self._h, _ptr(x)))
        return x

    def ar_gradient(self):
        fx = C.c_double(0)
        check(self._l.dca_ar_gradient(self._h, C.byref(fx)))
        return fx.value

    def ar_get_g(self):
        g = np.zeros(self.ar_num_params(), dtype=np.float64)
        check(self._l.dca_ar_get_g(self._h, _ptr(g)))
        return g

    def ar_fit(self, max_iterations=1000, epsilon=1e-5):
        """L-BFGS from the current x -> dict(status, iterations, evaluations, fx, gnorm, seconds); status AR_CONVERGED,
        AR_MAX_ITERATIONS or AR_LINE_SEARCH_FAILED."""
        st = ArStats()
        check(self._l.dca_ar_fit(self._h, int(max_iterations), float(epsilon), C.byref(st)))
        return {k: getattr(st, k) for k, _t in ArStats._fields_}

    def ar_log_probabilities(self, X, per_site=False, conditionals=False):
        """log P(s) of codes X (n x L, model order) -> float64[n], or a tuple with float64[n, L] site values (per_site) and
        float64[n, L, q] conditionals (conditionals)."""
        return self._pseudo_likelihood(self._l.dca_ar_log_probabilities, X, per_site, conditionals)

    def ar_sample(self, n, seed=0, first_chain=0):
        """n ancestral samples -> uint8[n, L] codes (model order)"""
        n = int(n)
        out = np.zeros((max(n, 0), self.L), dtype=np.uint8)
        check(self._l.dca_ar_sample(self._h, n, int(seed), int(first_chain), _ptr(out)))
        return out

    def ar_release(self):
        check(self._l.dca_ar_release(self._h))

    def _ar_wildtype(self, wildtype):
        w = np.ascontiguousarray(wildtype, dtype=np.uint8).reshape(-1)
        if w.size != self.L:
            raise ValueError("the wild type must hold L = %d codes, not %d" % (self.L, w.size))
        return w

    def ar_epistasis(self, wildtype, eps=True, single=True):
        """dca_ar_epistasis of the wild type (L codes, model order) -> (eps float64[pairs, q, q] in pair order, a at the earlier
        site, or None; d float64[L, q] or None)."""
        w = self._ar_wildtype(wildtype)
        e = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), dtype=np.float64) if eps else None
        d = np.zeros((self.L, self.q), dtype=np.float64) if single else None
        check(self._l.dca_ar_epistasis(self._h, _ptr(w), _ptr(e) if eps else None, _ptr(d) if single else None))
        return e, d

    def ar_epistatic_scores(self, wildtype, apc=True):
        """dca_ar_epistatic_scores -> float64[pairs] in pair order over the model's sites; scores_order() ranks them."""
        w = self._ar_wildtype(wildtype)
        out = np.zeros(self.L * (self.L - 1) // 2, dtype=np.float64)
        check(self._l.dca_ar_epistatic_scores(self._h, _ptr(w), int(bool(apc)), _ptr(out)))
        return out

    # ---- Boltzmann machine learning of x (boltzmann.hip): persistent chains on the device, records (eps_h, eps_J, pearson)
    def plm_bm_begin(self, chains, sweeps, equilibration_sweeps, seed=0, eta_h=0.0, eta_J=0.0, mu_h=0.0, mu_J=0.0,
                     pseudocount=0.0, initial=None):
        init = None
        if initial is not None:
            init = np.ascontiguousarray(initial, dtype=np.uint8)
            if init.shape != (int(chains), self.L):
                raise ValueError("initial must be uint8[%d, %d]" % (int(chains), self.L))
        args = BmArgs(int(chains), int(sweeps), int(equilibration_sweeps), int(seed), float(eta_h), float(eta_J), float(mu_h),
                      float(mu_J), float(pseudocount), None if init is None else init.ctypes.data)
        check(self._l.dca_plm_bm_begin(self._h, C.byref(args)))
        self._bm_chains = int(chains)

    def plm_bm_iterate(self, iterations):
        """-> float64[iterations, 3]: (eps_h, eps_J, pearson) of every iteration"""
        out = np.zeros((max(int(iterations), 0), 3), dtype=np.float64)
        check(self._l.dca_plm_bm_iterate(self._h, int(iterations), _ptr(out) if out.size else None))
        return out

    def plm_bm_freqs(self, which):
        """which 0: the regularised data frequencies; 1: the chains' frequencies of the last iteration
        -> (float64[L, q], float64[pairs, q, q])"""
        fi = np.zeros((self.L, self.q), dtype=np.float64)
        fij = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), dtype=np.float64)
        check(self._l.dca_plm_bm_freqs(self._h, int(which), _ptr(fi), _ptr(fij)))
        return fi, fij

    def plm_bm_chains(self):
        out = np.zeros((getattr(self, "_bm_chains", 0), self.L), dtype=np.uint8)
        check(self._l.dca_plm_bm_chains(self._h, _ptr(out)))
        return out

    def plm_bm_end(self):
        check(self._l.dca_plm_bm_end(self._h))

    # ---- sparse bmDCA (decimation.hip): the run's mask on the couplings, their decimation, the zero-sum gauge of x
    def plm_bm_set_mask(self, mask):
        """mask: pairs*q*q values 0 / 1 (any shape), 1 = active; x becomes +0 at the zeros"""
        m = np.ascontiguousarray(mask, dtype=np.uint8).ravel()
        n = self.L * (self.L - 1) // 2 * self.q * self.q
        if m.size != n:
            raise ValueError("mask must hold %d values, not %d" % (n, m.size))
        check(self._l.dca_plm_bm_set_mask(self._h, _ptr(m)))

    def plm_bm_get_mask(self):
        """-> uint8[pairs, q, q], all ones if the run has no mask"""
        out = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), dtype=np.uint8)
        check(self._l.dca_plm_bm_get_mask(self._h, _ptr(out)))
        return out

    def plm_bm_decimate(self, remove, return_scores=False):
        """Removes the `remove` active coupling elements of lowest score -> dict(active_before, removed, active_after,
        threshold, removed_sum), with return_scores also 'scores': float64[pairs, q, q] (-1 at removed elements)"""
        info = BmDecimation()
        sc = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), dtype=np.float64) if return_scores else None
        check(self._l.dca_plm_bm_decimate(self._h, int(remove), _ptr(sc) if sc is not None else None, C.byref(info)))
        out = {k: getattr(info, k) for k, _t in BmDecimation._fields_}
        if return_scores:
            out["scores"] = sc
        return out

    def plm_zero_sum_gauge(self):
        check(self._l.dca_plm_zero_sum_gauge(self._h))

    # ---- a sequence set against the alignment (distance.hip, set_stats.hip): model-free, nothing of the context changes
    def hamming_nearest(self, Q=None, R=None, skip_same_index=False, return_index=True, return_histogram=True):
        """Hamming distance of every row of Q (uint8[nq, L]; None: the reference set itself) to its nearest row of R (uint8[nr, L];
        None: the context's alignment) -> (int32[nq] distances, int32[nq] smallest nearest index or None, uint64[L + 1] histogram
        of all compared pairs or None).  skip_same_index leaves the pairs k == m out; a query without partner gets -1, -1."""
        q_ = None if Q is None else np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, self.L)
        r_ = None if R is None else np.ascontiguousarray(R, dtype=np.uint8).reshape(-1, self.L)
        nr = self.N if r_ is None else r_.shape[0]
        nq = nr if q_ is None else q_.shape[0]
        dist = np.zeros(nq, dtype=np.int32)
        index = np.zeros(nq, dtype=np.int32) if return_index else None
        hist = np.zeros(self.L + 1, dtype=np.uint64) if return_histogram else None
        check(self._l.dca_hamming_nearest(self._h, None if q_ is None else _ptr(q_), int(nq), None if r_ is None else _ptr(r_), int(nr),
                                          int(bool(skip_same_index)), _ptr(dist), None if index is None else _ptr(index),
                                          None if hist is None else _ptr(hist)))
        return dist, index, hist

    def sequence_statistics(self, Q, frequencies=True, compare=True):
        """Unweighted frequencies of the rows of Q (uint8[n, L]) and their comparison with the alignment's weighted ones ->
        (fi float64[L, q] or None, fij float64[pairs, q, q] or None, dict of the dca_set_comparison fields (3-vectors) or None)"""
        Q = np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, self.L)
        fi = np.zeros((self.L, self.q), dtype=np.float64) if frequencies else None
        fij = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), dtype=np.float64) if frequencies else None
        cmp_ = SetComparison() if compare else None
        check(self._l.dca_sequence_statistics(self._h, _ptr(Q), int(Q.shape[0]), None if fi is None else _ptr(fi),
                                              None if fij is None else _ptr(fij), None if cmp_ is None else C.byref(cmp_)))
        out = None if cmp_ is None else {k: np.array(getattr(cmp_, k), dtype=np.float64) for k, _t in SetComparison._fields_}
        return fi, fij, out

    def alignment_statistics(self):
        """The alignment's weighted frequencies of all q states, no pseudocount -> (float64[L, q], float64[pairs, q, q])"""
        fi = np.zeros((self.L, self.q), dtype=np.float64)
        fij = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), dtype=np.float64)
        check(self._l.dca_alignment_statistics(self._h, _ptr(fi), _ptr(fij)))
        return fi, fij

    # ---- redundancy filter and identity clusters (redundancy.hip): model-free, nothing of the context changes
    def _identity_rows(self, X):
        x_ = None if X is None else np.ascontiguousarray(X, dtype=np.uint8).reshape(-1, self.L)
        return x_, (self.N if x_ is None else x_.shape[0])

    def identity_filter(self, min_identical, X=None, order=None, return_representatives=True):
        """The sequential greedy filter at `min_identical` identical sites over the rows X (uint8[n, L]; None: the context's
        alignment) visited in `order` (a permutation; None: ascending) -> (uint8[n] keep, int32[n] representative or None,
        dict of the dca_filter_info fields)"""
        x_, n = self._identity_rows(X)
        o_ = None if order is None else np.ascontiguousarray(order, dtype=np.int32).reshape(-1)
        if o_ is not None and o_.size != n:
            raise ValueError("order must hold %d entries, not %d" % (n, o_.size))
        keep = np.zeros(n, dtype=np.uint8)
        rep = np.zeros(n, dtype=np.int32) if return_representatives else None
        info = FilterInfo()
        check(self._l.dca_identity_filter(self._h, None if x_ is None else _ptr(x_), int(n), int(min_identical),
                                          None if o_ is None else _ptr(o_), _ptr(keep), None if rep is None else _ptr(rep), C.byref(info)))
        return keep, rep, {k: int(getattr(info, k)) for k, _t in FilterInfo._fields_}

    def identity_clusters(self, min_identical, X=None, return_degrees=True):
        """Connected components of the similar pairs (single linkage) -> (int32[n] labels: the smallest row index of the
        component, int32[n] degrees (the row itself included) or None, dict of the dca_cluster_info fields)"""
        x_, n = self._identity_rows(X)
        label = np.zeros(n, dtype=np.int32)
        degree = np.zeros(n, dtype=np.int32) if return_degrees else None
        info = ClusterInfo()
        check(self._l.dca_identity_clusters(self._h, None if x_ is None else _ptr(x_), int(n), int(min_identical), _ptr(label),
                                            None if degree is None else _ptr(degree), C.byref(info)))
        return label, degree, {k: int(getattr(info, k)) for k, _t in ClusterInfo._fields_}

    # ---- profile alignment (align.hip): needs the context only, no alignment
    def profile_align(self, match, del_open, del_extend, ins_open, ins_extend, mode, seqs, traceback=True):
        """match: int32[Lp, A]; del_open, del_extend: int32[Lp]; seqs: a list of uint8 code arrays (codes < A) ->
        (int32[n] scores, int32[n, Lp] residue_at or None without traceback).  mode: DCA_ALIGN_LOCAL or DCA_ALIGN_GLOCAL."""
        m = np.ascontiguousarray(match, dtype=np.int32)
        if m.ndim != 2:
            raise ValueError("match must be a 2-D array (Lp x A)")
        Lp, A = m.shape
        do, de = np.ascontiguousarray(del_open, dtype=np.int32).reshape(-1), np.ascontiguousarray(del_extend, dtype=np.int32).reshape(-1)
        if do.size != Lp or de.size != Lp:
            raise ValueError("del_open and del_extend must hold Lp = %d entries" % Lp)
        rows = [np.ascontiguousarray(r, dtype=np.uint8).reshape(-1) for r in seqs]
        n = len(rows)
        offs = np.zeros(n + 1, dtype=np.int64)
        if n:
            offs[1:] = np.cumsum([r.size for r in rows])
        blob = np.concatenate(rows) if n and offs[-1] else np.zeros(1, dtype=np.uint8)
        score = np.zeros(n, dtype=np.int32)
        res = np.full((n, Lp), -1, dtype=np.int32) if traceback else None
        check(self._l.dca_profile_align(self._h, _ptr(m), int(Lp), int(A), _ptr(do), _ptr(de), int(ins_open), int(ins_extend), int(mode),
                                        _ptr(blob), _ptr(offs), n, _ptr(score), None if res is None else _ptr(res)))
        return score, res

    def msa(self):
        """The context's alignment as set_msa received it -> uint8[N, L]"""
        X = np.zeros((self.N, self.L), dtype=np.uint8)
        check(self._l.dca_get_msa(self._h, _ptr(X)))
        return X

    def profile_align_last_scratch(self):
        b = C.c_ulonglong(0)
        check(self._l.dca_profile_align_last_scratch(self._h, C.byref(b)))
        return int(b.value)

    def sw_scores(self, ref, seqs, sub, gap_open, gap_extend):
        """sw_scores on the device (dca_sw_scores_device): the same integers"""
        return _sw_scores_call(lambda *a: self._l.dca_sw_scores_device(self._h, *a), ref, seqs, sub, gap_open, gap_extend)

    # ---- three-site connected correlations (three_site.hip): integer counts, quantised alignment weights (include/dca_hip.h)
    def three_site_values(self, elements, Q=None):
        """elements: int32[T, 6] rows (i, j, k, a, b, c) in the context's column order; Q: uint8[nq, L] or None (the alignment
        under its weights) -> (uint64[T] counts, int denominator, float64[T] f3, float64[T] c3)"""
        el = np.ascontiguousarray(elements, dtype=np.int32).reshape(-1, 6)      # the library checks the rows
        q_ = None if Q is None else np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, self.L)
        T = el.shape[0]
        count, denom = np.zeros(T, dtype=np.uint64), C.c_uint64(0)
        f3, c3 = np.zeros(T, dtype=np.float64), np.zeros(T, dtype=np.float64)
        check(self._l.dca_three_site_values(self._h, None if q_ is None else _ptr(q_), 0 if q_ is None else int(q_.shape[0]),
                                            _ptr(el) if T else None, int(T), _ptr(count) if T else None, C.byref(denom),
                                            _ptr(f3) if T else None, _ptr(c3) if T else None))
        return count, int(denom.value), f3, c3

    def three_site_scan(self, K, Q=None, skip_state=-1):
        """The K elements of largest |c_ijk(a, b, c)| of the alignment (Q None) or of the set Q, |c| descending, ties by ascending
        (i, j, k, a, b, c) -> (int32[found, 6], float64[found] c3, float64[found] f3)"""
        q_ = None if Q is None else np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, self.L)
        K = int(K)
        el = np.zeros((max(K, 1), 6), dtype=np.int32)
        c3, f3 = np.zeros(max(K, 1), dtype=np.float64), np.zeros(max(K, 1), dtype=np.float64)
        found = C.c_int(0)
        check(self._l.dca_three_site_scan(self._h, None if q_ is None else _ptr(q_), 0 if q_ is None else int(q_.shape[0]), K,
                                          int(skip_state), _ptr(el), _ptr(c3), _ptr(f3), C.byref(found)))
        n = found.value
        return el[:n].copy(), c3[:n].copy(), f3[:n].copy()

    # ---- principal components of the reweighted alignment (pca.hip): model-free, nothing of the context changes
    def pca_fit(self, k, tol=1e-10, max_iterations=1000, seed=0):
        """dca_pca_fit -> dict: eigenvalues float64[k], components float64[k, L, q] (the context's column order), offsets float64[k],
        residuals float64[k], total_variance, iterations, converged (bool).  A fit out of iterations returns converged False."""
        k = int(k)
        lam, off, res = np.zeros(max(k, 1)), np.zeros(max(k, 1)), np.zeros(max(k, 1))
        comp = np.zeros((max(k, 1), self.L, self.q), dtype=np.float64)
        total, it, conv = C.c_double(0), C.c_int(0), C.c_int(0)
        check(self._l.dca_pca_fit(self._h, k, float(tol), int(max_iterations), int(seed), _ptr(lam), _ptr(comp), _ptr(off), _ptr(res),
                                  C.byref(total), C.byref(it), C.byref(conv)))
        return {"eigenvalues": lam, "components": comp, "offsets": off, "residuals": res, "total_variance": total.value,
                "iterations": it.value, "converged": bool(conv.value)}

    def pca_project(self, components, offsets, Q=None):
        """dca_pca_project: components float64[k, L, q], offsets float64[k]; Q uint8[n, L] or None (the alignment) -> float64[n, k]"""
        off = np.ascontiguousarray(offsets, dtype=np.float64).reshape(-1)
        k = int(off.size)
        comp = np.ascontiguousarray(components, dtype=np.float64)
        if comp.size != k * self.L * self.q:
            raise ValueError("components must hold k x L x q = %d x %d x %d values, not %d" % (k, self.L, self.q, comp.size))
        q_ = None if Q is None else np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, self.L)
        n = self.N if q_ is None else int(q_.shape[0])
        out = np.zeros((n, max(k, 1)), dtype=np.float64)
        check(self._l.dca_pca_project(self._h, None if q_ is None else _ptr(q_), 0 if q_ is None else n, k,
                                      _ptr(comp) if k else None, _ptr(off) if k else None, _ptr(out) if n else None))
        return out[:, :k]

    # ---- log Z by annealed importance sampling (ais.hip) -> (float64[n] log weights, log Z0, uint8[n, L] final chains or None)
    def _ais(self, fn, chains, temperatures, sweeps_per_temperature, seed, first_chain, betas, base_fields, return_chains):
        n = int(chains)
        b = ais_schedule(temperatures, betas)
        h0 = ais_base_fields(base_fields, self.L, self.q)
        args = AisArgs(n, int(temperatures), None if b is None else b.ctypes.data, int(sweeps_per_temperature), int(seed),
                       int(first_chain), None if h0 is None else h0.ctypes.data)
        logw = np.zeros(max(n, 0), dtype=np.float64)
        lz0 = C.c_double(0)
        out = np.zeros((max(n, 0), self.L), dtype=np.uint8) if return_chains else None
        check(fn(self._h, C.byref(args), _ptr(logw) if logw.size else None, C.byref(lz0), None if out is None else _ptr(out)))
        return logw, lz0.value, out

    def plm_ais(self, chains, temperatures, sweeps_per_temperature=1, seed=0, first_chain=0, betas=None, base_fields=None,
                return_chains=False):
        return self._ais(self._l.dca_plm_ais, chains, temperatures, sweeps_per_temperature, seed, first_chain, betas, base_fields,
                         return_chains)

    def mf_ais(self, chains, temperatures, sweeps_per_temperature=1, seed=0, first_chain=0, betas=None, base_fields=None,
               return_chains=False):
        return self._ais(self._l.dca_mf_ais, chains, temperatures, sweeps_per_temperature, seed, first_chain, betas, base_fields,
                         return_chains)

    def mf_di_scores(self, apc=False):
        out = np.zeros(self.L * (self.L - 1) // 2, dtype=np.float64)
        check(self._l.dca_mf_di_scores(self._h, int(bool(apc)), _ptr(out)))
        return out

    def mf_single_site_freqs(self):
        out = np.zeros((self.L, self.q), dtype=np.float64)
        check(self._l.dca_mf_single_site_freqs(self._h, _ptr(out)))
        return out

    def mf_pair_site_freqs(self):
        qm = self.q - 1
        out = np.zeros((self.L * (self.L - 1) // 2, qm, qm), dtype=np.float64)
        check(self._l.dca_mf_pair_site_freqs(self._h, _ptr(out)))
        return out

    def mf_corr_mat(self, pseudocount, want=True):
        n = self.L * (self.q - 1)
        out = np.zeros((n, n), dtype=np.float64) if want else None
        check(self._l.dca_mf_corr_mat(self._h, float(pseudocount), _ptr(out) if want else None))
        return out

    def mf_couplings(self, want=True):
        n = self.L * (self.q - 1)
        out = np.zeros((n, n), dtype=np.float64) if want else None
        check(self._l.dca_mf_couplings(self._h, _ptr(out) if want else None))
        return out

    def mf_scores(self, apc=True):
        out = np.zeros(self.L * (self.L - 1) // 2, dtype=np.float64)
        check(self._l.dca_mf_scores(self._h, int(bool(apc)), _ptr(out)))
        return out

    def mf_run(self, pseudocount, apc=True, want_couplings=False):
        n = self.L * (self.q - 1)
        scores = np.zeros(self.L * (self.L - 1) // 2, dtype=np.float64)
        J = np.zeros((n, n), dtype=np.float64) if want_couplings else None
        check(self._l.dca_mf_run(self._h, float(pseudocount), int(bool(apc)), _ptr(scores),
                                 _ptr(J) if want_couplings else None))
        return (scores, J) if want_couplings else scores

    def mf_corr_from_freqs(self, reg_fi, reg_fij, L, q):
        reg_fi = np.ascontiguousarray(reg_fi, dtype=np.float64)
        reg_fij = np.ascontiguousarray(reg_fij, dtype=np.float64)
        n = L * (q - 1)
        out = np.zeros((n, n), dtype=np.float64)
        check(self._l.dca_mf_corr_from_freqs(self._h, _ptr(reg_fi), _ptr(reg_fij), int(L), int(q), _ptr(out)))
        return out

    # ---- Hopfield-Potts model (hopfield.hip): afterwards the mf_* entries serve its couplings
    def mf_hopfield_fit(self, pseudocount, num_patterns=None, num_attractive=None, num_repulsive=None, tol=1e-10, max_iterations=1000,
                        seed=0):
        """dca_mf_hopfield_fit -> dict: eigenvalues, gains, residuals float64[p], signs int32[p], patterns float64[p, L, q - 1] (the
        attractive ones first, descending eigenvalue, then the repulsive ones, ascending), num_attractive, num_repulsive,
        iterations (attractive, repulsive), converged (bool, bool)."""
        explicit = num_patterns is None
        a, r = int(num_attractive or 0), int(num_repulsive or 0)
        cap = max(a + r if explicit else int(num_patterns), 1)
        args = HopfieldArgs(HOPFIELD_EXPLICIT if explicit else HOPFIELD_LIKELIHOOD, 0 if explicit else int(num_patterns), a, r,
                            int(max_iterations), float(tol), int(seed))
        lam, gain, res = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        sign = np.zeros(cap, dtype=np.int32)
        xi = np.zeros((cap, self.L, self.q - 1), dtype=np.float64)
        info = HopfieldInfo()
        check(self._l.dca_mf_hopfield_fit(self._h, float(pseudocount), C.byref(args), _ptr(lam), _ptr(gain), _ptr(sign), _ptr(xi),
                                          _ptr(res), C.byref(info)))
        p = info.num_attractive + info.num_repulsive
        return {"eigenvalues": lam[:p], "gains": gain[:p], "signs": sign[:p], "patterns": xi[:p], "residuals": res[:p],
                "num_attractive": int(info.num_attractive), "num_repulsive": int(info.num_repulsive),
                "iterations": (int(info.iterations[0]), int(info.iterations[1])),
                "converged": (bool(info.converged[0]), bool(info.converged[1]))}

    def mf_model_kind(self):
        kind = C.c_int(0)
        check(self._l.dca_mf_model_kind(self._h, C.byref(kind)))
        return kind.value

    def mf_hopfield_couplings(self):
        n = self.L * (self.q - 1)
        out = np.zeros((n, n), dtype=np.float64)
        check(self._l.dca_mf_hopfield_couplings(self._h, _ptr(out)))
        return out

    def hopfield_project(self, patterns, Q=None):
        """dca_hopfield_project: patterns float64[p, L, q - 1]; Q uint8[n, L] or None (the alignment) -> float64[n, p]"""
        xi = np.ascontiguousarray(patterns, dtype=np.float64)
        per = self.L * (self.q - 1)
        if xi.size == 0 or xi.size % per:
            raise ValueError("patterns must hold p x L x (q - 1) = p x %d x %d values, not %d" % (self.L, self.q - 1, xi.size))
        p = xi.size // per
        q_ = None if Q is None else np.ascontiguousarray(Q, dtype=np.uint8).reshape(-1, self.L)
        n = self.N if q_ is None else int(q_.shape[0])
        out = np.zeros((n, p), dtype=np.float64)
        check(self._l.dca_hopfield_project(self._h, None if q_ is None else _ptr(q_), 0 if q_ is None else n, p, _ptr(xi),
                                           _ptr(out) if n else None))
        return out

    def dense_apply(self, A, V, n=None):
        """dca_dense_apply: A float64[n, ld] (ld >= n), V float64[n, b] -> A[:, :n] V through the operator kernel of the fit"""
        A = np.ascontiguousarray(A, dtype=np.float64)
        V = np.ascontiguousarray(V, dtype=np.float64)
        n = A.shape[0] if n is None else int(n)
        out = np.zeros((n, V.shape[1]), dtype=np.float64)
        check(self._l.dca_dense_apply(self._h, _ptr(A), n, A.shape[1], _ptr(V), V.shape[1], _ptr(out)))
        return out

    def spd_inverse(self, A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        out = np.zeros_like(A)
        check(self._l.dca_spd_inverse(self._h, _ptr(A), A.shape[0], _ptr(out)))
        return out

    # ---- timing
    def set_profiling(self, on=True):
        check(self._l.dca_set_profiling(self._h, int(bool(on))))

    def set_profiling_only(self, stage):
        """Clock ONE stage only (None: profiling off): two event records per launch of it instead of two per stage."""
        check(self._l.dca_set_profiling_only(self._h, stage.encode() if stage else None))

    def reset_kernel_times(self):
        check(self._l.dca_reset_kernel_times(self._h))

    def kernel_time(self, tag):
        ms, n = C.c_double(0), C.c_int(0)
        check(self._l.dca_get_kernel_time(self._h, tag.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


DCA_ALIGN_LOCAL, DCA_ALIGN_GLOCAL = 0, 1


def sw_scores(ref, seqs, sub, gap_open, gap_extend):
    """Best local alignment score of `ref` against every string of `seqs` (host code in libdca_hip.so)."""
    return _sw_scores_call(lib().dca_sw_scores, ref, seqs, sub, gap_open, gap_extend)


def _sw_scores_call(entry, ref, seqs, sub, gap_open, gap_extend):
    enc = [s.encode("ascii") for s in seqs]
    offs = np.zeros(len(enc) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(e) for e in enc])
    blob = b"".join(enc)
    sub = np.ascontiguousarray(sub, dtype=np.int32)
    out = np.zeros(len(enc), dtype=np.int32)
    r = ref.encode("ascii")
    check(entry(r, len(r), blob, _ptr(offs), len(enc), _ptr(sub), int(gap_open), int(gap_extend), _ptr(out)))
    return out


def sw_align(a, b, sub, gap_open, gap_extend):
    """One optimal local alignment -> (aligned_a, aligned_b, score, start_a, start_b)."""
    L = lib()
    ea, eb = a.encode("ascii"), b.encode("ascii")
    sub = np.ascontiguousarray(sub, dtype=np.int32)
    cap = len(ea) + len(eb) + 1
    ba, bb = C.create_string_buffer(cap), C.create_string_buffer(cap)
    score, sa, sb, n = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(L.dca_sw_align(ea, len(ea), eb, len(eb), _ptr(sub), int(gap_open), int(gap_extend), C.byref(score), C.byref(sa),
                         C.byref(sb), ba, bb, C.byref(n)))
    return ba.value.decode("ascii"), bb.value.decode("ascii"), score.value, sa.value, sb.value

"""ctypes binding of lib/pygmm.so (the C ABI in include/pygmm_hip.h).

Every pointer-returning function gets an explicit ``restype`` (the reference's wrapper does
not -- src/gmm/python/pygmm.py:30-31 -- and truncates handles to 32 bits on 64-bit Pythons).
There is no CPU fallback: if the library is missing, or no GPU is visible when a compute call
is made, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SR_PYGMM_LIB points at another build of the same library (A/B timing of kernel variants)
# (SR_PYGMM_ALLOW_MISSING: comma-separated calls such a build may lack, e.g. the parent commit's; any other missing call fails the load)
LIB_PATH = os.environ.get("SR_PYGMM_LIB") or os.path.join(_HERE, "lib", "pygmm.so")

LEGACY_SYMBOLS = ["new_gmm", "load", "dump", "train_model", "train_model_from_ubm", "score_all",
                  "score_batch", "score_instance", "get_dim", "get_nr_mixtures"]
EXT_SYMBOLS = [
    "sr_last_error", "sr_gpu_runtime_lost", "sr_device_count", "sr_set_device", "sr_set_thread_device", "sr_get_device", "sr_device_synchronize",
    "sr_device_name", "sr_device_numa_node", "sr_bind_thread_near_device", "sr_multi_slot_numa_node", "sr_free_gmm", "sr_gmm_from_arrays", "sr_gmm_get_params", "sr_gmm_dumps",
    "sr_gmm_loads", "sr_score_frames_f32", "sr_score_models_f32", "sr_modelset_create", "sr_modelset_free",
    "sr_modelset_size", "sr_modelset_info", "sr_modelset_dim", "sr_batch_from_pcm", "sr_batch_from_pcm_f32",
    "sr_batch_from_features", "sr_batch_update_pcm", "sr_batch_reset_pcm", "sr_batch_reset_features", "sr_batch_free", "sr_batch_num_utterances", "sr_batch_num_rows",
    "sr_batch_dim", "sr_batch_offsets", "sr_batch_download", "sr_score_batch_set",
    "sr_mfcc_create", "sr_mfcc_set_lpc", "sr_mfcc_free", "sr_mfcc_frame_len", "sr_mfcc_frame_shift",
    "sr_mfcc_num_frames", "sr_mfcc_tables", "sr_mfcc_plan", "sr_mfcc_extract_batch", "sr_predict_pcm_batch",
    "sr_train_f32", "sr_profile_enable", "sr_profile_reset", "sr_profile_get", "sr_set_option",
    "sr_last_score_kernel", "sr_last_em_stats_engine", "sr_ltsd_num_windows", "sr_ltsd_noise_spectrum", "sr_ltsd_compute", "sr_stream_create", "sr_stream_submit", "sr_stream_collect", "sr_stream_free",
    "sr_multi_create", "sr_multi_free", "sr_multi_slots", "sr_multi_slot_device", "sr_multi_predict_pcm",
    "sr_hbm_copy_gbps", "sr_reference_rand_sample", "sr_flush_stats", "sr_host_register", "sr_host_unregister",
    "sr_mfma_peak_probe", "sr_mfma_streamed_probe", "sr_kmeans_fast_stats",
    "sr_fullgmm_create", "sr_fullgmm_fit", "sr_fullgmm_info", "sr_fullgmm_get", "sr_fullgmm_free", "sr_fullset_create",
    "sr_fullset_score_batch", "sr_fullset_free", "sr_fullset_predict_pcm_batch", "sr_stream_create_full", "sr_multi_create_full",
    "sr_stream_create_vad", "sr_stream_collect_vad",
    "sr_fullgmm_fit_batch", "sr_fullgmm_fit_batch_error", "sr_full_fit_batch_stats", "sr_full_fit_batch_bytes",
    "sr_full_fit_plan",
    "sr_open_set_decide", "sr_score_batch_set_open", "sr_predict_pcm_batch_open", "sr_stream_set_open", "sr_stream_collect_open",
    "sr_multi_predict_pcm_open",
    "sr_batch_download_pcm16", "sr_silence_remove_batch", "sr_silence_plan",
    "sr_score_batch_set_topc", "sr_predict_pcm_batch_topc", "sr_topc_plan",
    "sr_bw_stats_batch", "sr_bw_plan",
    "sr_jfa_open", "sr_jfa_factors", "sr_jfa_update", "sr_jfa_train", "sr_jfa_close", "sr_jfa_plan",
    "sr_jfa_score_integrated", "sr_jfa_score_linear", "sr_jfa_score_plan",
    "sr_bw_stats_resident", "sr_stats_from_host", "sr_stats_info", "sr_stats_get", "sr_stats_take", "sr_stats_close",
    "sr_jfa_open_centred", "sr_jfa_statistics", "sr_jfa_centre_plan", "sr_jfa_zd", "sr_jfa_score_integrated_stats", "sr_jfa_score_linear_stats",
    "sr_multi_slot_pieces", "sr_multi_plan",
    "sr_map_fit_batch", "sr_map_fit_batch_error", "sr_map_fit_batch_stats", "sr_map_fit_batch_bytes", "sr_map_fit_plan",
    "sr_score_norm", "sr_score_norm_select", "sr_score_norm_plan",
    "sr_backend_fit", "sr_backend_apply", "sr_cosine_score", "sr_plda_train", "sr_plda_score", "sr_plda_plan",
    "sr_sym_eig", "sr_gen_eig", "sr_lda_fit", "sr_backend_project", "sr_plda_score_diag", "sr_eig_plan",
    "sr_calib_train", "sr_calib_eval", "sr_calib_apply", "sr_calib_counts", "sr_calib_plan",
    "sr_feature_norm_batch", "sr_feature_norm_plan", "sr_norm_quantile",
    "sr_timeline_windows", "sr_timeline_plan", "sr_timeline_decide", "sr_timeline_batch", "sr_fullset_timeline_batch", "sr_timeline_pcm_batch",
    "sr_diar_segments", "sr_diar_plan", "sr_diar_stats_batch", "sr_diar_bic_matrix", "sr_diar_cluster_batch", "sr_diar_cluster_pcm_batch",
    "sr_ahc_matrix", "sr_diar_cut",
    "sr_xvector_create", "sr_xvector_free", "sr_xvector_info", "sr_xvector_plan", "sr_xvector_extract_batch", "sr_xvector_extract",
]

SR_CLAMP_COMPAT = 1
SR_SCORE_PRECISE = 0x200
SR_STREAM_GRAPH = 0x100
T_SCORE, T_MFCC, T_CMVN, T_FINALIZE, T_ESTEP, T_SCORE_REF = 0, 1, 2, 3, 4, 5
T_TOPC_SELECT, T_TOPC_ROUTE, T_TOPC_EVAL, T_TOPC_COMBINE = 6, 7, 8, 9      # the four stages of sr_score_batch_set_topc
T_BW_LSE, T_BW_STATS, T_BW_REDUCE = 10, 11, 12                             # the three passes of sr_bw_stats_batch
T_JFA_GRAM, T_JFA_GEMM_L, T_JFA_GEMM_B, T_JFA_GEMM_A, T_JFA_GEMM_C, T_JFA_FACTOR, T_JFA_UPDATE = 13, 14, 15, 16, 17, 18, 19      # sr_jfa_*'s stages


class Parameter(C.Structure):
    """struct Parameter, src/gmm/src/pygmm.hh:12-26 (== GMMParameter, pygmm.py:18-27)."""
    _fields_ = [("nr_instance", C.c_int), ("nr_dim", C.c_int), ("nr_mixture", C.c_int),
                ("min_covar", C.c_double), ("threshold", C.c_double), ("nr_iteration", C.c_int),
                ("init_with_kmeans", C.c_int), ("concurrency", C.c_int), ("verbosity", C.c_int)]


class FullFitParams(C.Structure):
    """struct SRFullFitParams (include/pygmm_hip.h)."""
    _fields_ = [("tol", C.c_double), ("reg_covar", C.c_double), ("max_iter", C.c_int), ("init_given", C.c_int),
                ("seed", C.c_longlong)]


class FullFitStats(C.Structure):
    """struct SRFullFitStats (include/pygmm_hip.h)."""
    _fields_ = [("n_iter", C.c_int), ("converged", C.c_int), ("lower_bound", C.c_double)]


class SRError(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and prototype the shared library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SRError("%s is missing: build it with `python -c 'import __graft_entry__ as g; "
                      "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    dpp = C.POINTER(C.POINTER(C.c_double))
    sig = {
        # legacy (pygmm.hh:28-41)
        "new_gmm": (vp, [i32, i32]),
        "load": (vp, [C.c_char_p]),
        "dump": (None, [vp, C.c_char_p]),
        "train_model": (None, [vp, dpp, C.POINTER(Parameter)]),
        "train_model_from_ubm": (None, [vp, vp, dpp, C.POINTER(Parameter)]),
        "score_all": (dbl, [vp, dpp, i32, i32, i32]),
        "score_batch": (None, [vp, dpp, dp, i32, i32, i32]),
        "score_instance": (dbl, [vp, dp, i32]),
        "get_dim": (i32, [vp]),
        "get_nr_mixtures": (i32, [vp]),
        # extensions
        "sr_last_error": (C.c_char_p, []),
        "sr_gpu_runtime_lost": (i32, []),
        "sr_device_count": (i32, []),
        "sr_set_device": (i32, [i32]),
        "sr_set_thread_device": (i32, [i32]),
        "sr_get_device": (i32, []),
        "sr_device_synchronize": (i32, []),
        "sr_device_name": (i32, [C.c_char_p, i32]),
        "sr_device_numa_node": (i32, [i32]),
        "sr_bind_thread_near_device": (i32, [i32]),
        "sr_multi_slot_numa_node": (i32, [vp, i32]),
        "sr_free_gmm": (None, [vp]),
        "sr_gmm_from_arrays": (vp, [i32, i32, dp, dp, dp]),
        "sr_gmm_get_params": (i32, [vp, dp, dp, dp]),
        "sr_gmm_dumps": (i32, [vp, C.c_char_p, C.c_long, C.POINTER(C.c_long)]),
        "sr_gmm_loads": (vp, [C.c_char_p]),
        "sr_score_frames_f32": (i32, [vp, fp, C.c_long, i32, fp, dp, i32]),
        "sr_score_models_f32": (i32, [C.POINTER(vp), i32, fp, C.c_long, i32, dp, i32]),
        "sr_modelset_create": (vp, [C.POINTER(vp), i32]),
        "sr_modelset_free": (None, [vp]),
        "sr_modelset_size": (i32, [vp]),
        "sr_modelset_info": (i32, [vp, dp]),
        "sr_modelset_dim": (i32, [vp]),
        "sr_batch_from_pcm": (vp, [C.POINTER(C.c_int16), C.POINTER(i64), i32]),
        "sr_batch_from_pcm_f32": (vp, [fp, C.POINTER(i64), i32]),
        "sr_batch_from_features": (vp, [fp, i64, i32, C.POINTER(i64), i32]),
        "sr_batch_update_pcm": (i32, [vp, C.POINTER(C.c_int16), i64]),
        "sr_batch_reset_pcm": (i32, [vp, C.POINTER(C.c_int16), C.POINTER(i64), i32]),
        "sr_batch_reset_features": (i32, [vp, fp, i64, i32, C.POINTER(i64), i32]),
        "sr_batch_free": (None, [vp]),
        "sr_batch_num_utterances": (i32, [vp]),
        "sr_batch_num_rows": (i64, [vp]),
        "sr_batch_dim": (i32, [vp]),
        "sr_batch_offsets": (i32, [vp, C.POINTER(i64)]),
        "sr_batch_download": (i32, [vp, fp]),
        "sr_batch_download_pcm16": (i32, [vp, C.POINTER(C.c_int16)]),
        "sr_silence_remove_batch": (vp, [vp, dbl, dbl, dbl, dbl, C.POINTER(i64)]),
        "sr_silence_plan": (i32, [dbl, dbl, dbl, i64, C.POINTER(C.c_int32), i32]),
        "sr_score_batch_set": (i32, [vp, vp, dp, C.POINTER(i32), fp, i32]),
        "sr_mfcc_create": (vp, [dbl, dbl, dbl, i32, i32, i32, dbl]),
        "sr_mfcc_set_lpc": (i32, [vp, i32]),
        "sr_mfcc_free": (None, [vp]),
        "sr_mfcc_frame_len": (i32, [vp]),
        "sr_mfcc_frame_shift": (i32, [vp]),
        "sr_mfcc_num_frames": (i64, [vp, i64]),
        "sr_mfcc_tables": (i32, [vp, dp, dp, dp]),
        "sr_mfcc_plan": (i32, [vp, i32, i32, i32, i64, i32, C.POINTER(C.c_int32), i32]),
        "sr_mfcc_extract_batch": (vp, [vp, vp, i32, i32]),
        "sr_predict_pcm_batch": (i32, [vp, vp, vp, i32, dp, C.POINTER(i32), i32]),
        "sr_train_f32": (i32, [vp, vp, fp, C.c_long, i32, C.POINTER(Parameter), C.c_long]),
        "sr_profile_enable": (i32, [i32]),
        "sr_profile_reset": (i32, []),
        "sr_profile_get": (i32, [i32, dp, C.POINTER(C.c_long)]),
        "sr_set_option": (i32, [C.c_char_p, C.c_long]),
        "sr_last_score_kernel": (C.c_char_p, []),
        "sr_last_em_stats_engine": (C.c_int, []),
        "sr_flush_stats": (None, [C.POINTER(C.c_long)] * 3),
        "sr_mfma_peak_probe": (i32, [C.c_double, dp, dp]),
        "sr_mfma_streamed_probe": (i32, [C.c_double, dp, dp]),
        "sr_kmeans_fast_stats": (None, [C.POINTER(C.c_long)] * 2),
        "sr_host_register": (i32, [vp, C.c_size_t]),
        "sr_host_unregister": (i32, [vp]),
        "sr_reference_rand_sample": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
        "sr_ltsd_num_windows": (i64, [i64, i32]),
        "sr_ltsd_noise_spectrum": (i32, [vp, i32, fp]),
        "sr_ltsd_compute": (i32, [vp, i32, i32, fp, fp, C.POINTER(i64)]),
        "sr_stream_create": (vp, [vp, vp, i32, i64, i32, i32]),
        "sr_stream_submit": (i32, [vp, C.POINTER(C.c_int16)]),
        "sr_stream_collect": (i32, [vp, dp, C.POINTER(i32), dp]),
        "sr_stream_free": (None, [vp]),
        "sr_multi_create": (vp, [C.POINTER(vp), i32, dbl, dbl, dbl, i32, i32, i32, dbl, i32]),
        "sr_multi_free": (None, [vp]),
        "sr_multi_slots": (i32, [vp]),
        "sr_multi_slot_device": (i32, [vp, i32]),
        "sr_multi_predict_pcm": (i32, [vp, C.POINTER(C.c_int16), C.POINTER(i64), i32, i32, dp, C.POINTER(i32), dp, i32]),
        "sr_hbm_copy_gbps": (i32, [C.c_size_t, i32, dp]),
        "sr_fullgmm_create": (vp, [i32, i32, dp, dp, dp]),
        "sr_fullgmm_fit": (i32, [vp, dp, i64, i32, C.POINTER(FullFitParams), C.POINTER(FullFitStats)]),
        "sr_fullgmm_fit_batch": (i32, [C.POINTER(vp), i32, dp, C.POINTER(i64), i32, C.POINTER(FullFitParams), C.POINTER(FullFitStats),
                                       C.POINTER(i32)]),
        "sr_fullgmm_fit_batch_error": (C.c_char_p, [i32]),
        "sr_full_fit_batch_stats": (None, [C.POINTER(C.c_long)] * 3),
        "sr_full_fit_batch_bytes": (C.c_long, []),
        "sr_full_fit_plan": (i32, [i32, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), i32, i64, C.POINTER(i64), C.POINTER(i64), i64,
                                   C.POINTER(i64), i32]),
        "sr_fullgmm_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "sr_fullgmm_get": (i32, [vp, dp, dp, dp, dp]),
        "sr_fullgmm_free": (None, [vp]),
        "sr_fullset_create": (vp, [C.POINTER(vp), i32]),
        "sr_fullset_score_batch": (i32, [vp, vp, dp, C.POINTER(i32), fp]),
        "sr_fullset_free": (None, [vp]),
        "sr_fullset_predict_pcm_batch": (i32, [vp, vp, vp, i32, dp, C.POINTER(i32)]),
        "sr_stream_create_full": (vp, [vp, vp, i32, i64, i32, i32]),
        "sr_multi_create_full": (vp, [C.POINTER(vp), i32, dbl, dbl, dbl, i32, i32, i32, dbl, i32, i32]),
        "sr_stream_create_vad": (vp, [vp, vp, vp, i32, i64, i32, i32, i32, i32, fp, dbl, dbl]),
        "sr_stream_collect_vad": (i32, [vp, dp, C.POINTER(i32), C.POINTER(i32), dp]),
        "sr_open_set_decide": (i32, [dp, i32, i32, i32, C.POINTER(i64), dbl, C.POINTER(i32), dp]),
        "sr_score_batch_set_open": (i32, [vp, vp, i32, dbl, dp, C.POINTER(i32), dp, i32]),
        "sr_predict_pcm_batch_open": (i32, [vp, vp, vp, i32, i32, dbl, dp, C.POINTER(i32), dp, i32]),
        "sr_stream_set_open": (i32, [vp, i32, dbl]),
        "sr_stream_collect_open": (i32, [vp, dp, C.POINTER(i32), dp, C.POINTER(i32), dp]),
        "sr_multi_predict_pcm_open": (i32, [vp, C.POINTER(C.c_int16), C.POINTER(i64), i32, i32, i32, dbl, dp, C.POINTER(i32), dp, dp,
                                            i32]),
        "sr_score_batch_set_topc": (i32, [vp, vp, i32, i32, dp, C.POINTER(i32), C.POINTER(i32), fp, i32]),
        "sr_predict_pcm_batch_topc": (i32, [vp, vp, vp, i32, i32, i32, dp, C.POINTER(i32), i32]),
        "sr_topc_plan": (i32, [i32, i32, i32, i32, i64, i64, i32, C.POINTER(C.c_int32), i32]),
        "sr_bw_stats_batch": (i32, [vp, i32, vp, dp, dp, dp, C.POINTER(i64)]),
        "sr_bw_plan": (i32, [i32, i32, i32, i32, i32, i32, C.POINTER(i64), i64, i64, i64, i32, C.POINTER(i64), i64, C.POINTER(i64), i32]),
        "sr_jfa_open": (vp, [i64, i32, i32, dp, dp, dp]),
        "sr_jfa_factors": (i32, [vp, dp, i32, dp, dp, dp, C.POINTER(i64)]),
        "sr_jfa_update": (i32, [i32, i32, i32, dp, dp, dp, C.POINTER(i64)]),
        "sr_jfa_train": (i32, [vp, dp, i32, i32, dp, C.POINTER(i64)]),
        "sr_jfa_close": (None, [vp]),
        "sr_jfa_plan": (i32, [i64, i32, i32, i32, i64, i32, i32, C.POINTER(i64), i32]),
        "sr_jfa_score_integrated": (i32, [i64, i64, i32, i32, i32, i32, dp, dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_uint8), i64, i64, dp,
                                          C.POINTER(i64), C.POINTER(i64)]),
        "sr_jfa_score_linear": (i32, [i64, i64, i32, i32, i32, i32, dp, dp, dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_uint8), i64, i64, dp,
                                      C.POINTER(i64)]),
        "sr_jfa_score_plan": (i32, [i64, i64, i32, i32, i32, i32, i32, i64, i32, i32, C.POINTER(i64), i32]),
        "sr_bw_stats_resident": (vp, [vp, i32, vp, dp, C.POINTER(i64)]),
        "sr_stats_from_host": (vp, [i64, i32, i32, dp, dp]),
        "sr_stats_info": (i32, [vp, C.POINTER(i64), i32]),
        "sr_stats_get": (i32, [vp, dp, dp]),
        "sr_stats_take": (vp, [vp, C.POINTER(i64), i64]),
        "sr_stats_close": (None, [vp]),
        "sr_jfa_open_centred": (vp, [vp, dp, dp, i32, C.POINTER(i64), i64, dp, dp, dp, i32, dp, dp, i32, dp]),
        "sr_jfa_statistics": (i32, [vp, dp, dp]),
        "sr_jfa_centre_plan": (i32, [i64, i64, i32, i32, i32, i32, i32, i64, C.POINTER(i64), i32]),
        "sr_jfa_zd": (i32, [vp, dp, i32, dp, dp, dp]),
        "sr_jfa_score_integrated_stats": (i32, [vp, i64, i32, i32, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_uint8), i64, i64, dp,
                                                C.POINTER(i64), C.POINTER(i64)]),
        "sr_jfa_score_linear_stats": (i32, [vp, i64, i32, i32, dp, dp, dp, dp, dp, dp, dp, dp, C.POINTER(C.c_uint8), i64, i64, dp, C.POINTER(i64)]),
        "sr_multi_slot_pieces": (i32, [vp, i32]),
        "sr_multi_plan": (i32, [C.POINTER(i64), i32, C.POINTER(i32), i32, i32, C.POINTER(i32)] + [C.POINTER(i32)] * 4),
        "sr_map_fit_batch": (i32, [C.POINTER(vp), i32, vp, fp, C.POINTER(i64), i32, C.POINTER(Parameter), C.c_long, C.POINTER(i32),
                                   C.POINTER(i32)]),
        "sr_map_fit_batch_error": (C.c_char_p, [i32]),
        "sr_map_fit_batch_stats": (None, [C.POINTER(C.c_long)] * 5),
        "sr_map_fit_batch_bytes": (C.c_long, []),
        "sr_map_fit_plan": (i32, [i32, i32, C.POINTER(i64), i32, C.POINTER(Parameter), i64, i32, C.POINTER(i64), C.POINTER(i64), i64,
                                  C.POINTER(i64), i64, C.POINTER(i64), i64, C.POINTER(i64), i32]),
        "sr_score_norm": (i32, [i32, i64, i64, i64, i64, i32, dp, dp, dp, dp, dp, C.POINTER(i64)]),
        "sr_score_norm_select": (i32, [i64, i64, i32, dp, C.POINTER(i64), dp, dp]),
        "sr_score_norm_plan": (i32, [i32, i64, i64, i64, i64, i32, i64, i32, C.POINTER(i64), i32]),
        "sr_calib_train": (i32, [i32, i64, dp, C.POINTER(C.c_int8), C.c_double, C.c_double, C.c_double, i32, dp, i32, dp, C.POINTER(i64)]),
        "sr_calib_eval": (i32, [i32, i64, dp, C.POINTER(C.c_int8), C.c_double, C.c_double, dp, dp, dp, dp, C.POINTER(i64)]),
        "sr_calib_apply": (i32, [i32, i64, dp, dp, dp]),
        "sr_calib_counts": (i32, [i64, dp, C.POINTER(C.c_int8), i32, dp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "sr_calib_plan": (i32, [i32, i64, i32, i32, i64, i32, C.POINTER(i64), i32]),
        "sr_backend_fit": (i32, [i32, i64, i32, dp, C.POINTER(i64), i64, dp, dp]),
        "sr_backend_apply": (i32, [i64, i32, dp, dp, dp, i32, dp, C.POINTER(i64)]),
        "sr_cosine_score": (i32, [i64, i64, i32, dp, dp, dp]),
        "sr_plda_train": (i32, [i64, i32, dp, C.POINTER(i64), i64, i32, i32, dp, dp, dp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "sr_plda_score": (i32, [i64, i64, i32, dp, dp, dp, dp, C.POINTER(i64), dp, dp, C.POINTER(i64)]),
        "sr_plda_plan": (i32, [i32, i32, i64, i64, i64, C.POINTER(i64), i64, i32, i32, C.POINTER(i64), i32, C.POINTER(i64), C.POINTER(i64)]),
        "sr_sym_eig": (i32, [i32, dp, dp, dp, C.POINTER(i32), C.POINTER(i32)]),
        "sr_gen_eig": (i32, [i32, dp, dp, dp, dp, C.POINTER(i32), C.POINTER(i32)]),
        "sr_lda_fit": (i32, [i64, i32, dp, C.POINTER(i64), i64, i32, dp, dp, dp]),
        "sr_backend_project": (i32, [i64, i32, i32, dp, dp, dp, i32, dp, C.POINTER(i64)]),
        "sr_plda_score_diag": (i32, [i64, i64, i32, dp, dp, dp, dp, C.POINTER(i64), dp, dp, C.POINTER(i64)]),
        "sr_eig_plan": (i32, [i32, i32, C.POINTER(i64), i32, C.POINTER(i32)]),
        "sr_feature_norm_batch": (vp, [vp, i32, i32, C.POINTER(i64), C.POINTER(C.c_int32)]),
        "sr_feature_norm_plan": (i32, [i32, i32, i32, i64, i32, C.POINTER(C.c_int32), i32]),
        "sr_norm_quantile": (dbl, [dbl]),
        "sr_timeline_windows": (i64, [i64, i64, i64]),
        "sr_timeline_plan": (i32, [i32, i32, i64, i32, i32, C.POINTER(C.c_int32), i32]),
        "sr_timeline_decide": (i32, [dp, C.POINTER(C.c_int32), C.POINTER(i64), i32, i32, i32, dbl, i32, dbl, i32, C.POINTER(i32), dp,
                                     C.POINTER(i64)]),
        "sr_timeline_batch": (i32, [vp, vp, i32, i32, i32, dbl, i32, dbl, i32, i32, C.POINTER(i64), C.POINTER(i32), dp, dp, C.POINTER(i64)]),
        "sr_fullset_timeline_batch": (i32, [vp, vp, i32, i32, dbl, i32, dbl, i32, C.POINTER(i64), C.POINTER(i32), dp, dp, C.POINTER(i64)]),
        "sr_timeline_pcm_batch": (i32, [vp, vp, vp, i32, i32, i32, i32, dbl, i32, dbl, i32, i32, C.POINTER(i64), C.POINTER(i32), dp, dp,
                                        C.POINTER(i64)]),
        "sr_diar_segments": (i64, [i64, i64]),
        "sr_diar_plan": (i32, [i32, i32, i32, C.POINTER(i64), i32, i64, C.POINTER(i64), i32, C.POINTER(C.c_int32), C.POINTER(i64)]),
        "sr_diar_stats_batch": (i32, [vp, i32, i64, C.POINTER(i64), dp]),
        "sr_diar_bic_matrix": (i32, [i32, i64, dp, dbl, dbl, dp, dp, C.POINTER(i64)]),
        "sr_diar_cluster_batch": (i32, [vp, i32, i32, i32, dbl, dbl, dbl, i32, i32, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), dp, C.POINTER(C.c_int32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]),
        "sr_diar_cluster_pcm_batch": (i32, [vp, vp, i32, i32, i32, i32, dbl, dbl, dbl, i32, i32, i64, C.POINTER(i64), C.POINTER(i64),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, C.POINTER(C.c_int32), C.POINTER(i64), C.POINTER(i64),
                                            C.POINTER(i64)]),
        "sr_ahc_matrix": (i32, [i64, dp, i32, dbl, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, C.POINTER(i64), C.POINTER(C.c_int32),
                                C.POINTER(i64)]),
        "sr_diar_cut": (i64, [i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp, i64, dbl, i32, i32, C.POINTER(C.c_int32), C.POINTER(i64)]),
        "sr_xvector_create": (vp, [i32, C.POINTER(C.c_int32), dp, C.POINTER(fp), C.POINTER(fp), C.POINTER(fp), C.POINTER(fp)]),
        "sr_xvector_free": (None, [vp]),
        "sr_xvector_info": (i32, [vp, C.POINTER(C.c_int32), i32]),
        "sr_xvector_plan": (i32, [i32, C.POINTER(C.c_int32), dp, C.POINTER(i64), i64, i32, i32, i64, C.POINTER(i64), i32, C.POINTER(C.c_int32),
                                  C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), i32, i64, C.POINTER(C.c_int32), i64]),
        "sr_xvector_extract_batch": (i32, [vp, vp, C.POINTER(C.c_int32), i64, i32, i32, fp, i64, dp]),
        "sr_xvector_extract": (i32, [vp, fp, i64, i32, C.POINTER(i64), i32, C.POINTER(C.c_int32), i64, i32, i32, fp, i64, dp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name, None)
        if fn is None:
            # another build loaded for an A/B run (SR_PYGMM_LIB) may predate a call: SR_PYGMM_ALLOW_MISSING names, comma-separated,
            # the calls the run does without (using one there raises AttributeError); any other missing call is a stale build
            if os.environ.get("SR_PYGMM_LIB") and name in os.environ.get("SR_PYGMM_ALLOW_MISSING", "").split(","):
                continue
            raise SRError("%s does not export %s: rebuild it (an older build loaded through SR_PYGMM_LIB on purpose: name the "
                          "calls it lacks in SR_PYGMM_ALLOW_MISSING)" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def gpu_runtime_lost() -> bool:
    """True in a process forked after its parent initialised the GPU runtime (include/pygmm_hip.h, "Processes"): the per-model
    entry points are served by a helper process there, the batched ones refuse."""
    return bool(lib().sr_gpu_runtime_lost())


def last_error() -> str:
    return lib().sr_last_error().decode("utf-8", "replace")


def check(status, what: str = "call"):
    """Raise on a negative status / NULL handle."""
    if status is None or (isinstance(status, int) and status < 0):
        raise SRError("%s failed: %s" % (what, last_error()))
    return status


# ---- small marshalling helpers ----

def f32_matrix(X) -> np.ndarray:
    a = np.ascontiguousarray(X, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("expected a 2-D [frames, dim] array, got shape %r" % (a.shape,))
    return a


def as_fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def as_dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def as_i64p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def as_i8p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int8))


def as_i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def set_device(device: int) -> None:
    check(lib().sr_set_device(int(device)), "sr_set_device")


def set_thread_device(device: int) -> None:
    """The calling host thread's current device (handles belong to the device they were created on)."""
    check(lib().sr_set_thread_device(int(device)), "sr_set_thread_device")


def hbm_copy_gbps(nbytes: int = 1 << 30, iters: int = 10) -> float:
    """Measured device-to-device copy rate (read + written bytes per second, GB/s)."""
    g = C.c_double(0)
    check(lib().sr_hbm_copy_gbps(int(nbytes), int(iters), C.byref(g)), "sr_hbm_copy_gbps")
    return g.value


def device_count() -> int:
    return int(lib().sr_device_count())


def bind_thread_near_device(device: int) -> int:
    """Pin the calling host thread to the cores of `device`'s NUMA node (sysfs); -> the node, -1 when left alone."""
    return int(lib().sr_bind_thread_near_device(int(device)))


def device_name() -> str:
    buf = C.create_string_buffer(256)
    check(lib().sr_device_name(buf, 256), "sr_device_name")
    return buf.value.decode()


def synchronize() -> None:
    check(lib().sr_device_synchronize(), "sr_device_synchronize")


def set_option(key: str, value: int) -> None:
    check(lib().sr_set_option(key.encode(), int(value)), "sr_set_option")


def host_register(a) -> None:
    """Page-lock a numpy array's memory so that the copy engines read it in place (sr_multi_predict_pcm)."""
    check(lib().sr_host_register(C.c_void_p(a.ctypes.data), a.nbytes), "sr_host_register")


def host_unregister(a) -> None:
    check(lib().sr_host_unregister(C.c_void_p(a.ctypes.data)), "sr_host_unregister")


def flush_stats():
    """(resolve calls, (tile, model) pairs noted, frames re-evaluated) of the partial-product path (csrc/gmm_flush.hip)."""
    v = [C.c_long(0) for _ in range(3)]
    lib().sr_flush_stats(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def kmeans_fast_stats():
    """(full nearest-centre searches of the k-means initialiser taken the fast way, points those left to the exact pass)"""
    v = [C.c_long(0) for _ in range(2)]
    lib().sr_kmeans_fast_stats(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def full_fit_batch_stats():
    """(sr_fullgmm_fit_batch calls that reached the device, speakers they carried, batch iterations launched)"""
    v = [C.c_long(0) for _ in range(3)]
    lib().sr_full_fit_batch_stats(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def full_fit_batch_bytes() -> int:
    """The current value of the option ``full_fit_batch_bytes``."""
    return int(lib().sr_full_fit_batch_bytes())


def full_fit_plan(K: int, D: int, lengths, init_given=None, max_iter=None, bound_bytes: int = 0) -> dict:
    """What a full-covariance fit of speakers of ``lengths`` frames decides before it touches the device (csrc/full_plan.cpp; no GPU
    needed): ``n_groups``, the lengths of the three work lists ``n_lp`` / ``n_lse`` / ``n_cov``, ``lds_logprob``, ``max_group_bytes``,
    ``lone_bytes`` (a speaker of ``lengths[0]`` frames alone); ``speakers`` [S, 8] = (frames, first row in its group, covariance
    chunks, frames per chunk, offset into ``partial``, bytes alone, group, slot); ``groups`` [G, 28] = (first speaker, speakers, rows,
    the three list ranges' starts, max_iter, any k-means start, any given start, bytes, then the 18 buffers' element counts).
    ``bound_bytes`` 0: the current ``full_fit_batch_bytes``."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    S = len(lengths)
    given = None if init_given is None else np.ascontiguousarray(init_given, dtype=np.int32)
    iters = None if max_iter is None else np.ascontiguousarray(max_iter, dtype=np.int32)
    as_ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    v = (C.c_int64 * 7)()
    spk = np.zeros((max(S, 1), 8), dtype=np.int64)
    args = (int(K), int(D), as_i64p(lengths), as_ip(given), as_ip(iters), S, int(bound_bytes))
    check(lib().sr_full_fit_plan(*args, as_i64p(spk), None, 0, v, 7), "sr_full_fit_plan")
    d = dict(zip(("n_groups", "n_lp", "n_lse", "n_cov", "lds_logprob", "max_group_bytes", "lone_bytes"), (int(x) for x in v)))
    groups = np.zeros((max(d["n_groups"], 1), 28), dtype=np.int64)
    check(lib().sr_full_fit_plan(*args, None, as_i64p(groups), d["n_groups"], v, 7), "sr_full_fit_plan")
    d.update(speakers=spk[:S], groups=groups[:d["n_groups"]])
    return d


def map_fit_batch_stats():
    """(sr_map_fit_batch calls that reached the device, speakers fitted in a batch, by the single fit, handed over, passes launched)"""
    v = [C.c_long(0) for _ in range(5)]
    lib().sr_map_fit_batch_stats(*[C.byref(x) for x in v])
    return tuple(int(x.value) for x in v)


def map_fit_batch_bytes() -> int:
    """The current value of the option ``map_fit_batch_bytes``."""
    return int(lib().sr_map_fit_batch_bytes())


def map_fit_plan(K: int, D: int, lengths, nr_iteration: int = 200, verbosity: int = 0, scratch_bytes: int = 1 << 30, n_cu: int = 256) -> dict:
    """What ``sr_map_fit_batch`` decides for a UBM of K mixtures in D dimensions and speakers of ``lengths`` frames (csrc/map_plan.cpp;
    no GPU needed when n_cu > 0): ``routes`` [S] (0 batched, 1 single, -1 failing), per speaker ``group``, ``slot``, ``n_pad``,
    ``n_chunks`` and ``scratch`` bytes, ``groups`` [G, 6] = (first speaker, speakers, density tiles = grid x, chunks = grid x, scratch
    bytes, first row of the density table), the tables ``tiles`` / ``chunks`` [n, 3] = (speaker, first row in the batch, local tile),
    the mixture blocks ``n_kb`` (every grid's y) and the LDS bytes of the two large kernels."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    S = len(lengths)
    p = Parameter()
    p.nr_iteration, p.verbosity = int(nr_iteration), int(verbosity)
    v = (C.c_int64 * 12)()
    spk = np.zeros((max(S, 1), 6), dtype=np.int64)
    args = (int(K), int(D), as_i64p(lengths), S, C.byref(p), int(scratch_bytes), int(n_cu))
    check(lib().sr_map_fit_plan(*args, as_i64p(spk), None, 0, None, 0, None, 0, v, 12), "sr_map_fit_plan")
    names = ("n_batched", "n_single", "n_error", "n_groups", "n_tiles", "n_chunks", "n_kb", "lds_density", "lds_stats", "max_group_bytes",
             "waves", "state_doubles")
    d = dict(zip(names, (int(x) for x in v)))
    groups = np.zeros((max(d["n_groups"], 1), 6), dtype=np.int64)
    tiles = np.zeros((max(d["n_tiles"], 1), 3), dtype=np.int64)
    chunks = np.zeros((max(d["n_chunks"], 1), 3), dtype=np.int64)
    check(lib().sr_map_fit_plan(*args, as_i64p(spk), as_i64p(groups), d["n_groups"], as_i64p(tiles), d["n_tiles"], as_i64p(chunks),
                                d["n_chunks"], v, 12), "sr_map_fit_plan")
    spk = spk[:S]
    d.update(routes=spk[:, 0].copy(), group=spk[:, 1].copy(), slot=spk[:, 2].copy(), n_pad=spk[:, 3].copy(), n_chunks_of=spk[:, 4].copy(),
             scratch=spk[:, 5].copy(), groups=groups[:d["n_groups"]], tiles=tiles[:d["n_tiles"]], chunks=chunks[:d["n_chunks"]])
    return d


def mfma_peak_probe(ms_target: float = 50.0):
    """(executed fp16 MFMA TFLOP/s, shader clock in MHz) of a kernel that only issues v_mfma_f32_32x32x16_f16, on the current
    device, for about ms_target milliseconds: what the matrix pipe sustains under the socket's power cap (csrc/probe.hip)."""
    t, f = C.c_double(0.0), C.c_double(0.0)
    check(lib().sr_mfma_peak_probe(C.c_double(ms_target), C.byref(t), C.byref(f)), "sr_mfma_peak_probe")
    return float(t.value), float(f.value)


def mfma_streamed_probe(ms_target: float = 50.0):
    """The same, with the chains fed as the scoring kernel feeds them: a fresh A fragment from LDS for every MFMA, random operand
    bits (csrc/probe.hip, mode 1)."""
    t, f = C.c_double(0.0), C.c_double(0.0)
    check(lib().sr_mfma_streamed_probe(C.c_double(ms_target), C.byref(t), C.byref(f)), "sr_mfma_streamed_probe")
    return float(t.value), float(f.value)


MFCC_KERNELS = ("fp32-fast", "fp32-generic", "f64-fast", "f64-generic")


def mfcc_plan(handle, precision: int = 2, generic: int = 0, pcm_kind: int = 0, n_frames: int = 1, n_cu: int = 0) -> dict:
    """What a pass of `n_frames` frames over the extractor `handle` (an SRMfcc *) launches (csrc/mfcc_plan.cpp): kernel and its
    template arguments, workgroup shape, LDS bytes, frames per wave, grid, cmvn_delta_kernel's column padding, and the padded mel
    layout.  n_cu > 0: that many compute units, no GPU needed; n_cu <= 0: the current device's."""
    v = (C.c_int32 * 16)()
    check(lib().sr_mfcc_plan(handle, int(precision), int(generic), int(pcm_kind), int(n_frames), int(n_cu), v, 16), "sr_mfcc_plan")
    names = ("kernel", "N1", "NZ1", "preset", "wpb", "lds", "frames_per_wave", "grid", "cp", "pad_floats")
    d = dict(zip(names, (int(x) for x in v[:10])))
    d["kernel"] = MFCC_KERNELS[d["kernel"]]
    d["pass_len"] = [int(x) for x in v[10:14]]
    d["max_read"] = int(v[14])
    d["n_empty"] = int(v[15])
    return d


def silence_plan(fs, frame_duration: float = 0.02, frame_shift: float = 0.01, max_samples: int = 1) -> dict:
    """What ``sr_silence_remove_batch`` decides for a longest utterance of ``max_samples`` under the current ``silence_block``
    option (csrc/silence_plan.cpp; no GPU needed): frame length L and shift S in samples, g = gcd(L, S), the width E of a
    block's transfer map, positions per block B, the blocks of that utterance and the shape of the maps launch."""
    v = (C.c_int32 * 12)()
    check(lib().sr_silence_plan(float(fs), float(frame_duration), float(frame_shift), int(max_samples), v, 12), "sr_silence_plan")
    names = ("L", "S", "g", "E", "B", "blocks", "variant", "blocks_per_wg", "list_cap", "grid", "chunk_lanes", "positions")
    return dict(zip(names, (int(x) for x in v)))


FEATURE_NORM_MODES = ("warp", "cmn", "cmvn")
FEATURE_NORM_PLAN_FIELDS = ("F", "span", "stride", "cols", "passes", "lds", "tiles", "grid", "table", "table_len", "workgroup", "max_window")


def feature_norm_mode(mode) -> int:
    """The C ABI's number of a normalisation mode name (-1 for anything else: the library refuses it)."""
    return FEATURE_NORM_MODES.index(mode) if isinstance(mode, str) and mode in FEATURE_NORM_MODES else -1


def feature_norm_plan(mode: str = "warp", window: int = 301, dim: int = 39, max_frames: int = 1, n_cu: int = 256) -> dict:
    """What ``sr_feature_norm_batch`` decides for columns of width ``dim`` and a longest utterance of ``max_frames`` under the
    current ``norm_tile`` option (csrc/featnorm_plan.cpp; no GPU needed when n_cu > 0): the refusals, frames per workgroup ``F``,
    the rows a workgroup stages at most, the column stride in LDS, columns per pass and passes, LDS bytes, the workgroups of that
    utterance and the grid, whether full windows read their warped values from a table, and the built limits."""
    v = (C.c_int32 * 12)()
    check(lib().sr_feature_norm_plan(feature_norm_mode(mode), int(window), int(dim), int(max_frames), int(n_cu), v, 12), "sr_feature_norm_plan")
    return dict(zip(FEATURE_NORM_PLAN_FIELDS, (int(x) for x in v)))


TIMELINE_MODES = ("none", "hold", "viterbi")       # the C ABI's modes 0 (raw), 1, 2 under the names of ``smooth=``
TIMELINE_PLAN_FIELDS = ("windows", "variant", "lanes", "states_per_lane", "tile", "chain_slots", "chain_lds", "fwd_lds", "sum_span", "sum_chunk",
                        "sum_lds", "sum_grid_x", "sum_grid_y", "bp_bytes", "max_states", "max_min_dur")


def timeline_mode(smooth) -> int:
    """The C ABI's number of a smoothing name (-1 for anything else: the library refuses it)."""
    return TIMELINE_MODES.index(smooth) if isinstance(smooth, str) and smooth in TIMELINE_MODES else -1


def timeline_windows(n_frames: int, window: int, hop: int) -> int:
    """Windows of a recording of ``n_frames``: 0 if empty, else 1 + ceil(max(0, n - W) / H), and with W < H no window that
    would start at or behind frame n (sr_timeline_windows; no GPU needed)."""
    return int(lib().sr_timeline_windows(int(n_frames), int(window), int(hop)))


def timeline_plan(S: int, min_dur: int = 1, n_frames: int = 0, window: int = 150, hop: int = 40) -> dict:
    """What the timeline decides for ``S`` columns, a minimum turn of ``min_dur`` windows and a recording of ``n_frames``
    (csrc/timeline_plan.cpp; no GPU needed): the windows, the forward kernel's variant, lanes, states per lane and tile, the ring of
    the minimum-duration chain, LDS bytes, the sum kernel's span, chunk, LDS bytes and grid, back-pointer bytes per window, limits."""
    v = (C.c_int32 * 16)()
    check(lib().sr_timeline_plan(int(S), int(min_dur), int(n_frames), int(window), int(hop), v, 16), "sr_timeline_plan")
    return dict(zip(TIMELINE_PLAN_FIELDS, (int(x) for x in v)))


def timeline_decide(sums, counts, win_off, bg: int = -1, threshold: float = 0.0, mode: int = 0, beta: float = 0.0, min_dur: int = 1):
    """``sr_timeline_decide`` on window sums [Nw_total, S] in host memory, their frame counts and the recordings' window offsets
    [U + 1]: -> (labels [Nw_total] int32, path scores [U], NaN-window counts [U])."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.ndim != 2:
        raise ValueError("expected sums [windows, columns], got shape %r" % (sums.shape,))
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    win_off = np.ascontiguousarray(win_off, dtype=np.int64)
    U = len(win_off) - 1
    if U < 0 or len(counts) != len(sums) or (U >= 0 and int(win_off[-1]) != len(sums)):
        raise ValueError("counts, sums and window offsets do not agree")
    labels = np.zeros(len(sums), dtype=np.int32)
    path = np.zeros(max(U, 1), dtype=np.float64)
    bad = np.zeros(max(U, 1), dtype=np.int64)
    check(lib().sr_timeline_decide(as_dp(sums), as_i32p(counts), as_i64p(win_off), U, sums.shape[1], int(bg), float(threshold), int(mode),
                                   float(beta), int(min_dur), as_i32p(labels), as_dp(path), as_i64p(bad)),
          "sr_timeline_decide")
    return labels, path[:U], bad[:U]


DIAR_CHANGE_MODES = ("uniform", "bic")
AHC_LINKAGES = ("average", "complete", "single")
DIAR_PLAN_FIELDS = ("bucket", "stat_len", "entries_per_lane", "stats_wg", "stats_chunk", "stats_lds", "change_lds", "groups", "max_dim",
                    "max_init", "waves", "argmin_blocks", "cadence", "bytes", "bound")


def diar_change_mode(change) -> int:
    """The C ABI's number of a change-detection name (-1 for anything else: the library refuses it)."""
    return DIAR_CHANGE_MODES.index(change) if isinstance(change, str) and change in DIAR_CHANGE_MODES else -1


def ahc_linkage(linkage) -> int:
    return AHC_LINKAGES.index(linkage) if isinstance(linkage, str) and linkage in AHC_LINKAGES else -1


def diar_segments(n_frames: int, L: int) -> int:
    """Base segments of a recording of ``n_frames``: floor(n / L), 1 if that is 0 and n > 0 (sr_diar_segments; no GPU needed)."""
    return int(lib().sr_diar_segments(int(n_frames), int(L)))


def diar_stat_len(D: int) -> int:
    return 1 + D + D * (D + 1) // 2


def diar_plan(D: int, lengths=(), L: int = 100, change: str = "bic", scratch_bytes: int = 0) -> dict:
    """What the diarisation decides for ``D`` dimensions and recordings of ``lengths`` frames (csrc/diar_plan.cpp; no GPU needed):
    the factorisation's bucket width, the layout of a statistic, the kernels' shapes, the grouping of the recordings under the bound
    (``scratch_bytes`` 0: the option diar_scratch_mib), per recording its base segments, the most initial clusters and its bytes;
    ``edges``: the initial-cluster counts at which a kernel's indexing wraps (waves per workgroup, argmin workgroups, its lanes)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    U = len(lengths)
    v = (C.c_int64 * 16)()
    groups = np.zeros(U + 1, dtype=np.int32)
    rec = np.zeros((max(U, 1), 3), dtype=np.int64)
    n = check(lib().sr_diar_plan(int(D), int(L), diar_change_mode(change), as_i64p(lengths), U, int(scratch_bytes), v, 16,
                                 groups.ctypes.data_as(C.POINTER(C.c_int32)), as_i64p(rec)), "sr_diar_plan")
    out = dict(zip(DIAR_PLAN_FIELDS, (int(x) for x in v)))
    out["group_begin"] = groups[:n + 1].tolist() if U else []
    out["n_seg"], out["n_init_bound"], out["rec_bytes"] = (rec[:U, k].tolist() for k in range(3))
    out["edges"] = [out["waves"], out["argmin_blocks"], out["stats_wg"]]
    return out


def diar_bic_matrix(stats, D: int, penalty: float = 1.0, ridge: float = 1e-3):
    """``sr_diar_bic_matrix`` on statistics [n, 1 + D + D (D + 1) / 2] in host memory: -> (delta-BIC [n, n], logdets [n] with NaN
    where the factorisation failed, the count of those)."""
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    if stats.ndim != 2 or (1 <= int(D) <= 64 and stats.shape[1] != diar_stat_len(int(D))):
        raise ValueError("expected statistics [clusters, 1 + D + D (D + 1) / 2], got shape %r for D = %r" % (stats.shape, D))
    n = len(stats)
    out = np.zeros((n, n), dtype=np.float64)
    ld = np.zeros(max(n, 1), dtype=np.float64)
    nf = C.c_int64(0)
    check(lib().sr_diar_bic_matrix(int(D), n, as_dp(stats), float(penalty), float(ridge), as_dp(out), as_dp(ld), C.byref(nf)),
          "sr_diar_bic_matrix")
    return out, ld[:n], int(nf.value)


def ahc_matrix(dist, linkage: int = 0, threshold: float = 0.0, k_min: int = 1, k_max: int = 0):
    """``sr_ahc_matrix``: -> (labels [n] int32, merge_i, merge_j, merge_d of the steps taken)."""
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError("expected a square dissimilarity matrix, got shape %r" % (dist.shape,))
    n = len(dist)
    mi = np.zeros(max(n - 1, 1), dtype=np.int32)
    mj = np.zeros(max(n - 1, 1), dtype=np.int32)
    md = np.zeros(max(n - 1, 1), dtype=np.float64)
    lab = np.zeros(max(n, 1), dtype=np.int32)
    nm, nc = C.c_int64(0), C.c_int64(0)
    check(lib().sr_ahc_matrix(n, as_dp(dist), int(linkage), float(threshold), int(k_min), int(k_max), as_i32p(mi), as_i32p(mj), as_dp(md),
                              C.byref(nm), as_i32p(lab), C.byref(nc)), "sr_ahc_matrix")
    t = int(nm.value)
    return lab[:n], mi[:t], mj[:t], md[:t]


def diar_cut(n: int, merge_i, merge_j, merge_d, threshold: float = 0.0, k_min: int = 1, k_max: int = 0):
    """``sr_diar_cut``: the labels [n] a stop rule gives on a merge log, and the steps it takes (no GPU needed)."""
    mi = np.ascontiguousarray(merge_i, dtype=np.int32).reshape(-1)
    mj = np.ascontiguousarray(merge_j, dtype=np.int32).reshape(-1)
    md = np.ascontiguousarray(merge_d, dtype=np.float64).reshape(-1)
    if not (len(mi) == len(mj) == len(md)):
        raise ValueError("the three columns of the merge log differ in length")
    lab = np.zeros(max(int(n), 1), dtype=np.int32)
    nm = C.c_int64(0)
    check(int(lib().sr_diar_cut(int(n), as_i32p(mi), as_i32p(mj), as_dp(md), len(mi), float(threshold), int(k_min), int(k_max), as_i32p(lab),
                                C.byref(nm))), "sr_diar_cut")
    return lab[:int(n)], int(nm.value)


def norm_quantile(p: float) -> float:
    """The standard normal quantile as the library computes it (AS241 in float64; csrc/norm_quantile.hpp); no GPU needed."""
    return float(lib().sr_norm_quantile(float(p)))


def topc_plan(K: int, D: int, S: int, top_c: int, n_frames: int, scratch_bytes: int = 1 << 30, n_cu: int = 256) -> dict:
    """What ``sr_score_batch_set_topc`` decides for a set of S models of K mixtures in D dimensions, `n_frames` frames and a scratch
    bound (csrc/topc_plan.cpp; no GPU needed when n_cu > 0): padded row width, the selection's register slots (0: the rank kernel),
    scratch bytes per frame, frames per chunk, chunks, and the shapes of the four stages' launches."""
    v = (C.c_int32 * 16)()
    check(lib().sr_topc_plan(int(K), int(D), int(S), int(top_c), int(n_frames), int(scratch_bytes), int(n_cu), v, 16), "sr_topc_plan")
    names = ("tp", "cr", "row_bytes", "chunk", "n_chunks", "run", "stage", "eval_waves", "eval_grid_x", "eval_grid_y", "select_grid",
             "route_grid", "combine_wg", "tile", "rank_lds")
    return dict(zip(names, (int(x) for x in v[:15])))


def bw_plan(K: int, D: int, lengths, range_frames: int = 0, scratch_bytes: int = 1 << 30, n_cu: int = 256, S: int = 1, model: int = 0,
            features: bool = True, feat_dim=None) -> dict:
    """What ``sr_bw_stats_batch`` decides for a model of K mixtures in D dimensions (model ``model`` of a set of S) and utterances of
    ``lengths`` frames (csrc/bw_plan.cpp; no GPU needed when n_cu > 0): the refusals, the padded row width, one range's slab, the
    range table ``ranges`` [n, 3] = (utterance, first row of the batch, rows), ranges per group, groups and the launch shapes."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    v = (C.c_int64 * 12)()
    args = (int(S), int(model), int(K), int(D), 1 if features else 0, int(D if feat_dim is None else feat_dim), as_i64p(lengths), len(lengths),
            int(range_frames), int(scratch_bytes), int(n_cu))
    check(lib().sr_bw_plan(*args, None, 0, v, 12), "sr_bw_plan")
    names = ("dp", "ncb", "n_mix_blocks", "slab_bytes", "n_ranges", "group_ranges", "n_groups", "lse_grid", "stats_lds", "reduce_blocks",
             "stats_rounds", "auto_range")
    d = dict(zip(names, (int(x) for x in v)))
    ranges = np.zeros((d["n_ranges"], 3), dtype=np.int64)
    check(lib().sr_bw_plan(*args, as_i64p(ranges), d["n_ranges"], v, 12), "sr_bw_plan")
    d["ranges"] = ranges
    return d


JFA_PLAN_FIELDS = ("chunk", "n_chunks", "bytes_N", "bytes_Fc", "bytes_E", "bytes_P", "bytes_A", "bytes_C", "bytes_W", "bytes_y",
                   "bytes_scratch", "path", "lds_rows", "gram_grid_x", "gram_grid_y", "gemm_L_x", "gemm_L_y", "gemm_b_x", "gemm_b_y",
                   "gemm_A_x", "gemm_A_y", "gemm_C_x", "gemm_C_y", "gram_lds", "gemm_lds", "factor_lds", "update_lds", "factor_rounds",
                   "k_step", "max_R", "max_lds_rows")


def jfa_plan(G: int, K: int, D: int, R: int, scratch_bytes: int = 1 << 30, lds_rows: int = 0, n_cu: int = 256) -> dict:
    """What ``sr_jfa_factors`` / ``sr_jfa_train`` decide for G groups, a K x D model and R factors under a scratch bound and the
    option ``jfa_lds_rows`` (csrc/jfa_plan.cpp; no GPU needed when n_cu > 0): the refusals, groups per chunk, chunks, the bytes of
    each resident array, the factorisation ``path`` ("lds" or "global"), the grids of the gram and the four GEMM launches, and
    every kernel's LDS bytes."""
    v = (C.c_int64 * 32)()
    check(lib().sr_jfa_plan(int(G), int(K), int(D), int(R), int(scratch_bytes), int(lds_rows), int(n_cu), v, 32), "sr_jfa_plan")
    d = dict(zip(JFA_PLAN_FIELDS, (int(x) for x in v)))
    d["path"] = ("lds", "global")[d["path"]]
    return d


JFA_SCORE_PLAN_FIELDS = ("mode", "chunk", "n_chunks", "seg_bytes", "bytes_scratch", "bytes_M", "bytes_ME", "bytes_uE", "bytes_P", "bytes_q",
                         "bytes_G", "bytes_N", "bytes_F", "bytes_lin", "bytes_quad", "bytes_a", "bytes_out", "bytes_comp", "path", "lds_rows",
                         "gemm_yv_x", "gemm_yv_y", "synth_grid", "scale_M_grid", "scale_u_grid", "gram_grid_x", "gram_grid_y", "cross_grid_x",
                         "cross_grid_y", "cross_grid_z", "gemm_L_x", "gemm_L_y", "gemm_a_x", "gemm_a_y", "gemm_lin_x", "gemm_lin_y", "gemm_quad_x",
                         "gemm_quad_y", "gemm_h_x", "gemm_h_y", "kscore_grid", "gemm_xu_x", "gemm_xu_y", "comp_grid", "gemm_out_x", "gemm_out_y",
                         "gram_lds", "gemm_lds", "cross_lds", "kscore_lds", "kscore_rounds", "max_R", "max_lds_rows", "max_J")


def jfa_centre_plan(n: int, n_labels: int, K: int, D: int, Ry: int = 0, Ru: int = 0, groups: str = "speakers", scratch_bytes: int = 1 << 30) -> dict:
    """What ``sr_jfa_open_centred`` decides for n sessions with labels below n_labels, a K x D model and y v / x u terms of Ry / Ru
    factors (0: absent) under a scratch bound (csrc/jfa_plan.cpp; host only): the refusals, sessions per chunk of the x u product,
    chunks, bytes, doubles per lane and the grids."""
    v = (C.c_int64 * 16)()
    check(lib().sr_jfa_centre_plan(int(n), int(n_labels), int(K), int(D), int(Ry), int(Ru), {"speakers": 0, "sessions": 1}.get(groups, -1),
                                   int(scratch_bytes), v, 16), "sr_jfa_centre_plan")
    keys = ("mode", "chunk", "n_chunks", "bytes_scratch", "bytes_N", "bytes_Fc", "bytes_yv", "bytes_z", "vec", "gemm_xu_x", "gemm_xu_y",
            "gemm_yv_x", "gemm_yv_y", "centre_x", "centre_y", "row_tile")
    return dict(zip(keys, (int(x) for x in v)))


def jfa_score_plan(T: int, J: int, K: int, D: int, Ry: int, Ru: int, mode: str = "integrated", scratch_bytes: int = 1 << 30, lds_rows: int = 0,
                   n_cu: int = 256) -> dict:
    """What ``sr_jfa_score_integrated`` / ``sr_jfa_score_linear`` decide for T test segments, J models, a K x D model, Ry eigenvoices
    and Ru eigenchannels under a scratch bound and the option ``jfa_lds_rows`` (csrc/jfa_plan.cpp; no GPU needed when n_cu > 0): the
    refusals, segments per chunk, chunks, a segment's bytes inside the bound, the bytes of every array outside it, the factorisation
    ``path`` ("lds" or "global"), the grid of every launch and every kernel's LDS bytes."""
    v = (C.c_int64 * 56)()
    check(lib().sr_jfa_score_plan(int(T), int(J), int(K), int(D), int(Ry), int(Ru), {"integrated": 0, "linear": 1}.get(mode, -1),
                                  int(scratch_bytes), int(lds_rows), int(n_cu), v, 56), "sr_jfa_score_plan")
    d = dict(zip(JFA_SCORE_PLAN_FIELDS, (int(x) for x in v)))
    d["path"] = ("lds", "global")[d["path"]]
    d["mode"] = ("integrated", "linear")[d["mode"]]
    return d


NORM_MODES = ("z", "t", "zt", "s", "as1", "as2")
NORM_PLAN_FIELDS = ("mode", "n_sel", "n_sel_test", "chunk", "n_chunks", "fixed_bytes", "seg_bytes", "bytes_scratch", "bytes_S", "bytes_Ez",
                    "bytes_Tt", "bytes_Zt", "bytes_out", "bytes_moments", "bytes_tnorm", "bytes_counts", "select_enrol_grid", "select_test_grid",
                    "select_zt_grid", "select_lds_enrol", "select_lds_test", "shift_enrol_grid", "shift_test_grid", "gemm_enrol_x", "gemm_enrol_y",
                    "gemm_test_x", "gemm_test_y", "gemm_lds", "apply_x", "apply_y", "select_rounds", "max_C", "max_rows", "workgroup")


def score_norm_plan(mode: str, J: int, T: int, Cz: int, Ct: int, top_n: int = 0, scratch_bytes: int = 1 << 30, n_cu: int = 256) -> dict:
    """What ``sr_score_norm`` decides for a J x T score matrix, cohorts of Cz and Ct members and a scratch bound (csrc/norm_plan.cpp;
    no GPU needed when n_cu > 0): the refusals, the values per moment pair, test segments per chunk and chunks (as2), the bytes of
    every array inside and outside the bound, the grid of every launch, the selection kernel's LDS bytes and the built limits."""
    v = (C.c_int64 * 40)()
    m = NORM_MODES.index(mode) if mode in NORM_MODES else -1
    check(lib().sr_score_norm_plan(m, int(J), int(T), int(Cz), int(Ct), int(top_n), int(scratch_bytes), int(n_cu), v, 40), "sr_score_norm_plan")
    d = dict(zip(NORM_PLAN_FIELDS, (int(x) for x in v)))
    d["mode"] = NORM_MODES[d["mode"]]
    return d


CALIB_CALLS = ("train", "apply", "counts")
CALIB_STOPS = ("CONVERGED", "CAP", "SINGULAR", "STALLED")
CALIB_PLAN_FIELDS = ("S", "n", "n_blocks", "acc", "state_len", "bytes_X", "bytes_lab", "bytes_partial", "bytes_state", "bytes_out", "bytes_thr",
                     "bytes_counts", "resident_train", "resident_apply", "resident_counts", "pass_grid", "step_grid", "apply_grid", "counts_grid",
                     "pass_rounds", "max_S", "max_thresholds", "block", "workgroup", "cadence", "max_pass", "max_n")


def calib_plan(S: int, n: int, n_thr: int = 0, call: str = "train", scratch_bytes: int = 0, n_cu: int = 256) -> dict:
    """What a calibration call decides for S systems and n trials (csrc/calib_plan.cpp; no GPU needed when n_cu > 0): the refusals, the
    blocks of 4096 trials, the accumulators and the state length, the bytes of every array, each call's resident bytes, the grids and the
    built limits.  ``scratch_bytes`` > 0: refuse as ``call`` ("train" -- also evaluation --, "apply" or "counts") under that bound would."""
    v = (C.c_int64 * 28)()
    c = CALIB_CALLS.index(call) if call in CALIB_CALLS else -1
    check(lib().sr_calib_plan(int(S), int(n), int(n_thr), c, int(scratch_bytes), int(n_cu), v, 28), "sr_calib_plan")
    return dict(zip(CALIB_PLAN_FIELDS, (int(x) for x in v)))


PLDA_PLAN_FIELDS = ("kind", "R", "rows", "groups", "T", "n_classes", "sum_chunk", "sum_chunks", "grp_chunk", "grp_chunks", "chunk", "n_chunks",
                    "seg_bytes", "bytes_scratch", "bytes_blocks", "bytes_rows", "path", "lds_rows", "factor_lds", "gemm_lds", "centre_grid",
                    "class_sums_x", "class_sums_y", "invert_grid", "gemm_rows_x", "gemm_rows_y", "gemm_acc_x", "gemm_acc_y", "rowdot_grid",
                    "gemm_cross_x", "gemm_cross_y", "assemble_grid", "invert_rounds", "max_R", "max_rows", "tri_inverse_y")


def plda_plan(kind: str, R: int, counts, T: int = 0, n_labels=None, scratch_bytes: int = 1 << 30, lds_rows: int = 0, n_cu: int = 256) -> dict:
    """What ``sr_plda_train`` (``kind`` "train": ``counts`` the 0-based labels, one per training vector) or ``sr_plda_score`` ("score":
    ``counts`` the models' enrolment counts, ``T`` test segments) decides (csrc/plda_plan.cpp; no GPU needed when n_cu > 0): the
    refusals, the count classes ("classes": (count, first sorted position, size), ascending count) and the permutation that sorts
    the speakers or models by count ("perm": sorted position -> label or model), the chunks, the factorisation path, the bytes, the
    grid of every launch and the built limits."""
    counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int64)
    k = ("train", "score").index(kind) if kind in ("train", "score") else -1
    rows = int(counts.size)
    groups = rows if k != 0 else int(n_labels if n_labels is not None else (counts.max() + 1 if rows else 0))
    width = max(1, min(groups, rows) if k == 0 else rows)
    v, perm, classes = (C.c_int64 * 36)(), np.zeros(width, dtype=np.int64), np.zeros(3 * width, dtype=np.int64)
    check(lib().sr_plda_plan(k, int(R), rows, groups, int(T), as_i64p(counts), int(scratch_bytes), int(lds_rows), int(n_cu), v, 36, as_i64p(perm),
                             as_i64p(classes)), "sr_plda_plan")
    d = dict(zip(PLDA_PLAN_FIELDS, (int(x) for x in v)))
    d["kind"] = kind
    d["perm"] = perm[:d["groups"]]
    d["classes"] = [tuple(int(x) for x in classes[3 * c:3 * c + 3]) for c in range(d["n_classes"])]
    return d


EIG_PLAN_FIELDS = ("R", "b", "blocks", "phantom", "rounds", "pairs", "single", "max_sweeps", "inner_sweeps", "solve_lds", "update_lds", "solve_grid",
                   "cols_x", "cols_y", "cols_z", "rows_x", "rows_y", "launches_per_sweep", "bytes_work", "pair_rounds", "max_R", "tile_rows",
                   "sub_problem", "wg")


def eig_plan(R: int, n_cu: int = 256) -> dict:
    """What ``sr_sym_eig`` decides for an R x R matrix (csrc/eig_plan.cpp; no GPU needed when n_cu > 0): the block width ``b``, the
    blocks and the phantom, the rounds and pairs of a sweep, the single-launch path, the caps, the LDS bytes, the grids, and
    "schedule": [rounds][pairs] block pairs (p, q), p < q, q == blocks naming the phantom (that pair does no work)."""
    v = (C.c_int64 * 24)()
    sched = np.zeros(2 * 16 * 8 + 2, dtype=np.int32)
    check(lib().sr_eig_plan(int(R), int(n_cu), v, 24, as_i32p(sched)), "sr_eig_plan")
    d = dict(zip(EIG_PLAN_FIELDS, (int(x) for x in v)))
    d["schedule"] = [[(int(sched[2 * (r * d["pairs"] + k)]), int(sched[2 * (r * d["pairs"] + k) + 1])) for k in range(d["pairs"])]
                     for r in range(d["rounds"])]
    return d


def multi_plan(offsets, devices, merge: bool = True, schedules=None) -> list:
    """What ``sr_multi_predict_pcm`` decides for utterances at the cumulative sample ``offsets`` over slots on ``devices`` (one device
    index per slot) before it touches a GPU (csrc/multi_plan.cpp; no GPU needed): for every slot that takes work a dict of its
    ``slot`` index, its utterances ``utts`` (ascending) and its ``pieces`` [(u0, u1), ...], ranges of that list.  ``schedules``: a
    slot's piece schedule, 0 (nearly equal pieces, the default) or 1 (growing ones)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    devices = np.ascontiguousarray(devices, dtype=np.int32)
    n_utt, n_slots = len(offsets) - 1, len(devices)
    sched = np.ascontiguousarray(schedules if schedules is not None else np.zeros(n_slots), dtype=np.int32)
    if n_utt < 0 or len(sched) != n_slots:
        raise ValueError("offsets holds U + 1 values, schedules one per slot")
    active, counts = np.zeros(max(1, n_slots), np.int32), np.zeros(max(1, n_slots), np.int32)
    utts, pieces = np.zeros(max(1, n_utt), np.int32), np.zeros((max(1, n_slots), 17), np.int32)
    n = check(lib().sr_multi_plan(as_i64p(offsets), n_utt, as_i32p(devices), n_slots, 1 if merge else 0, as_i32p(sched), as_i32p(active),
                                  as_i32p(counts), as_i32p(utts), as_i32p(pieces)), "sr_multi_plan")
    ends = np.cumsum(counts[:n])
    return [{"slot": int(active[a]), "utts": utts[ends[a] - counts[a]:ends[a]].tolist(),
             "pieces": [(int(pieces[a, 1 + 2 * c]), int(pieces[a, 2 + 2 * c])) for c in range(pieces[a, 0])]} for a in range(n)]


def last_score_kernel() -> str:
    return lib().sr_last_score_kernel().decode()


def last_em_stats_engine() -> int:
    """1 vector ALU, 2 fp64 matrix cores, 3 the same with the responsibilities on the 16-bit matrix cores (0: no E-step yet)"""
    return int(lib().sr_last_em_stats_engine())


def profile_enable(on: bool = True) -> None:
    lib().sr_profile_enable(1 if on else 0)


def profile_reset() -> None:
    check(lib().sr_profile_reset(), "sr_profile_reset")


def profile_get(kind: int):
    ms = C.c_double(0)
    n = C.c_long(0)
    check(lib().sr_profile_get(kind, C.byref(ms), C.byref(n)), "sr_profile_get")
    return ms.value, n.value

"""ctypes binding of include/rustpotter_hip.h.

Class and method names follow the reference's public API (src/lib.rs:8-21,
src/detector.rs, src/config.rs) so that the parity tests read like the reference's
own tests (tests/detector.rs).
"""
import ctypes as C
import weakref
import enum
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class RustpotterError(RuntimeError):
    """Result::Err(String) of the reference."""


def lib_path():
    # RP_LIB_PATH: load another build of the same library (kernel experiments under tools/scratch); the product is the in-tree one
    return os.environ.get("RP_LIB_PATH") or os.path.join(_HERE, "librustpotter_hip.so")


class SampleFormat(enum.IntEnum):  # src/audio/audio_types.rs:4-9
    I8 = 0
    I16 = 1
    I32 = 2
    F32 = 3


class Endianness(enum.IntEnum):  # src/audio/audio_types.rs:52-56
    Big = 0
    Little = 1
    Native = 2


class ScoreMode(enum.IntEnum):  # src/config.rs:86-96
    Average = 0
    Max = 1
    Median = 2
    P25 = 3
    P50 = 4
    P75 = 5
    P80 = 6
    P90 = 7
    P95 = 8


class VADMode(enum.IntEnum):  # src/config.rs:134-138 (+ None)
    Off = 0
    Easy = 1
    Medium = 2
    Hard = 3


class _AudioFmt(C.Structure):
    _fields_ = [("sample_rate", C.c_size_t), ("sample_format", C.c_int), ("channels", C.c_uint16), ("endianness", C.c_int)]


class _DetectorConfig(C.Structure):
    _fields_ = [("avg_threshold", C.c_float), ("threshold", C.c_float), ("min_scores", C.c_size_t), ("eager", C.c_bool),
                ("score_ref", C.c_float), ("band_size", C.c_uint16), ("score_mode", C.c_int), ("vad_mode", C.c_int)]


class _GainCfg(C.Structure):
    _fields_ = [("enabled", C.c_bool), ("has_gain_ref", C.c_bool), ("gain_ref", C.c_float), ("min_gain", C.c_float),
                ("max_gain", C.c_float)]


class _BandPassCfg(C.Structure):
    _fields_ = [("enabled", C.c_bool), ("low_cutoff", C.c_float), ("high_cutoff", C.c_float)]


class _FiltersCfg(C.Structure):
    _fields_ = [("gain_normalizer", _GainCfg), ("band_pass", _BandPassCfg)]


class _Config(C.Structure):
    _fields_ = [("fmt", _AudioFmt), ("detector", _DetectorConfig), ("filters", _FiltersCfg)]


class _Detection(C.Structure):
    _fields_ = [("name", C.c_char_p), ("avg_score", C.c_float), ("score", C.c_float), ("n_scores", C.c_size_t),
                ("score_names", C.POINTER(C.c_char_p)), ("scores", C.POINTER(C.c_float)), ("counter", C.c_size_t),
                ("gain", C.c_float)]


class _TrainOptions(C.Structure):
    _fields_ = [("m_type", C.c_int), ("learning_rate", C.c_float), ("epochs", C.c_size_t), ("test_epochs", C.c_size_t),
                ("mfcc_size", C.c_uint16), ("seed", C.c_uint64)]


class _BatchDetection(C.Structure):
    _fields_ = [("stream", C.c_int32), ("frame", C.c_int32), ("window", C.c_int32), ("counter", C.c_int32),
                ("avg_score", C.c_float), ("score", C.c_float)]


# every symbol include/rustpotter_hip.h declares (tests/test_capi_symbols.py checks the header against this)
SYMBOLS = [
    "rp_config_default", "rp_new", "rp_free", "rp_add_wakeword_from_buffer", "rp_add_wakeword_from_file",
    "rp_remove_wakeword", "rp_remove_wakewords", "rp_get_samples_per_frame", "rp_get_bytes_per_frame",
    "rp_get_partial_detection", "rp_get_rms_level", "rp_get_gain", "rp_get_rms_level_ref", "rp_process_bytes",
    "rp_process_samples_i8", "rp_process_samples_i16", "rp_process_samples_i32", "rp_process_samples_f32",
    "rp_update_config", "rp_update_detector_config", "rp_update_filters_config", "rp_reset", "rp_last_error",
    "rp_ctx_new", "rp_ctx_free", "rp_ctx_set_stream", "rp_ctx_synchronize", "rp_ctx_dtw_ref_pairs", "rp_ctx_dtw_kernels", "rp_ctx_last_window_scores", "rp_ctx_set_arithmetic", "rp_ctx_arithmetic", "rp_ctx_last_mlp_kernel", "rp_build_info", "rp_sharded_gather_info", "rp_mfcc_num_frames", "rp_mfcc_batch", "rp_mfcc_batch_fmt", "rp_batch_detect_fmt", "rp_batch_detect_ingest", "rp_frontend_batch", "rp_wakeword_ref_build", "rp_buffer_free",
    "rp_mfcc_average_batch", "rp_wakeword_ref_build_batch",
    "rp_templates_new", "rp_templates_free", "rp_templates_max_len", "rp_dtw_score_batch", "rp_detect_scan", "rp_batch_detect",
    "rp_model_new", "rp_model_free", "rp_mlp_forward_batch", "rp_mlp_forward_windows", "rp_synth_pcm_batch", "rp_ctx_timing_enable", "rp_ctx_timing_read", "rp_ctx_timing_reset",
    "rp_version", "rp_stream_batch_new", "rp_stream_batch_free", "rp_stream_batch_process", "rp_stream_batch_reset",
    "rp_stream_batch_chunks_seen", "rp_resampler_frame_lengths", "rp_resample_batch",
    "rp_wakeword_model_train", "rp_wakeword_model_train_batch", "rp_mlp_train_batch", "rp_train_batch_last_profile", "rp_stream_batch_set_input", "rp_stream_batch_samples_per_chunk",
    "rp_batch_detect_multi", "rp_batch_detect_model", "rp_batch_detect_sharded",
    "rp_stream_batch_new_multi", "rp_stream_batch_process_multi",
    "rp_stream_batch_set_filters", "rp_stream_batch_levels",
    "rp_wakeword_bank_new", "rp_wakeword_bank_new_from_rpw", "rp_wakeword_bank_free", "rp_wakeword_bank_max_len", "rp_dtw_score_bank",
    "rp_batch_detect_bank", "rp_stream_batch_new_bank", "rp_stream_batch_set_wakewords",
    "rp_wakeword_bank_set_rms_levels", "rp_wakeword_bank_rms_level", "rp_frontend_batch_bank", "rp_stream_batch_set_filters_bank",
    "rp_wakeword_bank_reserve", "rp_wakeword_bank_size", "rp_wakeword_bank_reserved_len", "rp_wakeword_bank_pool_growths",
    "rp_wakeword_bank_put", "rp_wakeword_bank_put_from_rpw", "rp_wakeword_bank_enrol",
    "rp_dtw_score_bank_sets", "rp_batch_detect_bank_sets", "rp_stream_batch_new_bank_sets", "rp_stream_batch_set_wakeword_sets",
    "rp_stream_batch_slot_scores",
    "rp_model_bank_new", "rp_model_bank_new_from_rpw", "rp_model_bank_free", "rp_model_bank_size", "rp_model_bank_train_size",
    "rp_model_bank_labels", "rp_mlp_forward_windows_bank", "rp_batch_detect_model_bank",
    "rp_model_bank_reserve", "rp_model_bank_reserved", "rp_model_bank_pool_growths", "rp_model_bank_put", "rp_model_bank_put_from_rpw",
    "rp_model_bank_train", "rp_model_bank_read_image", "rp_model_bank_last_put_ms",
    "rp_stream_batch_new_model_bank", "rp_stream_batch_set_models", "rp_stream_batch_logits",
    "rp_mlp_forward_windows_bank_sets", "rp_batch_detect_model_bank_sets", "rp_stream_batch_new_model_bank_sets", "rp_stream_batch_set_model_sets",
    "rp_model_bank_set_rms_levels", "rp_model_bank_rms_level", "rp_frontend_batch_bank_sets", "rp_frontend_batch_model_bank",
    "rp_stream_batch_set_filters_per_stream",
    "rp_batch_detect_mixed_sets", "rp_frontend_batch_mixed_sets", "rp_stream_batch_new_mixed_sets", "rp_stream_batch_set_mixed_sets",
]


class _WakewordSpec(C.Structure):  # rp_wakeword_spec
    _fields_ = [("templates", C.c_void_p), ("model", C.c_void_p), ("none_index", C.c_int), ("precision", C.c_int),
                ("threshold", C.c_float), ("avg_threshold", C.c_float)]


def load_library():
    """Loads librustpotter_hip.so.  torch (if importable) is imported FIRST so that the
    process uses torch's bundled HIP runtime (same SONAME libamdhip64.so.7) instead of
    loading a second one."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RustpotterError(
            "librustpotter_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C rustpotter_amd/csrc`; there is no CPU fallback" % path)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for pure C users
        pass
    L = C.CDLL(path)
    vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.rp_last_error.restype = C.c_char_p
    L.rp_version.restype = C.c_char_p
    L.rp_config_default.argtypes = [C.POINTER(_Config)]
    L.rp_new.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    L.rp_free.argtypes = [vp]
    L.rp_add_wakeword_from_buffer.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_size_t]
    L.rp_add_wakeword_from_file.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.rp_remove_wakeword.argtypes = [vp, C.c_char_p]
    L.rp_remove_wakeword.restype = C.c_bool
    L.rp_remove_wakewords.argtypes = [vp]
    L.rp_remove_wakewords.restype = C.c_bool
    L.rp_get_samples_per_frame.argtypes = [vp]
    L.rp_get_samples_per_frame.restype = C.c_size_t
    L.rp_get_bytes_per_frame.argtypes = [vp]
    L.rp_get_bytes_per_frame.restype = C.c_size_t
    L.rp_get_partial_detection.argtypes = [vp, C.POINTER(_Detection)]
    for n in ("rp_get_rms_level", "rp_get_gain", "rp_get_rms_level_ref"):
        getattr(L, n).argtypes = [vp]
        getattr(L, n).restype = C.c_float
    L.rp_process_bytes.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(_Detection)]
    for n in ("rp_process_samples_i8", "rp_process_samples_i16", "rp_process_samples_i32", "rp_process_samples_f32"):
        getattr(L, n).argtypes = [vp, vp, C.c_size_t, C.POINTER(_Detection)]
    L.rp_update_config.argtypes = [vp, C.POINTER(_Config)]
    L.rp_update_detector_config.argtypes = [vp, C.POINTER(_DetectorConfig)]
    L.rp_update_filters_config.argtypes = [vp, C.POINTER(_FiltersCfg)]
    L.rp_reset.argtypes = [vp]
    L.rp_ctx_new.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.rp_ctx_free.argtypes = [vp]
    L.rp_ctx_set_stream.argtypes = [vp, vp]
    L.rp_ctx_synchronize.argtypes = [vp]
    L.rp_ctx_dtw_ref_pairs.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rp_ctx_dtw_kernels.argtypes = [vp]
    L.rp_ctx_dtw_kernels.restype = C.c_int
    L.rp_ctx_last_window_scores.argtypes = [vp, vp, C.c_size_t]
    L.rp_ctx_set_arithmetic.argtypes = [vp, C.c_int, C.c_int]
    L.rp_ctx_set_arithmetic.restype = C.c_int
    L.rp_ctx_arithmetic.argtypes = [vp, C.POINTER(C.c_int)]
    L.rp_ctx_arithmetic.restype = C.c_int
    L.rp_sharded_gather_info.argtypes = []
    L.rp_sharded_gather_info.restype = C.c_char_p
    L.rp_build_info.argtypes = []
    L.rp_build_info.restype = C.c_char_p
    L.rp_ctx_last_mlp_kernel.argtypes = [vp]
    L.rp_ctx_last_mlp_kernel.restype = C.c_char_p
    L.rp_mfcc_num_frames.argtypes = [C.c_size_t]
    L.rp_mfcc_num_frames.restype = C.c_size_t
    L.rp_mfcc_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.rp_mfcc_batch_fmt.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.rp_batch_detect_fmt.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.POINTER(_DetectorConfig), vp, vp, C.c_int, vp, vp]
    L.rp_batch_detect_ingest.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.POINTER(_DetectorConfig), vp, vp, C.c_int, C.c_size_t,
                                         C.POINTER(C.c_double)]
    L.rp_frontend_batch.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_FiltersCfg), C.c_float, C.c_size_t, vp, C.c_size_t, vp, vp]
    L.rp_wakeword_ref_build.argtypes = [vp, C.c_char_p, fp, fp, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                        C.POINTER(C.c_size_t), C.c_uint16, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rp_buffer_free.argtypes = [vp]
    L.rp_mfcc_average_batch.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), fp, fp]
    L.rp_wakeword_ref_build_batch.argtypes = [vp, C.c_size_t, C.POINTER(C.c_char_p), fp, fp, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p),
                                              C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_uint16, C.c_int, C.POINTER(vp),
                                              C.POINTER(C.c_size_t)]
    L.rp_templates_new.argtypes = [vp, C.c_int, C.c_int, ip, fp, C.c_int, fp, C.POINTER(vp)]
    L.rp_templates_free.argtypes = [vp]
    L.rp_templates_max_len.argtypes = [vp]
    L.rp_dtw_score_batch.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, C.c_float, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.rp_detect_scan.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(_DetectorConfig), C.c_int, vp, C.c_int, vp, vp, C.c_int]
    L.rp_batch_detect.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.POINTER(_DetectorConfig), vp, vp, C.c_int, vp, vp]
    L.rp_wakeword_model_train.argtypes = [vp, C.POINTER(_TrainOptions), C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                          C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p),
                                          C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t), fp, fp]
    L.rp_wakeword_model_train_batch.argtypes = [vp, C.POINTER(_TrainOptions), C.c_size_t, C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                                C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t), fp, fp]
    L.rp_mlp_train_batch.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), fp,
                                     C.POINTER(C.c_int32), fp, C.c_float, C.c_size_t, fp]
    L.rp_train_batch_last_profile.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.rp_batch_detect_multi.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(vp),
                                        C.POINTER(_DetectorConfig), fp, fp, vp, vp, vp, C.c_int]
    L.rp_batch_detect_sharded.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.POINTER(C.c_size_t), C.c_size_t,
                                          C.c_size_t, C.POINTER(_DetectorConfig), vp, vp, C.c_int]
    L.rp_batch_detect_model.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_int, C.c_int,
                                        C.POINTER(_DetectorConfig), C.c_int, vp, vp, vp, C.c_int]
    L.rp_resampler_frame_lengths.argtypes = [C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.rp_resample_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, vp, C.c_size_t]
    L.rp_stream_batch_new.argtypes = [vp, vp, C.POINTER(_DetectorConfig), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_new_multi.argtypes = [vp, C.c_size_t, C.POINTER(_WakewordSpec), C.c_int, C.POINTER(_DetectorConfig), C.c_size_t,
                                            C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_process_multi.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, vp, vp, vp, vp, C.c_int]
    L.rp_stream_batch_free.argtypes = [vp]
    L.rp_stream_batch_free.restype = None
    L.rp_stream_batch_process.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, vp, vp, C.c_int, vp]
    L.rp_stream_batch_reset.argtypes = [vp, C.c_longlong]
    L.rp_stream_batch_set_input.argtypes = [vp, C.c_size_t, C.c_int]
    L.rp_stream_batch_set_filters.argtypes = [vp, C.POINTER(_FiltersCfg), C.c_float]
    L.rp_stream_batch_levels.argtypes = [vp, vp, vp]
    L.rp_stream_batch_samples_per_chunk.argtypes = [vp]
    L.rp_stream_batch_samples_per_chunk.restype = C.c_size_t
    L.rp_stream_batch_chunks_seen.argtypes = [vp]
    L.rp_stream_batch_chunks_seen.restype = C.c_size_t
    L.rp_model_new.argtypes = [vp, C.c_int, ip, C.POINTER(fp), C.POINTER(fp), C.POINTER(vp)]
    L.rp_model_free.argtypes = [vp]
    L.rp_mlp_forward_batch.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp]
    L.rp_mlp_forward_windows.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp]
    L.rp_synth_pcm_batch.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_size_t, C.c_size_t, C.c_size_t, vp]
    L.rp_ctx_timing_enable.argtypes = [vp, C.c_int]
    L.rp_ctx_timing_read.argtypes = [vp, C.c_int, C.POINTER(C.c_double), ip]
    L.rp_ctx_timing_reset.argtypes = [vp]
    i32p = C.POINTER(C.c_int32)
    L.rp_wakeword_bank_new.argtypes = [vp, C.c_size_t, C.c_int, i32p, i32p, fp, i32p, fp, fp, fp, C.POINTER(vp)]
    L.rp_wakeword_bank_new_from_rpw.argtypes = [vp, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.rp_wakeword_bank_free.argtypes = [vp]
    L.rp_wakeword_bank_free.restype = None
    L.rp_wakeword_bank_max_len.argtypes = [vp, C.c_longlong]
    L.rp_model_bank_new.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.c_int, i32p, C.POINTER(vp)]
    L.rp_model_bank_new_from_rpw.argtypes = [vp, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(vp)]
    L.rp_model_bank_free.argtypes = [vp]
    L.rp_model_bank_free.restype = None
    L.rp_model_bank_size.argtypes = [vp]
    L.rp_model_bank_train_size.argtypes = [vp, C.c_longlong]
    L.rp_model_bank_labels.argtypes = [vp, C.c_longlong]
    L.rp_model_bank_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t]
    L.rp_model_bank_reserved.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rp_model_bank_pool_growths.argtypes = [vp]
    L.rp_model_bank_put.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(vp), i32p]
    L.rp_model_bank_put_from_rpw.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
    L.rp_model_bank_train.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(_TrainOptions), C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t), fp, fp]
    L.rp_model_bank_read_image.argtypes = [vp, C.c_longlong, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rp_model_bank_last_put_ms.argtypes = [vp]
    L.rp_model_bank_last_put_ms.restype = C.c_double
    L.rp_mlp_forward_windows_bank.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t]
    L.rp_batch_detect_model_bank.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(_DetectorConfig), C.c_int,
                                             vp, vp, vp, C.c_int]
    L.rp_wakeword_bank_set_rms_levels.argtypes = [vp, fp]
    L.rp_wakeword_bank_rms_level.argtypes = [vp, C.c_longlong]
    L.rp_wakeword_bank_rms_level.restype = C.c_float
    L.rp_wakeword_bank_reserve.argtypes = [vp, C.c_int, C.c_size_t, C.c_size_t]
    L.rp_wakeword_bank_size.argtypes = [vp]
    L.rp_wakeword_bank_reserved_len.argtypes = [vp]
    L.rp_wakeword_bank_pool_growths.argtypes = [vp]
    L.rp_wakeword_bank_put.argtypes = [vp, C.c_size_t, C.c_size_t, i32p, i32p, fp, i32p, fp, fp, fp, fp]
    L.rp_wakeword_bank_put_from_rpw.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
    L.rp_wakeword_bank_enrol.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_char_p), fp, fp, C.POINTER(C.c_size_t), C.POINTER(C.c_char_p),
                                         C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.rp_frontend_batch_bank.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_FiltersCfg), vp, vp, vp, C.c_size_t, vp, vp]
    L.rp_stream_batch_set_filters_bank.argtypes = [vp, C.POINTER(_FiltersCfg)]
    L.rp_dtw_score_bank.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_float, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t]
    L.rp_batch_detect_bank.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(_DetectorConfig), vp, vp, C.c_int,
                                       vp, vp, C.c_size_t]
    L.rp_stream_batch_new_bank.argtypes = [vp, vp, vp, C.POINTER(_DetectorConfig), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_set_wakewords.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.rp_dtw_score_bank_sets.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t]
    L.rp_batch_detect_bank_sets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, C.c_int, C.POINTER(_DetectorConfig), vp, vp, vp,
                                            C.c_int, vp, vp, C.c_size_t]
    L.rp_stream_batch_new_bank_sets.argtypes = [vp, vp, vp, C.c_int, C.POINTER(_DetectorConfig), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_set_wakeword_sets.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.rp_stream_batch_slot_scores.argtypes = [vp, vp, vp]
    L.rp_stream_batch_new_model_bank.argtypes = [vp, vp, vp, C.POINTER(_DetectorConfig), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_set_models.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.rp_stream_batch_logits.argtypes = [vp, vp]
    L.rp_mlp_forward_windows_bank_sets.argtypes = [vp, vp, vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t]
    L.rp_batch_detect_model_bank_sets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, C.c_int, C.POINTER(_DetectorConfig), C.c_int,
                                                  vp, vp, vp, vp, C.c_int]
    L.rp_stream_batch_new_model_bank_sets.argtypes = [vp, vp, vp, C.c_int, C.POINTER(_DetectorConfig), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_set_model_sets.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.rp_model_bank_set_rms_levels.argtypes = [vp, fp]
    L.rp_model_bank_rms_level.argtypes = [vp, C.c_longlong]
    L.rp_model_bank_rms_level.restype = C.c_float
    L.rp_frontend_batch_bank_sets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_FiltersCfg), vp, vp, C.c_int, vp,
                                              C.c_size_t, vp, vp]
    L.rp_frontend_batch_model_bank.argtypes = L.rp_frontend_batch_bank_sets.argtypes
    L.rp_stream_batch_set_filters_per_stream.argtypes = [vp, C.POINTER(_FiltersCfg)]
    L.rp_batch_detect_mixed_sets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, C.c_int, vp, vp, C.c_int,
                                             C.POINTER(_DetectorConfig), C.c_int, vp, vp, vp, vp, C.c_int]
    L.rp_stream_batch_new_mixed_sets.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.POINTER(_DetectorConfig), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.rp_stream_batch_set_mixed_sets.argtypes = [vp, C.c_size_t, C.c_size_t, vp, vp]
    L.rp_frontend_batch_mixed_sets.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(_FiltersCfg), vp, vp, C.c_int, vp, vp,
                                               C.c_int, vp, C.c_size_t, vp, vp]
    _LIB = L
    return L


def _err():
    return RustpotterError(load_library().rp_last_error().decode("utf-8", "replace"))


def sharded_gather_info():
    """How this thread's last batch_detect_sharded[_dev] gathered its results (rp_sharded_gather_info)."""
    return load_library().rp_sharded_gather_info().decode()


def build_info():
    """Architecture and non-default compiler flags of the loaded library (rp_build_info)."""
    return load_library().rp_build_info().decode()


def resampler_frame_lengths(sample_rate):
    """(input frame length per channel, 16 kHz samples it yields) -- AudioEncoder::new, src/audio/encoder.rs:63-83."""
    a, b = C.c_size_t(), C.c_size_t()
    if load_library().rp_resampler_frame_lengths(sample_rate, C.byref(a), C.byref(b)) < 0:
        raise _err()
    return a.value, b.value


def mfcc_num_frames(n_samples):
    return int(load_library().rp_mfcc_num_frames(n_samples))


# ------------------------------------------------------------------ config mirror
class AudioFmt:  # src/config.rs:10-29
    def __init__(self):
        self.sample_rate = 16000
        self.sample_format = SampleFormat.F32
        self.channels = 1
        self.endianness = Endianness.Little


class GainNormalizationConfig:  # src/config.rs:32-52
    def __init__(self):
        self.enabled = False
        self.gain_ref = None
        self.min_gain = 0.1
        self.max_gain = 1.0


class BandPassConfig:  # src/config.rs:55-71
    def __init__(self):
        self.enabled = False
        self.low_cutoff = 80.0
        self.high_cutoff = 400.0


class FiltersConfig:  # src/config.rs:75-82
    def __init__(self):
        self.gain_normalizer = GainNormalizationConfig()
        self.band_pass = BandPassConfig()


class DetectorConfig:  # src/config.rs:172-207
    def __init__(self):
        self.avg_threshold = 0.2
        self.threshold = 0.5
        self.min_scores = 5
        self.eager = False
        self.score_ref = 0.22
        self.band_size = 5
        self.score_mode = ScoreMode.Max
        self.vad_mode = None

    def _c(self):
        c = _DetectorConfig()
        c.avg_threshold, c.threshold, c.min_scores, c.eager = self.avg_threshold, self.threshold, self.min_scores, self.eager
        c.score_ref, c.band_size, c.score_mode = self.score_ref, self.band_size, int(self.score_mode)
        c.vad_mode = int(self.vad_mode) if self.vad_mode is not None else 0
        return c


class RustpotterConfig:  # src/config.rs:212-219
    def __init__(self):
        self.fmt = AudioFmt()
        self.detector = DetectorConfig()
        self.filters = FiltersConfig()

    @staticmethod
    def default():
        return RustpotterConfig()

    def _filters_c(self):
        f = _FiltersCfg()
        g, b = self.filters.gain_normalizer, self.filters.band_pass
        f.gain_normalizer.enabled = g.enabled
        f.gain_normalizer.has_gain_ref = g.gain_ref is not None
        f.gain_normalizer.gain_ref = g.gain_ref if g.gain_ref is not None else 0.0
        f.gain_normalizer.min_gain, f.gain_normalizer.max_gain = g.min_gain, g.max_gain
        f.band_pass.enabled, f.band_pass.low_cutoff, f.band_pass.high_cutoff = b.enabled, b.low_cutoff, b.high_cutoff
        return f

    def _c(self):
        c = _Config()
        c.fmt.sample_rate, c.fmt.sample_format = self.fmt.sample_rate, int(self.fmt.sample_format)
        c.fmt.channels, c.fmt.endianness = self.fmt.channels, int(self.fmt.endianness)
        c.detector = self.detector._c()
        c.filters = self._filters_c()
        return c


class RustpotterDetection:  # src/detector.rs:488-501
    def __init__(self, d):
        import numpy as np
        self.name = d.name.decode()
        self.avg_score = np.float32(d.avg_score)
        self.score = np.float32(d.score)
        self.scores = {d.score_names[i].decode(): np.float32(d.scores[i]) for i in range(d.n_scores)}
        self.counter = int(d.counter)
        self.gain = np.float32(d.gain)

    def __repr__(self):
        return "RustpotterDetection(name=%r, avg_score=%r, score=%r, counter=%d)" % (self.name, float(self.avg_score),
                                                                                      float(self.score), self.counter)


class Rustpotter:
    """src/detector.rs:34-501.  Raises RustpotterError where the reference returns Err(String)."""

    def __init__(self, config):
        self._L = load_library()
        self._h = C.c_void_p()
        c = config._c()
        if self._L.rp_new(C.byref(c), C.byref(self._h)) < 0:
            self._h = None
            raise _err()

    @staticmethod
    def new(config):
        return Rustpotter(config)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rp_free(self._h)
            self._h = None

    def add_wakeword_from_file(self, key, path):
        if self._L.rp_add_wakeword_from_file(self._h, key.encode(), path.encode()) < 0:
            raise _err()

    def add_wakeword_from_buffer(self, key, buffer):
        if self._L.rp_add_wakeword_from_buffer(self._h, key.encode(), bytes(buffer), len(buffer)) < 0:
            raise _err()

    def remove_wakeword(self, key):
        return bool(self._L.rp_remove_wakeword(self._h, key.encode()))

    def remove_wakewords(self):
        return bool(self._L.rp_remove_wakewords(self._h))

    def get_samples_per_frame(self):
        return int(self._L.rp_get_samples_per_frame(self._h))

    def get_bytes_per_frame(self):
        return int(self._L.rp_get_bytes_per_frame(self._h))

    def get_partial_detection(self):
        d = _Detection()
        return RustpotterDetection(d) if self._L.rp_get_partial_detection(self._h, C.byref(d)) == 1 else None

    def get_rms_level(self):
        return float(self._L.rp_get_rms_level(self._h))

    def get_gain(self):
        return float(self._L.rp_get_gain(self._h))

    def get_rms_level_ref(self):
        return float(self._L.rp_get_rms_level_ref(self._h))

    def _ret(self, r, d):
        if r < 0:
            raise _err()
        return RustpotterDetection(d) if r == 1 else None

    def process_bytes(self, audio_bytes):
        d = _Detection()
        b = bytes(audio_bytes)
        return self._ret(self._L.rp_process_bytes(self._h, b, len(b), C.byref(d)), d)

    def process_samples(self, samples):
        """samples: numpy array of int8/int16/int32/float32 (the reference's `Sample` types)."""
        import numpy as np
        a = np.ascontiguousarray(samples)
        fn = {np.dtype(np.int8): self._L.rp_process_samples_i8, np.dtype(np.int16): self._L.rp_process_samples_i16,
              np.dtype(np.int32): self._L.rp_process_samples_i32, np.dtype(np.float32): self._L.rp_process_samples_f32}[a.dtype]
        d = _Detection()
        return self._ret(fn(self._h, a.ctypes.data, a.size, C.byref(d)), d)

    def update_config(self, config):
        c = config._c()
        self._L.rp_update_config(self._h, C.byref(c))

    def update_detector_config(self, config):
        c = config._c()
        self._L.rp_update_detector_config(self._h, C.byref(c))

    def update_filters_config(self, config):
        rc = RustpotterConfig()
        rc.filters = config
        f = rc._filters_c()
        self._L.rp_update_filters_config(self._h, C.byref(f))

    def reset(self):
        self._L.rp_reset(self._h)


# ------------------------------------------------------------- batched operators
class Templates:
    """rp_templates: one wakeword reference resident on the device."""

    def __init__(self, ctx, templates, avg=None):
        import numpy as np
        self._L = load_library()
        self.ctx = ctx
        self.T = len(templates)
        self.K = int(np.asarray(templates[0]).shape[1])
        lens = np.array([len(t) for t in templates], np.int32)
        feats = np.concatenate([np.ascontiguousarray(t, np.float32).reshape(-1) for t in templates]).astype(np.float32)
        avg_a = None if avg is None else np.ascontiguousarray(avg, np.float32)
        self._h = C.c_void_p()
        r = self._L.rp_templates_new(ctx._h, self.T, self.K, lens.ctypes.data_as(C.POINTER(C.c_int)),
                                     feats.ctypes.data_as(C.POINTER(C.c_float)), 0 if avg_a is None else avg_a.shape[0],
                                     None if avg_a is None else avg_a.ctypes.data_as(C.POINTER(C.c_float)), C.byref(self._h))
        if r < 0:
            self._h = None
            raise _err()
        self.max_len = int(self._L.rp_templates_max_len(self._h))
        self.has_avg = avg_a is not None

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rp_templates_free(self._h)
            self._h = None


class Model:
    """rp_model: a wakeword model (Linear/ReLU stack) resident on the device."""

    def __init__(self, ctx, weights, biases):
        import numpy as np
        self._L = load_library()
        self.ctx = ctx
        ws = [np.ascontiguousarray(w, np.float32) for w in weights]
        bs = [np.ascontiguousarray(b, np.float32) for b in biases]
        dims = np.array([ws[0].shape[1]] + [w.shape[0] for w in ws], np.int32)
        fp = C.POINTER(C.c_float)
        wp = (fp * len(ws))(*[w.ctypes.data_as(fp) for w in ws])
        bp = (fp * len(bs))(*[b.ctypes.data_as(fp) for b in bs])
        self._h = C.c_void_p()
        if self._L.rp_model_new(ctx._h, len(ws), dims.ctypes.data_as(C.POINTER(C.c_int)), wp, bp, C.byref(self._h)) < 0:
            self._h = None
            raise _err()
        self.n_in, self.n_out = int(dims[0]), int(dims[-1])

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rp_model_free(self._h)
            self._h = None


class ModelBank:
    """rp_model_bank: W wakeword models resident on the device, run per stream through an index (BatchContext.mlp_forward_windows_bank /
    batch_detect_model_bank).  Exactly one of models = [Model, ...] with none_index = [index of each model's "none" label or -1, ...]
    (default: every -1), or rpw = [bytes of a wakeword-model .rpw, ...].  The bank copies what it needs: the Model objects may go.
    models=[] is an empty bank to reserve and fill later (reserve / put / put_rpw / train), also under a live StreamBatch."""

    def __init__(self, ctx, models=None, none_index=None, mfcc_size=16, rpw=None):
        import numpy as np
        if (models is None) == (rpw is None):
            raise RustpotterError("ModelBank takes either models or rpw")
        self._L = load_library()
        self.ctx = ctx
        self._h = C.c_void_p()
        if rpw is not None:
            W = len(rpw)
            bufs = [bytes(b) for b in rpw]
            r = self._L.rp_model_bank_new_from_rpw(ctx._h, W, (C.c_char_p * W)(*bufs), (C.c_size_t * W)(*[len(b) for b in bufs]), C.byref(self._h))
        else:
            W = len(models)
            ni = np.full(W, -1, np.int32) if none_index is None else np.ascontiguousarray(none_index, np.int32)
            assert ni.shape == (W,)
            hs = (C.c_void_p * W)(*[m._h for m in models])
            r = self._L.rp_model_bank_new(ctx._h, W, hs, int(mfcc_size), ni.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self._h))
        if r < 0:
            self._h = None
            raise _err()
        self._refresh()

    def _refresh(self):
        self.W = int(self._L.rp_model_bank_size(self._h))
        self.train_sizes = [int(self._L.rp_model_bank_train_size(self._h, w)) for w in range(self.W)]   # window length of every model
        self.labels = [int(self._L.rp_model_bank_labels(self._h, w)) for w in range(self.W)]
        self.max_train_size = int(self._L.rp_model_bank_train_size(self._h, -1))
        self.label_pitch = int(self._L.rp_model_bank_labels(self._h, -1))

    @property
    def reserved(self):
        """rp_model_bank_reserved: (train size, label count) the bank may ever hold, 0 = not reserved"""
        a, b = C.c_int(), C.c_int()
        if self._L.rp_model_bank_reserved(self._h, C.byref(a), C.byref(b)) < 0:
            raise _err()
        return a.value, b.value

    @property
    def pool_growths(self):
        return int(self._L.rp_model_bank_pool_growths(self._h))

    @property
    def last_put_ms(self):
        """model_bank_put_kernel's time in the last put (0 unless the context times its kernels)"""
        return float(self._L.rp_model_bank_last_put_ms(self._h))

    @property
    def rms_levels(self):
        """rp_model_bank_rms_level of every model: [W] float32, NaN = no level (kept from the .rpw files and by train(); NaN for Model handles)"""
        import numpy as np
        return np.array([self._L.rp_model_bank_rms_level(self._h, w) for w in range(self.W)], np.float32)

    def set_rms_levels(self, rms_levels):
        """rp_model_bank_set_rms_levels: [W] levels (NaN: none), in force from the next call that uses the bank"""
        import numpy as np
        a = np.ascontiguousarray(rms_levels, np.float32)
        if a.shape != (self.W,):
            raise ValueError("rms_levels must be [W]")
        if self._L.rp_model_bank_set_rms_levels(self._h, a.ctypes.data_as(C.POINTER(C.c_float))) < 0:
            raise _err()

    def reserve(self, max_train_size=0, max_labels=0, n_models=0, n_frames=0):
        """rp_model_bank_reserve: the largest window and label count the bank will ever hold (what a live batch over it keeps room for)
        and pool size hints"""
        r = self._L.rp_model_bank_reserve(self._h, max_train_size, max_labels, n_models, n_frames)
        self._refresh()
        if r < 0:
            raise _err()

    def put(self, first, models, none_index=None):
        """rp_model_bank_put: Model objects become the models first .. first + n - 1 -- replaced below W, appended at W"""
        import numpy as np
        n = len(models)
        ni = np.full(n, -1, np.int32) if none_index is None else np.ascontiguousarray(none_index, np.int32)
        assert ni.shape == (n,)
        r = self._L.rp_model_bank_put(self._h, first, n, (C.c_void_p * n)(*[m._h for m in models]), ni.ctypes.data_as(C.POINTER(C.c_int32)))
        self._refresh()
        if r < 0:
            raise _err()

    def put_rpw(self, first, rpw):
        """rp_model_bank_put_from_rpw: wakeword-model .rpw bytes into the slots first .. first + n - 1"""
        n = len(rpw)
        bufs = [bytes(b) for b in rpw]
        r = self._L.rp_model_bank_put_from_rpw(self._h, first, n, (C.c_char_p * n)(*bufs), (C.c_size_t * n)(*[len(b) for b in bufs]))
        self._refresh()
        if r < 0:
            raise _err()

    def train(self, first, models, m_type="tiny", learning_rate=0.027, epochs=10, mfcc_size=16, seeds=None, prev_models=None, want_rpw=True):
        """rp_model_bank_train: models as BatchContext.train_wakeword_models takes them, trained straight into the slots first .. first +
        n - 1.  Returns [(.rpw bytes or None, last loss, test accuracy)]."""
        W = len(models)

        def pack(sets):
            names = [k.encode() for d in sets for k in d]
            bufs = [bytes(v) for d in sets for v in d.values()]
            n = len(names)
            return ((C.c_size_t * W)(*[len(d) for d in sets]), (C.c_char_p * n)(*names), (C.c_char_p * n)(*bufs),
                    (C.c_size_t * n)(*[len(b) for b in bufs]))
        trc, trn, trb, trl = pack([m[0] for m in models])
        tec, ten, teb, tel = pack([m[1] for m in models])
        c_seeds = None if seeds is None else (C.c_uint64 * W)(*seeds)
        prev = prev_lens = None
        if prev_models is not None:
            prev = (C.c_char_p * W)(*[None if p is None else bytes(p) for p in prev_models])
            prev_lens = (C.c_size_t * W)(*[0 if p is None else len(p) for p in prev_models])
        opt = _TrainOptions({"tiny": 0, "small": 1, "medium": 2, "large": 3}[m_type], learning_rate, epochs, 0, mfcc_size, 1)
        out = (C.c_void_p * W)() if want_rpw else None
        out_lens = (C.c_size_t * W)() if want_rpw else None
        loss, acc = (C.c_float * W)(), (C.c_float * W)()
        r = self._L.rp_model_bank_train(self._h, first, W, C.byref(opt), c_seeds, trc, trn, trb, trl, tec, ten, teb, tel, prev, prev_lens,
                                        out, out_lens, loss, acc)
        self._refresh()
        if r < 0:
            raise _err()
        res = []
        for w in range(W):
            res.append((C.string_at(out[w], out_lens[w]) if want_rpw else None, loss[w], acc[w]))
            if want_rpw:
                self._L.rp_buffer_free(out[w])
        return res

    def read_image(self, model):
        """rp_model_bank_read_image: the bank image of one model as the kernels read it (wimg | b1 | wsum | padded tail), bytes"""
        need = C.c_size_t()
        if self._L.rp_model_bank_read_image(self._h, model, None, 0, C.byref(need)) < 0:
            raise _err()
        buf = C.create_string_buffer(max(need.value, 1))
        if self._L.rp_model_bank_read_image(self._h, model, buf, need.value, None) < 0:
            raise _err()
        return buf.raw[:need.value]

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rp_model_bank_free(self._h)
            self._h = None


class WakewordBank:
    """rp_wakeword_bank: W wakeword references resident on the device, scored per stream through an index
    (BatchContext.dtw_scores_bank / batch_detect_bank).  Exactly one of
    wakewords = [(templates, avg or None, threshold or None, avg_threshold or None), ...] with templates a list of [len][K] arrays, or
    rpw = [bytes of a wakeword reference .rpw, ...] (what BatchContext.build_wakeword_refs returns).  mfcc_size: what an empty list of
    wakewords declares (a bank to enrol into later: reserve / put / put_rpw / enrol)."""

    @staticmethod
    def _flat(wakewords):
        """the flat arrays of rp_wakeword_bank_new / _put: (W, K, counts, lens, feats, avg_lens, avg_feats or None, thr, athr)"""
        import numpy as np
        W = len(wakewords)
        nan = float("nan")
        tmpl = [[np.ascontiguousarray(t, np.float32) for t in w[0]] for w in wakewords]
        avgs = [None if w[1] is None else np.ascontiguousarray(w[1], np.float32) for w in wakewords]
        K = tmpl[0][0].shape[1] if W else 1
        counts = np.array([len(t) for t in tmpl], np.int32)
        lens = np.array([t.shape[0] for ww in tmpl for t in ww], np.int32)
        feats = np.ascontiguousarray(np.concatenate([t.reshape(-1) for ww in tmpl for t in ww]) if lens.size else np.zeros(0, np.float32), np.float32)
        avg_lens = np.array([0 if a is None else a.shape[0] for a in avgs], np.int32)
        some = [a.reshape(-1) for a in avgs if a is not None]
        avg_feats = np.ascontiguousarray(np.concatenate(some), np.float32) if some else None
        thr = np.array([nan if w[2] is None else w[2] for w in wakewords], np.float32)
        athr = np.array([nan if w[3] is None else w[3] for w in wakewords], np.float32)
        return W, K, counts, lens, feats, avg_lens, avg_feats, thr, athr

    def __init__(self, ctx, wakewords=None, rpw=None, mfcc_size=None):
        if (wakewords is None) == (rpw is None):
            raise RustpotterError("WakewordBank takes either wakewords or rpw")
        self._L = load_library()
        self.ctx = ctx
        self._h = C.c_void_p()
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        if rpw is not None:
            W = len(rpw)
            bufs = [bytes(b) for b in rpw]
            r = self._L.rp_wakeword_bank_new_from_rpw(ctx._h, W, (C.c_char_p * W)(*bufs), (C.c_size_t * W)(*[len(b) for b in bufs]), C.byref(self._h))
        else:
            W, K, counts, lens, feats, avg_lens, avg_feats, thr, athr = self._flat(wakewords)
            if W == 0 and mfcc_size is not None:
                K = int(mfcc_size)
            r = self._L.rp_wakeword_bank_new(ctx._h, W, K, counts.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), feats.ctypes.data_as(fp),
                                             avg_lens.ctypes.data_as(i32p), None if avg_feats is None else avg_feats.ctypes.data_as(fp),
                                             thr.ctypes.data_as(fp), athr.ctypes.data_as(fp), C.byref(self._h))
        if r < 0:
            self._h = None
            raise _err()
        self._refresh()

    def _refresh(self):
        self.W = int(self._L.rp_wakeword_bank_size(self._h))
        self.max_lens = [int(self._L.rp_wakeword_bank_max_len(self._h, w)) for w in range(self.W)]   # window length of every wakeword
        self.max_len = int(self._L.rp_wakeword_bank_max_len(self._h, -1))

    @property
    def reserved_len(self):
        """rp_wakeword_bank_reserved_len: the longest window the bank may ever hold, 0 = not reserved"""
        return int(self._L.rp_wakeword_bank_reserved_len(self._h))

    @property
    def pool_growths(self):
        return int(self._L.rp_wakeword_bank_pool_growths(self._h))

    def reserve(self, max_len=0, n_wakewords=0, n_rows=0):
        """rp_wakeword_bank_reserve: the longest window the bank will ever hold (what a live batch over it keeps room for) and pool size hints"""
        r = self._L.rp_wakeword_bank_reserve(self._h, max_len, n_wakewords, n_rows)
        self._refresh()
        if r < 0:
            raise _err()

    def put(self, first, wakewords, rms_levels=None):
        """rp_wakeword_bank_put: `wakewords` (as the constructor's) become the wakewords first .. first + n - 1 -- replaced below W, appended at W"""
        import numpy as np
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        n, _, counts, lens, feats, avg_lens, avg_feats, thr, athr = self._flat(wakewords)
        lv = None if rms_levels is None else np.ascontiguousarray(rms_levels, np.float32)
        if lv is not None and lv.shape != (n,):
            raise ValueError("rms_levels must be [n]")
        r = self._L.rp_wakeword_bank_put(self._h, first, n, counts.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), feats.ctypes.data_as(fp),
                                         avg_lens.ctypes.data_as(i32p), None if avg_feats is None else avg_feats.ctypes.data_as(fp),
                                         thr.ctypes.data_as(fp), athr.ctypes.data_as(fp), None if lv is None else lv.ctypes.data_as(fp))
        self._refresh()
        if r < 0:
            raise _err()

    def put_rpw(self, first, rpw):
        """rp_wakeword_bank_put_from_rpw: .rpw bytes into the slots first .. first + n - 1, thresholds and rms_level from each file"""
        n = len(rpw)
        bufs = [bytes(b) for b in rpw]
        r = self._L.rp_wakeword_bank_put_from_rpw(self._h, first, n, (C.c_char_p * n)(*bufs), (C.c_size_t * n)(*[len(b) for b in bufs]))
        self._refresh()
        if r < 0:
            raise _err()

    def enrol(self, first, wakewords, from_files=True, want_rpw=False):
        """rp_wakeword_bank_enrol: wakewords as BatchContext.build_wakeword_refs takes them -- (name, ordered {sample name: wav bytes},
        threshold or None, avg_threshold or None) -- enrolled straight into the slots first .. first + n - 1.  want_rpw: also return the
        .rpw bytes of each (what build_wakeword_refs gives); else None."""
        n = len(wakewords)
        nan = float("nan")
        names = (C.c_char_p * n)(*[w[0].encode() for w in wakewords])
        thr = (C.c_float * n)(*[nan if w[2] is None else w[2] for w in wakewords])
        athr = (C.c_float * n)(*[nan if w[3] is None else w[3] for w in wakewords])
        counts = (C.c_size_t * n)(*[len(w[1]) for w in wakewords])
        snames = [k.encode() for w in wakewords for k in w[1]]
        bufs = [bytes(v) for w in wakewords for v in w[1].values()]
        m = len(snames)
        out = (C.c_void_p * n)() if want_rpw else None
        out_lens = (C.c_size_t * n)() if want_rpw else None
        r = self._L.rp_wakeword_bank_enrol(self._h, first, n, names, thr, athr, counts, (C.c_char_p * m)(*snames), (C.c_char_p * m)(*bufs),
                                           (C.c_size_t * m)(*[len(b) for b in bufs]), 1 if from_files else 0, out, out_lens)
        self._refresh()
        if r < 0:
            raise _err()
        if not want_rpw:
            return None
        res = []
        for w in range(n):
            res.append(C.string_at(out[w], out_lens[w]))
            self._L.rp_buffer_free(out[w])
        return res

    @property
    def rms_levels(self):
        """rp_wakeword_bank_rms_level of every wakeword: [W] float32, NaN = no reference level"""
        import numpy as np
        return np.array([self._L.rp_wakeword_bank_rms_level(self._h, w) for w in range(self.W)], np.float32)

    def set_rms_levels(self, rms_levels):
        """rp_wakeword_bank_set_rms_levels: [W] levels (NaN: none), in force from the next call that uses the bank"""
        import numpy as np
        a = np.ascontiguousarray(rms_levels, np.float32)
        if a.shape != (self.W,):
            raise ValueError("rms_levels must be [W]")
        if self._L.rp_wakeword_bank_set_rms_levels(self._h, a.ctypes.data_as(C.POINTER(C.c_float))) < 0:
            raise _err()

    def n_win(self, n_frames, stream_wakeword):
        """windows each stream of a call has: n_frames - max_len(its wakeword) + 1, 0 without a wakeword"""
        return [max(0, n_frames - self.max_lens[w] + 1) if w >= 0 else 0 for w in stream_wakeword]

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rp_wakeword_bank_free(self._h)
            self._h = None


DET_DTYPE = [("stream", "<i4"), ("frame", "<i4"), ("window", "<i4"), ("counter", "<i4"), ("avg_score", "<f4"), ("score", "<f4")]


class StreamBatch:
    """S live streams fed chunk by chunk (rp_stream_batch_*): the batched form of calling
    Rustpotter::process_samples on S instances sharing one wakeword and config -- or, over a WakewordBank, each holding its own."""

    def __init__(self, ctx, templates, detector_config, S, max_chunks_per_call=1, sample_rate=16000, channels=1, wakewords=None,
                 mfcc_size=None, filters=None, rms_level_ref=float("nan"), bank=None, stream_wakeword=None, bank_filters=None,
                 stream_wakewords=None, set_size=None, model_bank=None, stream_model=None, stream_models=None, per_stream_filters=None,
                 model_set_size=None):
        """templates: one wakeword reference (rp_stream_batch_new).  wakewords (rp_stream_batch_new_multi): a list of
        dicts, each {"templates": Templates} or {"model": Model, "none_index": int, "precision": "f32" | "bf16"}, optionally
        with "threshold" / "avg_threshold" (the wakeword's own overrides); mfcc_size is then required.
        filters (rp_stream_batch_set_filters): a FiltersConfig for the streams, with rms_level_ref the largest rms_level of the
        wakewords (NaN: none); levels() then reports every chunk's RMS level and gain.
        bank + stream_wakeword (rp_stream_batch_new_bank; templates is then None): stream s holds the one wakeword
        bank[stream_wakeword[s]], -1 = none; stream_wakeword is [S] int32 (with device pointers: the address of a device array).
        bank_filters (rp_stream_batch_set_filters_bank, with bank): a FiltersConfig whose gain normaliser works per stream, towards
        the rms_level of the stream's own wakeword over its own window.
        per_stream_filters (rp_stream_batch_set_filters_per_stream, with bank or model_bank, one entry or a set per stream): a FiltersConfig
        whose gain normaliser works per stream, towards the largest rms_level of the entries the stream holds over max(Lmax(s) / 3, 1) levels.
        bank + stream_wakewords (rp_stream_batch_new_bank_sets): stream s holds the SET of wakewords stream_wakewords[s], [S][set_size]
        int32 with -1 = an empty slot (with device pointers: the address of a device array and set_size).
        model_bank + stream_model (rp_stream_batch_new_model_bank; templates is then None): stream s runs its own model
        model_bank[stream_model[s]], -1 = none; set_models() re-targets streams, logits() returns the last call's logits.
        model_bank + stream_models (rp_stream_batch_new_model_bank_sets): stream s holds the SET of models stream_models[s], [S][set_size]
        int32 with -1 = an empty slot (with device pointers: the address of a device array and set_size); set_model_sets() re-targets
        streams, logits() is then [S][set_size][frames][label pitch].
        bank + model_bank (rp_stream_batch_new_mixed_sets): stream s holds the references stream_wakewords[s] of bank AND the models
        stream_models[s] of model_bank on one detector; either may be None (that side is absent).  With device pointers: addresses with
        set_size / model_set_size.  set_mixed_sets() re-targets streams; slot_scores() answers the reference slots, logits() the model slots."""
        self._L = load_library()
        self.set_size = 0
        self.model_set_size = 0
        self.mixed = False
        self.label_pitch = 0
        self.ctx, self.templates, self.S, self.max_chunks = ctx, templates, S, max_chunks_per_call
        h = C.c_void_p()
        c = detector_config._c()
        if model_bank is not None and bank is not None:
            self._keep = (bank, model_bank)   # the batch borrows both banks
            self.label_pitch = model_bank.label_pitch
            self.mixed = True
            ridx, rptr = self._indices(stream_wakewords)
            midx, mptr = self._indices(stream_models)
            self.set_size = int((ridx.shape[1] if ridx is not None else 0) if set_size is None else set_size)
            self.model_set_size = int((midx.shape[1] if midx is not None else 0) if model_set_size is None else model_set_size)
            if self._L.rp_stream_batch_new_mixed_sets(ctx._h, bank._h, rptr if self.set_size else None, self.set_size, model_bank._h,
                                                      mptr if self.model_set_size else None, self.model_set_size, C.byref(c), S, max_chunks_per_call,
                                                      C.byref(h)) < 0:
                raise _err()
        elif model_bank is not None and stream_models is not None:
            self._keep = model_bank   # the batch borrows the bank
            self.label_pitch = model_bank.label_pitch
            idx, ptr = self._indices(stream_models)
            self.set_size = int(idx.shape[1] if set_size is None else set_size)
            if self._L.rp_stream_batch_new_model_bank_sets(ctx._h, model_bank._h, ptr, self.set_size, C.byref(c), S, max_chunks_per_call, C.byref(h)) < 0:
                raise _err()
        elif model_bank is not None:
            self._keep = model_bank   # the batch borrows the bank
            self.label_pitch = model_bank.label_pitch
            idx, ptr = self._indices(stream_model)
            if self._L.rp_stream_batch_new_model_bank(ctx._h, model_bank._h, ptr, C.byref(c), S, max_chunks_per_call, C.byref(h)) < 0:
                raise _err()
        elif bank is not None and stream_wakewords is not None:
            self._keep = bank   # the batch borrows the bank
            idx, ptr = self._indices(stream_wakewords)
            self.set_size = int(idx.shape[1] if set_size is None else set_size)
            if self._L.rp_stream_batch_new_bank_sets(ctx._h, bank._h, ptr, self.set_size, C.byref(c), S, max_chunks_per_call, C.byref(h)) < 0:
                raise _err()
        elif bank is not None:
            self._keep = bank   # the batch borrows the bank
            idx, ptr = self._indices(stream_wakeword)
            if self._L.rp_stream_batch_new_bank(ctx._h, bank._h, ptr, C.byref(c), S, max_chunks_per_call, C.byref(h)) < 0:
                raise _err()
        elif wakewords is None:
            if self._L.rp_stream_batch_new(ctx._h, templates._h, C.byref(c), S, max_chunks_per_call, C.byref(h)) < 0:
                raise _err()
        else:
            specs = (_WakewordSpec * len(wakewords))()
            self._keep = list(wakewords)   # the batch borrows the handles
            for sp, w in zip(specs, wakewords):
                sp.templates = w["templates"]._h if w.get("templates") is not None else None
                sp.model = w["model"]._h if w.get("model") is not None else None
                sp.none_index = w.get("none_index", -1)
                sp.precision = {"f32": 0, "bf16": 1}[w.get("precision", "f32")]
                sp.threshold = float("nan") if w.get("threshold") is None else w["threshold"]
                sp.avg_threshold = float("nan") if w.get("avg_threshold") is None else w["avg_threshold"]
            if self._L.rp_stream_batch_new_multi(ctx._h, len(wakewords), specs, mfcc_size, C.byref(c), S, max_chunks_per_call, C.byref(h)) < 0:
                raise _err()
        self._h = h
        if (sample_rate, channels) != (16000, 1) and self._L.rp_stream_batch_set_input(h, sample_rate, channels) < 0:
            raise _err()
        if filters is not None:
            self.set_filters(filters, rms_level_ref)
        if bank_filters is not None:
            self.set_filters_bank(bank_filters)
        if per_stream_filters is not None:
            self.set_filters_per_stream(per_stream_filters)
        self.samples_per_chunk = self._L.rp_stream_batch_samples_per_chunk(h)
        self._last_chunks = 0
        # MFCC frames a stream gains per input frame: 3 (30 ms frames) or 4 (the 40 ms frames of 11.025 / 22.05 kHz input)
        self.frames_per_chunk = resampler_frame_lengths(sample_rate)[1] // 160

    def close(self):
        """rp_stream_batch_free now (a bank counts the batches over it: see WakewordBank.reserve)"""
        if getattr(self, "_h", None):
            self._L.rp_stream_batch_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _indices(self, idx):
        """wakeword indices as the context takes them: a host int32 array, or the address of a device one"""
        import numpy as np
        if idx is None or isinstance(idx, int):
            return None, idx
        a = np.ascontiguousarray(idx, np.int32)
        return a, a.ctypes.data

    def set_wakewords(self, first_stream, stream_wakeword, n=None):
        """rp_stream_batch_set_wakewords: streams first_stream .. get the bank indices stream_wakeword (-1: none) and are reset; between
        process calls.  With device pointers stream_wakeword is the address of a device int32 array of n indices."""
        idx, ptr = self._indices(stream_wakeword)
        if self._L.rp_stream_batch_set_wakewords(self._h, first_stream, len(idx) if n is None else n, ptr) < 0:
            raise _err()

    def set_wakeword_sets(self, first_stream, stream_wakewords, n=None):
        """rp_stream_batch_set_wakeword_sets: streams first_stream .. get the rows stream_wakewords [n][set_size] (-1: an empty slot) and are
        reset -- remove-all plus add-in-order; between process calls.  With device pointers: the address of a device int32 array of n rows."""
        idx, ptr = self._indices(stream_wakewords)
        if self._L.rp_stream_batch_set_wakeword_sets(self._h, first_stream, len(idx) if n is None else n, ptr) < 0:
            raise _err()

    def set_models(self, first_stream, stream_model, n=None):
        """rp_stream_batch_set_models (a batch over a ModelBank): streams first_stream .. get the model indices stream_model (-1: none) and are
        reset; between process calls.  With device pointers stream_model is the address of a device int32 array of n indices."""
        idx, ptr = self._indices(stream_model)
        if self._L.rp_stream_batch_set_models(self._h, first_stream, len(idx) if n is None else n, ptr) < 0:
            raise _err()

    def set_model_sets(self, first_stream, stream_models, n=None):
        """rp_stream_batch_set_model_sets: streams first_stream .. get the rows stream_models [n][set_size] (-1: an empty slot) and are
        reset -- remove-all plus add-in-order; between process calls.  With device pointers: the address of a device int32 array of n rows."""
        idx, ptr = self._indices(stream_models)
        if self._L.rp_stream_batch_set_model_sets(self._h, first_stream, len(idx) if n is None else n, ptr) < 0:
            raise _err()

    def set_mixed_sets(self, first_stream, stream_wakewords, stream_models, n=None):
        """rp_stream_batch_set_mixed_sets: streams first_stream .. get the rows stream_wakewords [n][set_size] and stream_models
        [n][model_set_size] (-1: an empty slot; None for a side the batch does not have) and are reset -- remove-all plus add-in-order;
        between process calls.  With device pointers: the addresses of device int32 arrays of n rows."""
        ridx, rptr = self._indices(stream_wakewords)
        midx, mptr = self._indices(stream_models)
        if n is None:
            n = len(ridx) if ridx is not None else len(midx)
        if self._L.rp_stream_batch_set_mixed_sets(self._h, first_stream, n, rptr if self.set_size else None, mptr if self.model_set_size else None) < 0:
            raise _err()

    def logits(self):
        """rp_stream_batch_logits -> [S][frames of the last process call][label pitch of the bank]; a batch over model sets:
        [S][set_size][frames][label pitch]; a batch over mixed sets: its model slots, [S][model_set_size][frames][label pitch]"""
        import numpy as np
        assert self.ctx.host
        n = max(self._last_chunks, 1) * self.frames_per_chunk
        slots = self.model_set_size if self.mixed else self.set_size
        out = np.empty((self.S, slots, n, self.label_pitch) if (slots or self.mixed) else (self.S, n, self.label_pitch), np.float32)
        if self._L.rp_stream_batch_logits(self._h, out.ctypes.data) < 0:
            raise _err()
        return out

    def logits_dev(self, logits_ptr):
        if self._L.rp_stream_batch_logits(self._h, logits_ptr) < 0:
            raise _err()

    def slot_scores(self):
        """rp_stream_batch_slot_scores -> (agg, avg), each [S][set_size][frames of the last process call]"""
        import numpy as np
        assert self.ctx.host
        n = max(self._last_chunks, 1) * self.frames_per_chunk
        agg = np.empty((self.S, self.set_size if self.mixed else max(self.set_size, 1), n), np.float32)
        avg = np.empty_like(agg)
        if self._L.rp_stream_batch_slot_scores(self._h, agg.ctypes.data, avg.ctypes.data) < 0:
            raise _err()
        return agg, avg

    def slot_scores_dev(self, agg_ptr, avg_ptr):
        if self._L.rp_stream_batch_slot_scores(self._h, agg_ptr, avg_ptr) < 0:
            raise _err()

    @property
    def chunks_seen(self):
        return self._L.rp_stream_batch_chunks_seen(self._h)

    def set_input(self, sample_rate, channels=1):
        """rp_stream_batch_set_input (before the first process call)"""
        if self._L.rp_stream_batch_set_input(self._h, sample_rate, channels) < 0:
            raise _err()
        self.samples_per_chunk = self._L.rp_stream_batch_samples_per_chunk(self._h)
        self.frames_per_chunk = resampler_frame_lengths(sample_rate)[1] // 160

    def set_filters(self, filters, rms_level_ref=float("nan")):
        """rp_stream_batch_set_filters (before the first process call)"""
        rc = RustpotterConfig()
        rc.filters = filters
        f = rc._filters_c()
        if self._L.rp_stream_batch_set_filters(self._h, C.byref(f), rms_level_ref) < 0:
            raise _err()

    def set_filters_bank(self, filters):
        """rp_stream_batch_set_filters_bank (a batch over a bank, before the first process call)"""
        rc = RustpotterConfig()
        rc.filters = filters
        f = rc._filters_c()
        if self._L.rp_stream_batch_set_filters_bank(self._h, C.byref(f)) < 0:
            raise _err()

    def set_filters_per_stream(self, filters):
        """rp_stream_batch_set_filters_per_stream (a batch over a WakewordBank or a ModelBank, one entry or a set per stream; before the
        first process call)"""
        rc = RustpotterConfig()
        rc.filters = filters
        f = rc._filters_c()
        if self._L.rp_stream_batch_set_filters_per_stream(self._h, C.byref(f)) < 0:
            raise _err()

    def levels(self):
        """rp_stream_batch_levels -> (rms, gains), each [S][n_chunks of the last process call]"""
        import numpy as np
        assert self.ctx.host
        n = max(self._last_chunks, 1)
        rms = np.empty((self.S, n), np.float32)
        gains = np.empty((self.S, n), np.float32)
        if self._L.rp_stream_batch_levels(self._h, rms.ctypes.data, gains.ctypes.data) < 0:
            raise _err()
        return rms, gains

    def process(self, pcm, max_det=4, want_agg=False, n_chunks=None):
        """pcm [S][n_chunks*480] numpy (i8 / i16 / i32 / f32) -> (det, n_det[, agg]) for these chunks.  With n_chunks
        given, rows may be longer than the chunks they carry (row pitch = pcm.shape[1])."""
        import numpy as np
        assert self.ctx.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        S, N = pcm.shape
        spc = self.samples_per_chunk
        if S != self.S or (n_chunks is None and N % spc) or (n_chunks is not None and n_chunks * spc > N):
            raise ValueError("pcm must be [S][n_chunks*samples_per_chunk]")
        nc = N // spc if n_chunks is None else n_chunks
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        n_det = np.zeros(S, np.int32)
        agg = np.empty((S, self.frames_per_chunk * nc), np.float32) if want_agg else None
        if self._L.rp_stream_batch_process(self._h, pcm.ctypes.data, fmt, nc, N, det.ctypes.data, n_det.ctypes.data, max_det,
                                           None if agg is None else agg.ctypes.data) < 0:
            raise _err()
        self._last_chunks = nc
        return (det, n_det, agg) if want_agg else (det, n_det)

    def process_multi(self, pcm, max_det=4, n_chunks=None):
        """rp_stream_batch_process_multi -> (det, det_wakeword, det_label, n_det)"""
        import numpy as np
        assert self.ctx.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        S, N = pcm.shape
        spc = self.samples_per_chunk
        if S != self.S or (n_chunks is None and N % spc) or (n_chunks is not None and n_chunks * spc > N):
            raise ValueError("pcm must be [S][n_chunks*samples_per_chunk]")
        nc = N // spc if n_chunks is None else n_chunks
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dww = np.zeros((S, max_det), np.int32)
        dlab = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        if self._L.rp_stream_batch_process_multi(self._h, pcm.ctypes.data, fmt, nc, N, det.ctypes.data, dww.ctypes.data, dlab.ctypes.data,
                                                 n_det.ctypes.data, max_det) < 0:
            raise _err()
        self._last_chunks = nc
        return det, dww, dlab, n_det

    def process_dev(self, pcm_ptr, fmt, n_chunks, stride, det_ptr, n_det_ptr, max_det, agg_ptr=None):
        if self._L.rp_stream_batch_process(self._h, pcm_ptr, fmt, n_chunks, stride, det_ptr, n_det_ptr, max_det, agg_ptr) < 0:
            raise _err()
        self._last_chunks = n_chunks

    def process_multi_dev(self, pcm_ptr, fmt, n_chunks, stride, det_ptr, det_ww_ptr, det_label_ptr, n_det_ptr, max_det):
        if self._L.rp_stream_batch_process_multi(self._h, pcm_ptr, fmt, n_chunks, stride, det_ptr, det_ww_ptr, det_label_ptr, n_det_ptr, max_det) < 0:
            raise _err()
        self._last_chunks = n_chunks

    def reset(self, stream=-1):
        if self._L.rp_stream_batch_reset(self._h, stream) < 0:
            raise _err()


def batch_detect_sharded(ctxs, templates, pcms, detector_config, max_det=8):
    """rp_batch_detect_sharded with host-pointer contexts: pcms = one [S_g][N] numpy array per shard (same N and dtype)
    -> (det [sum S][max_det], n_det [sum S]) gathered, global stream ids."""
    import numpy as np
    L = load_library()
    n = len(ctxs)
    assert n == len(templates) == len(pcms) and all(c.host for c in ctxs)
    arrs = [np.ascontiguousarray(p) for p in pcms]
    # the C call reads every shard as S_g * N samples of ONE format: refuse shards of another length or sample type
    if any(a.ndim != 2 for a in arrs):
        raise ValueError("batch_detect_sharded: every shard must be a 2-D array [streams][samples]")
    N = arrs[0].shape[1]
    if any(a.shape[1] != N or a.dtype != arrs[0].dtype for a in arrs):
        raise ValueError("batch_detect_sharded: all shards must hold streams of the same length and sample type")
    fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(arrs[0].dtype)
    if fmt is None:
        arrs, fmt = [np.ascontiguousarray(a, np.float32) for a in arrs], 3
    S = (C.c_size_t * n)(*[a.shape[0] for a in arrs])
    total = sum(a.shape[0] for a in arrs)
    det = np.zeros((total, max_det), dtype=DET_DTYPE)
    n_det = np.zeros(total, np.int32)
    c = detector_config._c()
    hc = (C.c_void_p * n)(*[x._h for x in ctxs])
    ht = (C.c_void_p * n)(*[x._h for x in templates])
    hp = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    if L.rp_batch_detect_sharded(hc, ht, n, hp, fmt, S, N, N, C.byref(c), det.ctypes.data, n_det.ctypes.data, max_det) < 0:
        raise _err()
    return det, n_det


def batch_detect_sharded_dev(ctxs, templates, pcm_ptrs, S_list, N, stride, detector_config, det_ptr, n_det_ptr, max_det):
    """Device-pointer form: pcm_ptrs[g] on ctxs[g]'s device, det / n_det gathered on ctxs[0]'s device."""
    L = load_library()
    n = len(ctxs)
    if not (n == len(templates) == len(pcm_ptrs) == len(S_list)):
        raise ValueError("batch_detect_sharded_dev: one context, template set, PCM pointer and stream count per shard")
    if any(x.host for x in ctxs):
        raise ValueError("batch_detect_sharded_dev: the contexts must take device pointers (host_pointers=False)")
    c = detector_config._c()
    hc = (C.c_void_p * n)(*[x._h for x in ctxs])
    ht = (C.c_void_p * n)(*[x._h for x in templates])
    hp = (C.c_void_p * n)(*pcm_ptrs)
    S = (C.c_size_t * n)(*S_list)
    if L.rp_batch_detect_sharded(hc, ht, n, hp, 3, S, N, stride, C.byref(c), det_ptr, n_det_ptr, max_det) < 0:
        raise _err()


MLP_PRECISION = {"f32": 0, "bf16": 1, "f32_strict": 2, "f32_fast": 3}   # RP_MLP_F32 / RP_MLP_BF16 / RP_MLP_F32_STRICT / RP_MLP_F32_FAST


_LIVE_CONTEXTS = weakref.WeakSet()   # every BatchContext alive (arithmetic_all)


class arithmetic_all:
    """Context manager for tests: every live BatchContext runs the calls inside with this arithmetic (rp_ctx_set_arithmetic on each),
    contexts made inside start with it too, and every setting comes back afterwards.  What the RP_DTW_MFMA / RP_DTW_RAGGED environment
    switches of rounds 3-5 did, through the ABI."""

    def __init__(self, arithmetic, ragged_matrix=False):
        self.arithmetic, self.ragged = arithmetic, ragged_matrix

    def __enter__(self):
        self.saved = [(c, c.get_arithmetic()) for c in list(_LIVE_CONTEXTS) if getattr(c, "_h", None)]
        for c, _ in self.saved:
            c.set_arithmetic(self.arithmetic, self.ragged)
        return self

    def __exit__(self, *a):
        for c, old in self.saved:
            if getattr(c, "_h", None):
                c.set_arithmetic(*old)


class BatchContext:
    """rp_ctx.  host_pointers=True: numpy in / numpy out (tests); False: raw device
    pointers (bench.py passes torch tensors' data_ptr())."""

    # RP_ARITH_* (include/rustpotter_hip.h): the arithmetic of the DTW cost's cosine products
    ARITH = {"f32_matrix": 0, "strict_f32": 1, "fast_split": 2}

    def __init__(self, device=0, host_pointers=True, full_scores=False, arithmetic="f32_matrix", ragged_matrix=False):
        """full_scores (RP_CTX_FULL_SCORES): batch_detect compares every window with every sample template even where the
        averaged-template gate would skip them.  arithmetic / ragged_matrix: RP_CTX_ARITH_* / RP_CTX_RAGGED_MATRIX."""
        self._L = load_library()
        self._h = C.c_void_p()
        self.host = host_pointers
        flags = (1 if host_pointers else 0) | (2 if full_scores else 0) | {0: 0, 1: 4, 2: 8}[self.ARITH[arithmetic]] | (16 if ragged_matrix else 0)
        if self._L.rp_ctx_new(device, flags, C.byref(self._h)) < 0:
            self._h = None
            raise _err()
        _LIVE_CONTEXTS.add(self)

    def set_arithmetic(self, arithmetic, ragged_matrix=False):
        """rp_ctx_set_arithmetic: "f32_matrix" (default: three bf16 parts, f32-grade), "strict_f32" (vector FMAs only), "fast_split" (two f16 parts)."""
        if self._L.rp_ctx_set_arithmetic(self._h, self.ARITH[arithmetic], 1 if ragged_matrix else 0) < 0:
            raise _err()

    def get_arithmetic(self):
        """(name, ragged_matrix) of rp_ctx_arithmetic."""
        r = C.c_int(0)
        m = int(self._L.rp_ctx_arithmetic(self._h, C.byref(r)))
        return {v: k for k, v in self.ARITH.items()}[m], bool(r.value)

    def arithmetic(self, arithmetic, ragged_matrix=False):
        """Context manager: the calls inside run with this arithmetic, the previous setting comes back afterwards."""
        ctx = self

        class _Scope:
            def __enter__(self):
                self.old = ctx.get_arithmetic()
                ctx.set_arithmetic(arithmetic, ragged_matrix)
                return ctx

            def __exit__(self, *a):
                ctx.set_arithmetic(*self.old)
        return _Scope()

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.rp_ctx_free(self._h)
            self._h = None

    def set_stream(self, hip_stream):
        self._L.rp_ctx_set_stream(self._h, C.c_void_p(hip_stream))

    def synchronize(self):
        if self._L.rp_ctx_synchronize(self._h) < 0:
            raise _err()

    def last_mlp_kernel(self):
        """Which kernel(s) the last dense-row wakeword-model forward of this context ran (rp_ctx_last_mlp_kernel)."""
        self._L.rp_ctx_last_mlp_kernel.restype = C.c_char_p
        v = self._L.rp_ctx_last_mlp_kernel(self._h)
        return v.decode() if v else ""

    def dtw_ref_pairs(self):
        """(window, templates) pairs this context's DTW calls rescored with the reference-shaped cosine so far (rp_ctx_dtw_ref_pairs)."""
        v = C.c_uint64(0)
        if self._L.rp_ctx_dtw_ref_pairs(self._h, C.byref(v)) < 0:
            raise _err()
        return int(v.value)

    def last_window_scores(self, S, n_win, T):
        """[S][n_win][T] sample-template scores as the last rp_batch_detect* of this context left them in its workspace
        (rp_ctx_last_window_scores): what a detect-only call computed, an abandoned DTW as 0.  Defined after ungated calls only."""
        import numpy as np
        out = np.empty((S, n_win, T), np.float32)
        if self._L.rp_ctx_last_window_scores(self._h, out.ctypes.data, out.size) < 0:
            raise _err()
        return out

    DTW_KERNELS = {1: "dtw_mfma_kernel", 2: "dtw_mfma_wide_kernel", 4: "dtw_ragged_kernel", 8: "register kernels", 16: "dtw_generic_kernel",
                   32: "dtw_single_kernel", 64: "dtw_ref_kernel (every window)", 128: "dtw_mfma_group_kernel", 4096: "dtw_bank_kernel",
                   8192: "dtw_bank_stream_kernel", 16384: "dtw_set_kernel", 32768: "dtw_set_stream_kernel",
                   65536: "dtw_mixed_stream_kernel"}
    DTW_PRODUCTS = {256: "bf16x3", 512: "f16x2"}
    DTW_MFMA_WAVES = {1024: 8, 2048: 12}

    def dtw_kernels(self):
        """Names of the DTW kernel families this context launched since the last call of this method (rp_ctx_dtw_kernels)."""
        m = int(self._L.rp_ctx_dtw_kernels(self._h))
        self.last_dtw_products = [n for b, n in self.DTW_PRODUCTS.items() if m & b]   # the matrix-core launches' product arithmetic
        self.last_dtw_mfma_waves = [n for b, n in self.DTW_MFMA_WAVES.items() if m & b]   # waves per workgroup of the dtw_mfma_kernel launches
        return [n for b, n in self.DTW_KERNELS.items() if m & b]

    # --- numpy convenience (host_pointers=True)
    def mfcc(self, pcm, K):
        """pcm: float32, or int8/int16/int32 samples decoded on the device like the reference's `Sample` types."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        nf = mfcc_num_frames(N)
        out = np.empty((S, nf, K), np.float32)
        if self._L.rp_mfcc_batch_fmt(self._h, pcm.ctypes.data, fmt, S, N, N, K, out.ctypes.data) < 0:
            raise _err()
        return out

    def build_wakeword_ref(self, name, samples, mfcc_size, threshold=None, avg_threshold=None, from_files=True):
        """WakewordRef::new_from_sample_files / _buffers + save_to_buffer: samples = ordered {name: wav bytes};
        returns the .rpw bytes."""
        names = [k.encode() for k in samples]
        bufs = [bytes(v) for v in samples.values()]
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_bufs = (C.c_char_p * n)(*bufs)
        c_lens = (C.c_size_t * n)(*[len(b) for b in bufs])
        thr = None if threshold is None else C.byref(C.c_float(threshold))
        athr = None if avg_threshold is None else C.byref(C.c_float(avg_threshold))
        out, out_len = C.c_void_p(), C.c_size_t()
        if self._L.rp_wakeword_ref_build(self._h, name.encode(), C.cast(thr, C.POINTER(C.c_float)) if thr else None,
                                         C.cast(athr, C.POINTER(C.c_float)) if athr else None, n, c_names, c_bufs, c_lens,
                                         mfcc_size, 1 if from_files else 0, C.byref(out), C.byref(out_len)) < 0:
            raise _err()
        data = C.string_at(out, out_len.value)
        self._L.rp_buffer_free(out)
        return data

    def average_templates(self, wakewords):
        """MfccAverager::average for many wakewords in one call (rp_mfcc_average_batch): wakewords = list of lists of [len][K]
        arrays, each list in FOLD order (the first template is the origin the others are folded into); returns one
        [len of the first][K] array per wakeword."""
        import numpy as np
        if not wakewords:
            return []
        tmpl = [[np.ascontiguousarray(t, np.float32) for t in ww] for ww in wakewords]
        if any(len(ww) == 0 for ww in tmpl):
            raise RustpotterError("a wakeword needs at least one template")
        K = tmpl[0][0].shape[1]
        if any(t.ndim != 2 or t.shape[1] != K for ww in tmpl for t in ww):
            raise RustpotterError("templates must be [len][K] arrays of one K")
        counts = np.array([len(ww) for ww in tmpl], np.int32)
        lens = np.array([t.shape[0] for ww in tmpl for t in ww], np.int32)
        feats = np.ascontiguousarray(np.concatenate([t for ww in tmpl for t in ww], axis=0))
        out_lens = [ww[0].shape[0] for ww in tmpl]
        avg = np.empty((sum(out_lens), K), np.float32)
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        if self._L.rp_mfcc_average_batch(self._h, len(tmpl), K, counts.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                         feats.ctypes.data_as(fp), avg.ctypes.data_as(fp)) < 0:
            raise _err()
        ends = np.cumsum(out_lens)
        return [avg[e - n:e].copy() for e, n in zip(ends, out_lens)]

    def build_wakeword_refs(self, wakewords, mfcc_size, from_files=True):
        """build_wakeword_ref for many wakewords in one call (rp_wakeword_ref_build_batch): wakewords = list of
        (name, ordered {sample name: wav bytes}, threshold or None, avg_threshold or None); returns the .rpw bytes of each,
        byte for byte what build_wakeword_ref gives.  One wakeword that cannot be built fails the whole call."""
        W = len(wakewords)
        nan = float("nan")
        names = (C.c_char_p * W)(*[w[0].encode() for w in wakewords])
        thr = (C.c_float * W)(*[nan if w[2] is None else w[2] for w in wakewords])
        athr = (C.c_float * W)(*[nan if w[3] is None else w[3] for w in wakewords])
        counts = (C.c_size_t * W)(*[len(w[1]) for w in wakewords])
        snames = [k.encode() for w in wakewords for k in w[1]]
        bufs = [bytes(v) for w in wakewords for v in w[1].values()]
        n = len(snames)
        c_names = (C.c_char_p * n)(*snames)
        c_bufs = (C.c_char_p * n)(*bufs)
        c_lens = (C.c_size_t * n)(*[len(b) for b in bufs])
        out = (C.c_void_p * W)()
        out_lens = (C.c_size_t * W)()
        if self._L.rp_wakeword_ref_build_batch(self._h, W, names, thr, athr, counts, c_names, c_bufs, c_lens, mfcc_size,
                                               1 if from_files else 0, out, out_lens) < 0:
            raise _err()
        res = []
        for w in range(W):
            res.append(C.string_at(out[w], out_lens[w]))
            self._L.rp_buffer_free(out[w])
        return res

    def train_wakeword_model(self, train, test, m_type="medium", learning_rate=0.027, epochs=10, test_epochs=10, mfcc_size=16,
                             seed=1, prev_model=None):
        """WakewordModel::train_from_buffers + save_to_buffer: train / test = ordered {file name: wav bytes}
        (label in [brackets]); returns (.rpw bytes, last loss, test accuracy)."""
        def pack(d):
            names = [k.encode() for k in d]
            bufs = [bytes(v) for v in d.values()]
            n = len(names)
            return n, (C.c_char_p * n)(*names), (C.c_char_p * n)(*bufs), (C.c_size_t * n)(*[len(b) for b in bufs])
        ntr, trn, trb, trl = pack(train)
        nte, ten, teb, tel = pack(test)
        opt = _TrainOptions({"tiny": 0, "small": 1, "medium": 2, "large": 3}[m_type], learning_rate, epochs, test_epochs, mfcc_size, seed)
        out, out_len, loss, acc = C.c_void_p(), C.c_size_t(), C.c_float(), C.c_float()
        if self._L.rp_wakeword_model_train(self._h, C.byref(opt), ntr, trn, trb, trl, nte, ten, teb, tel, prev_model,
                                           0 if prev_model is None else len(prev_model), C.byref(out), C.byref(out_len),
                                           C.byref(loss), C.byref(acc)) < 0:
            raise _err()
        data = C.string_at(out, out_len.value)
        self._L.rp_buffer_free(out)
        return data, loss.value, acc.value

    def train_wakeword_models(self, models, m_type="medium", learning_rate=0.027, epochs=10, mfcc_size=16, seeds=None, prev_models=None):
        """train_wakeword_model for many models in one call (rp_wakeword_model_train_batch): models = list of (train, test), each an
        ordered {file name: wav bytes}; seeds: one per model (None: 1 + index); prev_models: .rpw bytes or None per model (None: none
        at all).  Returns [(.rpw bytes, last loss, test accuracy)], per model what train_wakeword_model gives for its samples, seed and
        previous model.  One model that cannot be trained fails the whole call."""
        W = len(models)

        def pack(sets):
            names = [k.encode() for d in sets for k in d]
            bufs = [bytes(v) for d in sets for v in d.values()]
            n = len(names)
            return ((C.c_size_t * W)(*[len(d) for d in sets]), (C.c_char_p * n)(*names), (C.c_char_p * n)(*bufs),
                    (C.c_size_t * n)(*[len(b) for b in bufs]))
        trc, trn, trb, trl = pack([m[0] for m in models])
        tec, ten, teb, tel = pack([m[1] for m in models])
        c_seeds = None if seeds is None else (C.c_uint64 * W)(*seeds)
        prev = prev_lens = None
        if prev_models is not None:
            prev = (C.c_char_p * W)(*[None if p is None else bytes(p) for p in prev_models])
            prev_lens = (C.c_size_t * W)(*[0 if p is None else len(p) for p in prev_models])
        opt = _TrainOptions({"tiny": 0, "small": 1, "medium": 2, "large": 3}[m_type], learning_rate, epochs, 0, mfcc_size, 1)
        out, out_lens = (C.c_void_p * W)(), (C.c_size_t * W)()
        loss, acc = (C.c_float * W)(), (C.c_float * W)()
        if self._L.rp_wakeword_model_train_batch(self._h, C.byref(opt), W, c_seeds, trc, trn, trb, trl, tec, ten, teb, tel, prev, prev_lens,
                                                 out, out_lens, loss, acc) < 0:
            raise _err()
        res = []
        for w in range(W):
            res.append((C.string_at(out[w], out_lens[w]), loss[w], acc[w]))
            self._L.rp_buffer_free(out[w])
        return res

    def mlp_train_batch(self, dims, x, labels, params, learning_rate, epochs):
        """The epochs alone for many MLPs in one call (rp_mlp_train_batch): per model dims = its layer widths (input first, label count
        last), x [rows][dims[0]], labels [rows] and params = [(weight [out][in], bias [out]) per layer].  Returns (params in the same
        form, [loss of the last epoch per model])."""
        import numpy as np
        W = len(dims)
        i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        n_layers = np.array([len(d) - 1 for d in dims], np.int32)
        cdims = np.zeros((W, 5), np.int32)
        for w, d in enumerate(dims):
            if not 2 <= len(d) <= 5:
                raise RustpotterError("an MLP of 1 to 4 layers is required")
            cdims[w, :len(d)] = d
        xs = [np.ascontiguousarray(a, np.float32).reshape(-1, d[0]) for a, d in zip(x, dims)]
        n_rows = np.array([a.shape[0] for a in xs], np.int32)
        cx = np.ascontiguousarray(np.concatenate([a.ravel() for a in xs])) if W else np.zeros(0, np.float32)
        cl = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).ravel() for l in labels])) if W else np.zeros(0, np.int32)
        if cl.size != int(n_rows.sum()):
            raise RustpotterError("one label per row is required")
        flat = []
        for w, d in enumerate(dims):
            for l, (wt, b) in enumerate(params[w]):
                wt, b = np.asarray(wt, np.float32), np.asarray(b, np.float32)
                if wt.shape != (d[l + 1], d[l]) or b.shape != (d[l + 1],):
                    raise RustpotterError("model %d layer %d: weight [out][in] and bias [out] are required" % (w, l))
                flat += [wt.ravel(), b.ravel()]
            if len(params[w]) != len(d) - 1:
                raise RustpotterError("model %d: one (weight, bias) per layer is required" % w)
        cp = np.ascontiguousarray(np.concatenate(flat)) if W else np.zeros(0, np.float32)
        loss = np.zeros(W, np.float32)
        if self._L.rp_mlp_train_batch(self._h, W, n_layers.ctypes.data_as(i32p), cdims.ctypes.data_as(i32p), n_rows.ctypes.data_as(i32p),
                                      cx.ctypes.data_as(fp), cl.ctypes.data_as(i32p), cp.ctypes.data_as(fp), learning_rate, epochs,
                                      loss.ctypes.data_as(fp)) < 0:
            raise _err()
        out, at = [], 0
        for d in dims:
            layers = []
            for l in range(len(d) - 1):
                nw, nb = d[l] * d[l + 1], d[l + 1]
                layers.append((cp[at:at + nw].reshape(d[l + 1], d[l]).copy(), cp[at + nw:at + nw + nb].copy()))
                at += nw + nb
            out.append(layers)
        return out, loss

    def train_batch_profile(self):
        """(ms of the feature stage, ms of the longest launch -- 0 unless timing is enabled --, launches) of the last batched training"""
        f, m, n = C.c_double(), C.c_double(), C.c_int()
        if self._L.rp_train_batch_last_profile(self._h, C.byref(f), C.byref(m), C.byref(n)) < 0:
            raise _err()
        return f.value, m.value, n.value

    def frontend(self, pcm, filters_config, rms_level_ref, window_size):
        """Decode + gain normaliser + band-pass over whole streams -> (pcm f32, rms, gains)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        out = np.empty((S, N), np.float32)
        rms = np.empty((S, N // 480), np.float32)
        gains = np.empty((S, N // 480), np.float32)
        if self._L.rp_frontend_batch(self._h, pcm.ctypes.data, fmt, S, N, N, C.byref(f), rms_level_ref, window_size,
                                     out.ctypes.data, N, rms.ctypes.data, gains.ctypes.data) < 0:
            raise _err()
        return out, rms, gains

    def frontend_bank(self, pcm, filters_config, bank, stream_wakeword):
        """rp_frontend_batch_bank: frontend() with the gain normaliser of stream s working towards the rms_level of
        bank[stream_wakeword[s]] over that wakeword's window (-1: no wakeword, gain 1) -> (pcm f32, rms, gains)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        idx = np.ascontiguousarray(stream_wakeword, np.int32)
        assert idx.shape == (S,)
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        out = np.empty((S, N), np.float32)
        rms = np.empty((S, N // 480), np.float32)
        gains = np.empty((S, N // 480), np.float32)
        if self._L.rp_frontend_batch_bank(self._h, pcm.ctypes.data, fmt, S, N, N, C.byref(f), bank._h, idx.ctypes.data,
                                          out.ctypes.data, N, rms.ctypes.data, gains.ctypes.data) < 0:
            raise _err()
        return out, rms, gains

    def frontend_bank_dev(self, pcm_ptr, fmt, S, n_samples, pcm_stride, filters_config, bank, idx_ptr, out_ptr, out_stride, rms_ptr, gains_ptr):
        """rp_frontend_batch_bank with device pointers"""
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        if self._L.rp_frontend_batch_bank(self._h, pcm_ptr, fmt, S, n_samples, pcm_stride, C.byref(f), bank._h, idx_ptr, out_ptr, out_stride,
                                          rms_ptr, gains_ptr) < 0:
            raise _err()

    def _frontend_sets(self, fn, pcm, filters_config, bank, indices):
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        idx = np.ascontiguousarray(indices, np.int32)
        if idx.ndim == 1:
            idx = idx[:, None]
        assert idx.ndim == 2 and idx.shape[0] == S
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        out = np.empty((S, N), np.float32)
        rms = np.empty((S, N // 480), np.float32)
        gains = np.empty((S, N // 480), np.float32)
        if fn(self._h, pcm.ctypes.data, fmt, S, N, N, C.byref(f), bank._h, idx.ctypes.data, idx.shape[1], out.ctypes.data, N, rms.ctypes.data,
              gains.ctypes.data) < 0:
            raise _err()
        return out, rms, gains

    def frontend_bank_sets(self, pcm, filters_config, bank, stream_wakewords):
        """rp_frontend_batch_bank_sets: frontend_bank() for wakeword sets, stream_wakewords [S][set_size] (-1: an empty slot).  Stream s works
        towards the largest non-NaN rms_level of its live slots over max(Lmax(s) / 3, 1) chunk levels -> (pcm f32, rms, gains)."""
        return self._frontend_sets(self._L.rp_frontend_batch_bank_sets, pcm, filters_config, bank, stream_wakewords)

    def frontend_model_bank(self, pcm, filters_config, model_bank, stream_models):
        """rp_frontend_batch_model_bank: the same over a ModelBank, stream_models [S] or [S][set_size] (-1: none)."""
        return self._frontend_sets(self._L.rp_frontend_batch_model_bank, pcm, filters_config, model_bank, stream_models)

    @staticmethod
    def _mixed_rows(rows, S):
        """a side's rows of a mixed-set call -> (int32 array or None, pointer or None, set_size); None: the side is absent (set_size 0, NULL)"""
        import numpy as np
        if rows is None:
            return None, None, 0
        idx = np.ascontiguousarray(rows, np.int32)
        assert idx.ndim == 2 and idx.shape[0] == S
        return idx, (idx.ctypes.data if idx.shape[1] else None), idx.shape[1]

    def frontend_batch_mixed_sets(self, pcm, filters_config, bank, stream_wakewords, model_bank, stream_models):
        """rp_frontend_batch_mixed_sets: frontend_bank_sets() for streams that hold references AND models -- stream_wakewords [S][ref_set_size]
        over the WakewordBank, stream_models [S][model_set_size] over the ModelBank (-1: an empty slot; None: the side is absent).  Stream s
        works towards the largest non-NaN rms_level over the live slots of both rows over max(Lmax(s) / 3, 1) chunk levels
        -> (pcm f32, rms, gains)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        _ri, rp, rn = self._mixed_rows(stream_wakewords, S)
        _mi, mp, mn = self._mixed_rows(stream_models, S)
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        out = np.empty((S, N), np.float32)
        rms = np.empty((S, N // 480), np.float32)
        gains = np.empty((S, N // 480), np.float32)
        if self._L.rp_frontend_batch_mixed_sets(self._h, pcm.ctypes.data, fmt, S, N, N, C.byref(f), bank._h, rp, rn, model_bank._h, mp, mn,
                                                out.ctypes.data, N, rms.ctypes.data, gains.ctypes.data) < 0:
            raise _err()
        return out, rms, gains

    def frontend_bank_sets_dev(self, pcm_ptr, fmt, S, n_samples, pcm_stride, filters_config, bank, idx_ptr, set_size, out_ptr, out_stride, rms_ptr,
                               gains_ptr):
        """rp_frontend_batch_bank_sets with device pointers"""
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        if self._L.rp_frontend_batch_bank_sets(self._h, pcm_ptr, fmt, S, n_samples, pcm_stride, C.byref(f), bank._h, idx_ptr, set_size, out_ptr,
                                               out_stride, rms_ptr, gains_ptr) < 0:
            raise _err()

    def frontend_model_bank_dev(self, pcm_ptr, fmt, S, n_samples, pcm_stride, filters_config, model_bank, idx_ptr, set_size, out_ptr, out_stride,
                                rms_ptr, gains_ptr):
        """rp_frontend_batch_model_bank with device pointers"""
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        if self._L.rp_frontend_batch_model_bank(self._h, pcm_ptr, fmt, S, n_samples, pcm_stride, C.byref(f), model_bank._h, idx_ptr, set_size,
                                                out_ptr, out_stride, rms_ptr, gains_ptr) < 0:
            raise _err()

    def dtw_scores(self, mfcc, templates, score_ref=0.22, band_size=5, score_mode=ScoreMode.Max, with_avg=False):
        import numpy as np
        assert self.host
        mfcc = np.ascontiguousarray(mfcc, np.float32)
        if mfcc.ndim == 2:
            mfcc = mfcc[None]
        S, nf, K = mfcc.shape
        assert K == templates.K
        n_win = max(0, nf - templates.max_len + 1)
        scores = np.empty((S, n_win, templates.T), np.float32)
        agg = np.empty((S, n_win), np.float32)
        avg = np.empty((S, n_win), np.float32) if (with_avg and templates.has_avg) else None
        r = self._L.rp_dtw_score_batch(self._h, mfcc.ctypes.data, S, nf, templates._h, score_ref, band_size, int(score_mode),
                                       1 if avg is not None else 0, scores.ctypes.data,
                                       None if avg is None else avg.ctypes.data, agg.ctypes.data)
        if r < 0:
            raise _err()
        return scores, avg, agg

    def detect_scan(self, agg, avg, n_frames, max_len, detector_config, max_det=8, mfcc=None):
        import numpy as np
        assert self.host
        agg = np.ascontiguousarray(agg, np.float32)
        S = agg.shape[0]
        det = np.zeros((S, max_det), dtype=[("stream", "<i4"), ("frame", "<i4"), ("window", "<i4"), ("counter", "<i4"),
                                             ("avg_score", "<f4"), ("score", "<f4")])
        n_det = np.zeros(S, np.int32)
        c = detector_config._c()
        avg_a = None if avg is None else np.ascontiguousarray(avg, np.float32)
        mf = None if mfcc is None else np.ascontiguousarray(mfcc, np.float32)
        r = self._L.rp_detect_scan(self._h, agg.ctypes.data, None if avg_a is None else avg_a.ctypes.data, S, n_frames,
                                   max_len, C.byref(c), 1 if avg_a is not None else 0,
                                   None if mf is None else mf.ctypes.data, 0 if mf is None else mf.shape[-1],
                                   det.ctypes.data, n_det.ctypes.data, max_det)
        if r < 0:
            raise _err()
        return det, n_det

    def batch_detect(self, pcm, templates, detector_config, max_det=8, want_scores=False):
        """Whole path for S streams in one call (numpy in / out)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        nf = mfcc_num_frames(N)
        n_win = max(0, nf - templates.max_len + 1)
        det = np.zeros((S, max_det), dtype=[("stream", "<i4"), ("frame", "<i4"), ("window", "<i4"), ("counter", "<i4"),
                                             ("avg_score", "<f4"), ("score", "<f4")])
        n_det = np.zeros(S, np.int32)
        scores = np.empty((S, n_win, templates.T), np.float32) if want_scores else None
        agg = np.empty((S, n_win), np.float32) if want_scores else None
        c = detector_config._c()
        r = self._L.rp_batch_detect_fmt(self._h, pcm.ctypes.data, fmt, S, N, N, templates._h, C.byref(c), det.ctypes.data,
                                        n_det.ctypes.data, max_det, None if scores is None else scores.ctypes.data,
                                        None if agg is None else agg.ctypes.data)
        if r < 0:
            raise _err()
        return (det, n_det, scores, agg) if want_scores else (det, n_det)

    def dtw_scores_bank(self, mfcc, bank, stream_wakeword, score_ref=0.22, band_size=5, score_mode=ScoreMode.Max, with_avg=False, win_pitch=None):
        """rp_dtw_score_bank: stream s against bank wakeword stream_wakeword[s] (-1: none) -> (avg or None, agg), rows of win_pitch
        floats (default: the largest window count of the call): the stream's windows, zeros behind them."""
        import numpy as np
        assert self.host
        mfcc = np.ascontiguousarray(mfcc, np.float32)
        if mfcc.ndim == 2:
            mfcc = mfcc[None]
        S, nf, _ = mfcc.shape
        idx = np.ascontiguousarray(stream_wakeword, np.int32)
        assert idx.shape == (S,)
        if win_pitch is None:
            win_pitch = max([0] + [max(0, nf - bank.max_lens[w] + 1) for w in idx if 0 <= w < bank.W])
        agg = np.empty((S, win_pitch), np.float32)
        avg = np.empty((S, win_pitch), np.float32) if with_avg else None
        r = self._L.rp_dtw_score_bank(self._h, mfcc.ctypes.data, S, nf, bank._h, idx.ctypes.data, score_ref, band_size, int(score_mode),
                                      1 if with_avg else 0, None if avg is None else avg.ctypes.data, agg.ctypes.data, win_pitch)
        if r < 0:
            raise _err()
        return avg, agg

    def batch_detect_bank(self, pcm, bank, stream_wakeword, detector_config, max_det=8, want_agg=False, win_pitch=None):
        """rp_batch_detect_bank: the whole path with stream s carrying bank wakeword stream_wakeword[s] (-1: none) -> (det, n_det), with
        want_agg also (agg, avg) as rows of win_pitch floats (see dtw_scores_bank)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        nf = mfcc_num_frames(N)
        idx = np.ascontiguousarray(stream_wakeword, np.int32)
        assert idx.shape == (S,)
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        n_det = np.zeros(S, np.int32)
        agg = avg = None
        if want_agg:
            if win_pitch is None:
                win_pitch = max([0] + [max(0, nf - bank.max_lens[w] + 1) for w in idx if 0 <= w < bank.W])
            agg = np.empty((S, win_pitch), np.float32)
            avg = np.empty((S, win_pitch), np.float32)
        c = detector_config._c()
        r = self._L.rp_batch_detect_bank(self._h, pcm.ctypes.data, fmt, S, N, N, bank._h, idx.ctypes.data, C.byref(c), det.ctypes.data,
                                         n_det.ctypes.data, max_det, None if agg is None else agg.ctypes.data,
                                         None if avg is None else avg.ctypes.data, win_pitch or 0)
        if r < 0:
            raise _err()
        return (det, n_det, agg, avg) if want_agg else (det, n_det)

    def batch_detect_bank_dev(self, pcm_ptr, fmt, S, N, stride, bank, idx_ptr, detector_config, det_ptr, n_det_ptr, max_det,
                              agg_ptr=None, avg_ptr=None, win_pitch=0):
        """device pointers; detect-only unless agg_ptr / avg_ptr ([S][win_pitch] floats) are given (tools/bench_bank.py)"""
        c = detector_config._c()
        if self._L.rp_batch_detect_bank(self._h, pcm_ptr, fmt, S, N, stride, bank._h, idx_ptr, C.byref(c), det_ptr, n_det_ptr, max_det,
                                        agg_ptr, avg_ptr, win_pitch) < 0:
            raise _err()

    def dtw_scores_bank_dev(self, mfcc_ptr, S, n_frames, bank, idx_ptr, score_ref, band_size, score_mode, with_avg, avg_ptr, agg_ptr, win_pitch):
        """rp_dtw_score_bank on device pointers: avg_ptr (may be None) and agg_ptr are [S][win_pitch] floats"""
        if self._L.rp_dtw_score_bank(self._h, mfcc_ptr, S, n_frames, bank._h, idx_ptr, score_ref, band_size, int(score_mode),
                                     int(with_avg), avg_ptr, agg_ptr, win_pitch) < 0:
            raise _err()

    @staticmethod
    def _set_pitch(bank, sets, nf):
        """the largest window count of a call over sets: a stream's window is as long as its longest live slot"""
        lmax = [max([0] + [bank.max_lens[w] for w in row if 0 <= w < bank.W]) for row in sets]
        return max([0] + [max(0, nf - l + 1) for l in lmax if l > 0])

    def dtw_scores_bank_sets(self, mfcc, bank, stream_wakewords, score_ref=0.22, band_size=5, score_mode=ScoreMode.Max, with_avg=False, win_pitch=None):
        """rp_dtw_score_bank_sets: stream s against the set of bank wakewords stream_wakewords[s] ([S][set_size], -1: an empty slot) ->
        (avg or None, agg), each [S][set_size][win_pitch] (default: the largest window count of the call): a slot's windows, zeros behind."""
        import numpy as np
        assert self.host
        mfcc = np.ascontiguousarray(mfcc, np.float32)
        if mfcc.ndim == 2:
            mfcc = mfcc[None]
        S, nf, _ = mfcc.shape
        idx = np.ascontiguousarray(stream_wakewords, np.int32)
        assert idx.ndim == 2 and idx.shape[0] == S
        n = idx.shape[1]
        if win_pitch is None:
            win_pitch = self._set_pitch(bank, idx, nf)
        agg = np.empty((S, n, win_pitch), np.float32)
        avg = np.empty((S, n, win_pitch), np.float32) if with_avg else None
        r = self._L.rp_dtw_score_bank_sets(self._h, mfcc.ctypes.data, S, nf, bank._h, idx.ctypes.data, n, score_ref, band_size, int(score_mode),
                                           1 if with_avg else 0, None if avg is None else avg.ctypes.data, agg.ctypes.data, win_pitch)
        if r < 0:
            raise _err()
        return avg, agg

    def batch_detect_bank_sets(self, pcm, bank, stream_wakewords, detector_config, max_det=8, want_agg=False, win_pitch=None):
        """rp_batch_detect_bank_sets: the whole path with stream s carrying the set stream_wakewords[s] -> (det, det_wakeword, n_det), with
        want_agg also (agg, avg), each [S][set_size][win_pitch] (see dtw_scores_bank_sets).  det_wakeword: the winner's bank index."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        nf = mfcc_num_frames(N)
        idx = np.ascontiguousarray(stream_wakewords, np.int32)
        assert idx.ndim == 2 and idx.shape[0] == S
        n = idx.shape[1]
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dww = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        agg = avg = None
        if want_agg:
            if win_pitch is None:
                win_pitch = self._set_pitch(bank, idx, nf)
            agg = np.empty((S, n, win_pitch), np.float32)
            avg = np.empty((S, n, win_pitch), np.float32)
        c = detector_config._c()
        r = self._L.rp_batch_detect_bank_sets(self._h, pcm.ctypes.data, fmt, S, N, N, bank._h, idx.ctypes.data, n, C.byref(c), det.ctypes.data,
                                              dww.ctypes.data, n_det.ctypes.data, max_det, None if agg is None else agg.ctypes.data,
                                              None if avg is None else avg.ctypes.data, win_pitch or 0)
        if r < 0:
            raise _err()
        return (det, dww, n_det, agg, avg) if want_agg else (det, dww, n_det)

    def batch_detect_bank_sets_dev(self, pcm_ptr, fmt, S, N, stride, bank, idx_ptr, set_size, detector_config, det_ptr, det_ww_ptr, n_det_ptr, max_det,
                                   agg_ptr=None, avg_ptr=None, win_pitch=0):
        """device pointers; detect-only unless agg_ptr / avg_ptr ([S][set_size][win_pitch] floats) are given (tools/bench_bank_sets.py)"""
        c = detector_config._c()
        if self._L.rp_batch_detect_bank_sets(self._h, pcm_ptr, fmt, S, N, stride, bank._h, idx_ptr, set_size, C.byref(c), det_ptr, det_ww_ptr,
                                             n_det_ptr, max_det, agg_ptr, avg_ptr, win_pitch) < 0:
            raise _err()

    def dtw_scores_bank_sets_dev(self, mfcc_ptr, S, n_frames, bank, idx_ptr, set_size, score_ref, band_size, score_mode, with_avg, avg_ptr, agg_ptr,
                                 win_pitch):
        """rp_dtw_score_bank_sets on device pointers: avg_ptr (may be None) and agg_ptr are [S][set_size][win_pitch] floats"""
        if self._L.rp_dtw_score_bank_sets(self._h, mfcc_ptr, S, n_frames, bank._h, idx_ptr, set_size, score_ref, band_size, int(score_mode),
                                          int(with_avg), avg_ptr, agg_ptr, win_pitch) < 0:
            raise _err()

    def resample(self, pcm, sample_rate, channels=1):
        """pcm [S][n_samples*channels] (i8 / i16 / i32 / f32, interleaved) at sample_rate -> [S][n_out] f32 at 16 kHz."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        n = N // channels
        fi, fo = resampler_frame_lengths(sample_rate)
        n_out = (n // fi) * fo
        out = np.empty((S, n_out), np.float32)
        if self._L.rp_resample_batch(self._h, pcm.ctypes.data, fmt, channels, sample_rate, S, n, N, out.ctypes.data, n_out) < 0:
            raise _err()
        return out

    def resample_dev(self, pcm_ptr, fmt, channels, sample_rate, S, n, stride, out_ptr, out_stride):
        if self._L.rp_resample_batch(self._h, pcm_ptr, fmt, channels, sample_rate, S, n, stride, out_ptr, out_stride) < 0:
            raise _err()

    def batch_detect_multi(self, pcm, templates, detector_config, thresholds=None, avg_thresholds=None, max_det=8):
        """Several wakewords in one detector: templates = [Templates, ...]; thresholds / avg_thresholds = per-wakeword
        overrides (None entries = the config's).  -> (det, det_wakeword, n_det)"""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        n = len(templates)
        hs = (C.c_void_p * n)(*[t._h for t in templates])
        def arr(v):
            if v is None:
                return None
            a = np.array([np.nan if x is None else x for x in v], np.float32)
            return a
        th, ath = arr(thresholds), arr(avg_thresholds)
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dww = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        c = detector_config._c()
        fpt = C.POINTER(C.c_float)
        if self._L.rp_batch_detect_multi(self._h, pcm.ctypes.data, fmt, S, N, N, n, hs, C.byref(c),
                                         None if th is None else th.ctypes.data_as(fpt), None if ath is None else ath.ctypes.data_as(fpt),
                                         det.ctypes.data, dww.ctypes.data, n_det.ctypes.data, max_det) < 0:
            raise _err()
        return det, dww, n_det

    def batch_detect_model(self, pcm, model, mfcc_size, none_index, detector_config, precision="f32", max_det=8):
        """A wakeword model inside the batched detector -> (det, det_label, n_det)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dlab = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        c = detector_config._c()
        if self._L.rp_batch_detect_model(self._h, pcm.ctypes.data, fmt, S, N, N, model._h, mfcc_size, none_index, C.byref(c),
                                         MLP_PRECISION[precision], det.ctypes.data, dlab.ctypes.data, n_det.ctypes.data, max_det) < 0:
            raise _err()
        return det, dlab, n_det

    def batch_detect_dev(self, pcm_ptr, S, N, stride, templates, detector_config, det_ptr, n_det_ptr, max_det,
                         scores_ptr=None, agg_ptr=None):
        c = detector_config._c()
        if self._L.rp_batch_detect(self._h, pcm_ptr, S, N, stride, templates._h, C.byref(c), det_ptr, n_det_ptr, max_det,
                                   scores_ptr, agg_ptr) < 0:
            raise _err()

    def batch_detect_fmt_dev(self, pcm_ptr, fmt, S, N, stride, templates, detector_config, det_ptr, n_det_ptr, max_det,
                             scores_ptr=None, agg_ptr=None):
        """rp_batch_detect_fmt on device pointers: pcm in one of the reference's sample formats (SampleFormat: 1 = i16, 3 = f32)."""
        c = detector_config._c()
        if self._L.rp_batch_detect_fmt(self._h, pcm_ptr, int(fmt), S, N, stride, templates._h, C.byref(c), det_ptr, n_det_ptr, max_det,
                                       scores_ptr, agg_ptr) < 0:
            raise _err()

    def batch_detect_ingest(self, pcm, templates, detector_config, max_det=8, block_streams=0):
        """rp_batch_detect_ingest: pcm = HOST array [S][N] (numpy; page-locked or not) of f32 / i8 / i16 / i32 samples, taken in blocks
        with the copies under the kernels.  Returns (det [S][max_det], n_det [S], seconds)."""
        import numpy as np
        pcm = np.ascontiguousarray(pcm)
        S, N = pcm.shape
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2, np.dtype(np.float32): 3}[pcm.dtype]
        det = np.zeros((S, max_det), dtype=[("stream", "<i4"), ("frame", "<i4"), ("window", "<i4"), ("counter", "<i4"), ("avg_score", "<f4"), ("score", "<f4")])
        n_det = np.zeros((S,), np.int32)
        sec = C.c_double(0.0)
        c = detector_config._c()
        if self._L.rp_batch_detect_ingest(self._h, pcm.ctypes.data, fmt, S, N, N, templates._h, C.byref(c), det.ctypes.data, n_det.ctypes.data, max_det,
                                          block_streams, C.byref(sec)) < 0:
            raise _err()
        return det, n_det, sec.value

    def batch_detect_ingest_ptr(self, pcm_host_ptr, fmt, S, N, stride, templates, detector_config, det_host_ptr, n_det_host_ptr, max_det, block_streams=0):
        """The same on raw HOST pointers (e.g. torch pinned tensors); returns the call's wall seconds."""
        sec = C.c_double(0.0)
        c = detector_config._c()
        if self._L.rp_batch_detect_ingest(self._h, pcm_host_ptr, int(fmt), S, N, stride, templates._h, C.byref(c), det_host_ptr, n_det_host_ptr, max_det,
                                          block_streams, C.byref(sec)) < 0:
            raise _err()
        return sec.value

    def mlp_forward(self, x, model, precision="f32"):
        import numpy as np
        assert self.host
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty((x.shape[0], model.n_out), np.float32)
        if self._L.rp_mlp_forward_batch(self._h, model._h, x.ctypes.data, x.shape[0], MLP_PRECISION[precision],
                                        out.ctypes.data) < 0:
            raise _err()
        return out

    def mlp_forward_windows(self, mfcc, model, precision="f32"):
        """rp_mlp_forward_windows: mfcc [S][n_frames][K] -> logits [S][n_win][labels] of every window of the model's train_size frames."""
        import numpy as np
        assert self.host
        mfcc = np.ascontiguousarray(mfcc, np.float32)
        S, nf, K = mfcc.shape
        L = model.n_in // K
        n_win = max(nf - L + 1, 0)
        out = np.empty((S, n_win, model.n_out), np.float32)
        if self._L.rp_mlp_forward_windows(self._h, model._h, mfcc.ctypes.data, S, nf, K, MLP_PRECISION[precision], out.ctypes.data) < 0:
            raise _err()
        return out

    def model_bank(self, models=None, none_index=None, mfcc_size=16, rpw=None):
        """rp_model_bank_new / _new_from_rpw: a ModelBank on this context"""
        return ModelBank(self, models=models, none_index=none_index, mfcc_size=mfcc_size, rpw=rpw)

    def mlp_forward_windows_bank(self, mfcc, bank, stream_model, precision="f32", win_pitch=None):
        """rp_mlp_forward_windows_bank: mfcc [S][n_frames][16] -> logits [S][win_pitch][bank.label_pitch]; row (s, w) holds the labels of
        stream s's model bank[stream_model[s]] (-1: none) for its own windows, zeros behind both.  win_pitch defaults to the largest window
        count of the call."""
        import numpy as np
        assert self.host
        mfcc = np.ascontiguousarray(mfcc, np.float32)
        S, nf, K = mfcc.shape
        assert K == 16
        idx = np.ascontiguousarray(stream_model, np.int32)
        assert idx.shape == (S,)
        if win_pitch is None:
            win_pitch = max([0] + [max(0, nf - bank.train_sizes[w] + 1) for w in idx if 0 <= w < bank.W])
        out = np.full((S, win_pitch, bank.label_pitch), np.nan, np.float32)
        if self._L.rp_mlp_forward_windows_bank(self._h, bank._h, idx.ctypes.data, mfcc.ctypes.data, S, nf, MLP_PRECISION[precision],
                                               out.ctypes.data, win_pitch) < 0:
            raise _err()
        return out

    def mlp_forward_windows_bank_dev(self, bank, idx_ptr, mfcc_ptr, S, n_frames, precision, out_ptr, win_pitch):
        """rp_mlp_forward_windows_bank on device pointers"""
        if self._L.rp_mlp_forward_windows_bank(self._h, bank._h, idx_ptr, mfcc_ptr, S, n_frames, MLP_PRECISION[precision], out_ptr, win_pitch) < 0:
            raise _err()

    def batch_detect_model_bank(self, pcm, bank, stream_model, detector_config, precision="f32", max_det=8):
        """rp_batch_detect_model_bank: the whole path with stream s run by its own model bank[stream_model[s]] (-1: none)
        -> (det, det_label, n_det)."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        idx = np.ascontiguousarray(stream_model, np.int32)
        assert idx.shape == (S,)
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dlab = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        c = detector_config._c()
        if self._L.rp_batch_detect_model_bank(self._h, pcm.ctypes.data, fmt, S, N, N, bank._h, idx.ctypes.data, C.byref(c),
                                              MLP_PRECISION[precision], det.ctypes.data, dlab.ctypes.data, n_det.ctypes.data, max_det) < 0:
            raise _err()
        return det, dlab, n_det

    def mlp_forward_windows_bank_sets(self, mfcc, bank, stream_models, precision="f32", win_pitch=None):
        """rp_mlp_forward_windows_bank_sets: mfcc [S][n_frames][16] -> logits [S][set_size][win_pitch][bank.label_pitch]; row (s, j, w) holds
        model stream_models[s][j] (-1: an empty slot) on the window that starts at frame w, for w < n_frames - Lmax(s) + 1.  win_pitch
        defaults to the largest window count of the call."""
        import numpy as np
        assert self.host
        mfcc = np.ascontiguousarray(mfcc, np.float32)
        S, nf, K = mfcc.shape
        assert K == 16
        idx = np.ascontiguousarray(stream_models, np.int32)
        assert idx.ndim == 2 and idx.shape[0] == S
        if win_pitch is None:
            lmax = [max([0] + [bank.train_sizes[w] for w in row if 0 <= w < bank.W]) for row in idx]
            win_pitch = max([0] + [max(0, nf - l + 1) for l in lmax if l])
        out = np.full((S, idx.shape[1], win_pitch, bank.label_pitch), np.nan, np.float32)
        if self._L.rp_mlp_forward_windows_bank_sets(self._h, bank._h, idx.ctypes.data, idx.shape[1], mfcc.ctypes.data, S, nf, MLP_PRECISION[precision],
                                                    out.ctypes.data, win_pitch) < 0:
            raise _err()
        return out

    def mlp_forward_windows_bank_sets_dev(self, bank, idx_ptr, set_size, mfcc_ptr, S, n_frames, precision, out_ptr, win_pitch):
        """rp_mlp_forward_windows_bank_sets on device pointers"""
        if self._L.rp_mlp_forward_windows_bank_sets(self._h, bank._h, idx_ptr, set_size, mfcc_ptr, S, n_frames, MLP_PRECISION[precision], out_ptr,
                                                    win_pitch) < 0:
            raise _err()

    def batch_detect_model_bank_sets(self, pcm, bank, stream_models, detector_config, precision="f32", max_det=8):
        """rp_batch_detect_model_bank_sets: the whole path with stream s holding the set of models stream_models[s] ([S][set_size], -1: an
        empty slot) -> (det, det_model, det_label, n_det).  det_model: the winner's bank index."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        idx = np.ascontiguousarray(stream_models, np.int32)
        assert idx.ndim == 2 and idx.shape[0] == S
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dmod = np.zeros((S, max_det), np.int32)
        dlab = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        c = detector_config._c()
        if self._L.rp_batch_detect_model_bank_sets(self._h, pcm.ctypes.data, fmt, S, N, N, bank._h, idx.ctypes.data, idx.shape[1], C.byref(c),
                                                   MLP_PRECISION[precision], det.ctypes.data, dmod.ctypes.data, dlab.ctypes.data, n_det.ctypes.data,
                                                   max_det) < 0:
            raise _err()
        return det, dmod, dlab, n_det

    def batch_detect_model_bank_sets_dev(self, pcm_ptr, fmt, S, N, stride, bank, idx_ptr, set_size, detector_config, precision, det_ptr, model_ptr,
                                         label_ptr, n_det_ptr, max_det):
        """rp_batch_detect_model_bank_sets on device pointers (tools/bench_model_bank_sets.py)"""
        c = detector_config._c()
        if self._L.rp_batch_detect_model_bank_sets(self._h, pcm_ptr, int(fmt), S, N, stride, bank._h, idx_ptr, set_size, C.byref(c),
                                                   MLP_PRECISION[precision], det_ptr, model_ptr, label_ptr, n_det_ptr, max_det) < 0:
            raise _err()

    def batch_detect_mixed_sets(self, pcm, bank, stream_wakewords, model_bank, stream_models, detector_config, precision="f32", max_det=8):
        """rp_batch_detect_mixed_sets: the whole path with stream s holding references AND models on one detector -- stream_wakewords
        [S][ref_set_size] over the WakewordBank, stream_models [S][model_set_size] over the ModelBank (-1: an empty slot; None: the side is
        absent) -> (det, det_wakeword, det_label, n_det).  det_wakeword: the winner's index in its own bank; det_label: its label for a
        model, -1 for a reference."""
        import numpy as np
        assert self.host
        pcm = np.ascontiguousarray(pcm)
        fmt = {np.dtype(np.int8): 0, np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(pcm.dtype)
        if fmt is None:
            pcm, fmt = np.ascontiguousarray(pcm, np.float32), 3
        if pcm.ndim == 1:
            pcm = pcm[None, :]
        S, N = pcm.shape
        _ri, rp, rn = self._mixed_rows(stream_wakewords, S)
        _mi, mp, mn = self._mixed_rows(stream_models, S)
        det = np.zeros((S, max_det), dtype=DET_DTYPE)
        dww = np.zeros((S, max_det), np.int32)
        dlab = np.zeros((S, max_det), np.int32)
        n_det = np.zeros(S, np.int32)
        c = detector_config._c()
        if self._L.rp_batch_detect_mixed_sets(self._h, pcm.ctypes.data, fmt, S, N, N, bank._h, rp, rn, model_bank._h, mp, mn, C.byref(c),
                                              MLP_PRECISION[precision], det.ctypes.data, dww.ctypes.data, dlab.ctypes.data, n_det.ctypes.data,
                                              max_det) < 0:
            raise _err()
        return det, dww, dlab, n_det

    def batch_detect_mixed_sets_dev(self, pcm_ptr, fmt, S, N, stride, bank, ref_ptr, ref_set_size, model_bank, model_ptr, model_set_size,
                                    detector_config, precision, det_ptr, ww_ptr, label_ptr, n_det_ptr, max_det):
        """rp_batch_detect_mixed_sets on device pointers (tools/bench_mixed_sets.py)"""
        c = detector_config._c()
        if self._L.rp_batch_detect_mixed_sets(self._h, pcm_ptr, int(fmt), S, N, stride, bank._h, ref_ptr, ref_set_size, model_bank._h, model_ptr,
                                              model_set_size, C.byref(c), MLP_PRECISION[precision], det_ptr, ww_ptr, label_ptr, n_det_ptr,
                                              max_det) < 0:
            raise _err()

    def batch_detect_model_dev(self, pcm_ptr, fmt, S, N, stride, model, mfcc_size, none_index, detector_config, precision, det_ptr, label_ptr,
                               n_det_ptr, max_det):
        """rp_batch_detect_model on device pointers (tools/bench_model_bank.py)"""
        c = detector_config._c()
        if self._L.rp_batch_detect_model(self._h, pcm_ptr, int(fmt), S, N, stride, model._h, mfcc_size, none_index, C.byref(c),
                                         MLP_PRECISION[precision], det_ptr, label_ptr, n_det_ptr, max_det) < 0:
            raise _err()

    def batch_detect_model_bank_dev(self, pcm_ptr, fmt, S, N, stride, bank, idx_ptr, detector_config, precision, det_ptr, label_ptr, n_det_ptr, max_det):
        """rp_batch_detect_model_bank on device pointers (tools/bench_model_bank.py)"""
        c = detector_config._c()
        if self._L.rp_batch_detect_model_bank(self._h, pcm_ptr, int(fmt), S, N, stride, bank._h, idx_ptr, C.byref(c), MLP_PRECISION[precision],
                                              det_ptr, label_ptr, n_det_ptr, max_det) < 0:
            raise _err()

    def mlp_dev(self, model, x_ptr, B, precision, out_ptr):
        if self._L.rp_mlp_forward_batch(self._h, model._h, x_ptr, B, MLP_PRECISION[precision], out_ptr) < 0:
            raise _err()

    def synth_pcm(self, seed, first_stream, S, N):
        import numpy as np
        assert self.host
        out = np.empty((S, N), np.float32)
        if self._L.rp_synth_pcm_batch(self._h, seed, first_stream, S, N, N, out.ctypes.data) < 0:
            raise _err()
        return out

    # --- raw device-pointer calls (host_pointers=False)
    def mfcc_dev(self, pcm_ptr, S, N, stride, K, out_ptr):
        if self._L.rp_mfcc_batch(self._h, pcm_ptr, S, N, stride, K, out_ptr) < 0:
            raise _err()

    def mfcc_dev_fmt(self, pcm_ptr, fmt, S, N, stride, K, out_ptr):
        """rp_mfcc_batch_fmt with device pointers: rows of fmt samples (SampleFormat), `stride` samples apart"""
        if self._L.rp_mfcc_batch_fmt(self._h, pcm_ptr, int(fmt), S, N, stride, K, out_ptr) < 0:
            raise _err()

    def frontend_dev(self, pcm_ptr, fmt, S, n_samples, pcm_stride, filters_config, rms_level_ref, window_size, out_ptr, out_stride,
                     rms_ptr=None, gains_ptr=None):
        """rp_frontend_batch with device pointers"""
        rc = RustpotterConfig()
        rc.filters = filters_config
        f = rc._filters_c()
        if self._L.rp_frontend_batch(self._h, pcm_ptr, int(fmt), S, n_samples, pcm_stride, C.byref(f), rms_level_ref, window_size, out_ptr,
                                     out_stride, rms_ptr, gains_ptr) < 0:
            raise _err()

    def dtw_dev(self, mfcc_ptr, S, n_frames, templates, score_ref, band_size, score_mode, with_avg, scores_ptr, avg_ptr, agg_ptr):
        if self._L.rp_dtw_score_batch(self._h, mfcc_ptr, S, n_frames, templates._h, score_ref, band_size, int(score_mode),
                                      int(with_avg), scores_ptr, avg_ptr, agg_ptr) < 0:
            raise _err()

    def scan_dev(self, agg_ptr, avg_ptr, S, n_frames, max_len, detector_config, det_ptr, n_det_ptr, max_det):
        c = detector_config._c()
        if self._L.rp_detect_scan(self._h, agg_ptr, avg_ptr, S, n_frames, max_len, C.byref(c), 1 if avg_ptr else 0, None, 0,
                                  det_ptr, n_det_ptr, max_det) < 0:
            raise _err()

    def synth_dev(self, seed, first_stream, S, N, stride, out_ptr):
        if self._L.rp_synth_pcm_batch(self._h, seed, first_stream, S, N, stride, out_ptr) < 0:
            raise _err()

    def timing_enable(self, on=True):
        self._L.rp_ctx_timing_enable(self._h, 1 if on else 0)

    def timing_reset(self):
        self._L.rp_ctx_timing_reset(self._h)

    def timing_read(self, kernel):
        ms, n = C.c_double(), C.c_int()
        self._L.rp_ctx_timing_read(self._h, kernel, C.byref(ms), C.byref(n))
        return ms.value, n.value

"""ctypes binding of crispy_amd/libcrispy_hip.so (the C ABI declared in include/crispy_hip.h).

There is no Python or CPU fallback: if the shared library is missing, or no gfx950 device is
present, the failure is raised to the caller."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRISPY_HIP_LIB: developer override to A/B another build of the same HIP library (tools/ab_variants.sh)
LIB_PATH = os.environ.get("CRISPY_HIP_LIB") or os.path.join(_HERE, "libcrispy_hip.so")

RN_FRAME = 480
ABI_VERSION = 6
RN_WEIGHT_BYTES = 87503
RN_TAPS = 72
RN_DBG_FLOATS = 4304
LAYOUT_TBF = 0
LAYOUT_BTF = 1

# every symbol include/crispy_hip.h declares (checked by tests/test_abi.py)
RN_SYMBOLS = (
    "crispy_last_error", "crispy_version", "crispy_abi_version", "crispy_device_count",
    "crispy_rn_create", "crispy_rn_destroy", "crispy_rn_reset", "crispy_rn_n_streams",
    "crispy_rn_frames_per_launch", "crispy_rn_n_launches",
    "crispy_rn_process", "crispy_rn_process_device", "crispy_rn_process_s16", "crispy_rn_process_s16_device", "crispy_rn_synchronize",
    "crispy_rn_set_timing", "crispy_rn_last_kernel_ms",
    "crispy_rn_debug_capture", "crispy_rn_debug_read", "crispy_rn_stage_tansig_device",
    "crispy_host_register", "crispy_host_unregister",
    "crispy_rn_weights_from_file", "crispy_rn_create_from_file", "crispy_selftest_exception_guard",
    "crispy_rn_adapter_configure", "crispy_rn_adapter_set_volume", "crispy_rn_adapter_produced_rate_hz",
    "crispy_rn_push_out_len", "crispy_rn_push_device", "crispy_rn_push", "crispy_rn_last_push_ms",
    "crispy_linear_resampler_count",
    "crispy_rn_playback_configure", "crispy_rn_playback_buffered", "crispy_rn_pull_device", "crispy_rn_pull",
    "crispy_rn_record_configure", "crispy_rn_record_app_push_device", "crispy_rn_record_app_push",
    "crispy_rn_level_device", "crispy_rn_level", "crispy_rn_record_buffered", "crispy_rn_record_frames_ready",
    "crispy_rn_record_drain_device", "crispy_rn_record_drain", "crispy_record_worker_plan",
    "crispy_rn_bypass_configure", "crispy_rn_capture_out_len", "crispy_rn_capture_device", "crispy_rn_capture",
    "crispy_rn_record_app_push_at_device", "crispy_rn_record_app_push_at",
    "crispy_rn_model_configure", "crispy_rn_model", "crispy_ns_noise_state",
)
REC_FRAME = 1152                          # the recording worker's frame_size (commands/recording.rs:196)
PCM_F32, PCM_I16, PCM_U16 = 0, 1, 2      # CRISPY_PCM_*
NS_RNNOISE, NS_DUMMY, NS_NOISY = 0, 1, 2   # CRISPY_NS_*


MEL_SYMBOLS = ("crispy_mel_create", "crispy_mel_destroy", "crispy_mel_compute",
               "crispy_mel_compute_device", "crispy_mel_compute_long_device", "crispy_mel_window_device",
               "crispy_mel_synchronize", "crispy_mel_stage_log10_device")
ASR_SYMBOLS = ("crispy_asr_create", "crispy_asr_set_tensor", "crispy_asr_finalize", "crispy_asr_free",
               "crispy_asr_hparams_get", "crispy_asr_encode", "crispy_asr_encode_device", "crispy_asr_synchronize",
               "crispy_asr_set_suppress", "crispy_asr_decode_greedy_device", "crispy_asr_transcribe_tokens",
               "crispy_asr_load", "crispy_asr_load_resident", "crispy_asr_memory_info", "crispy_asr_token_text", "crispy_asr_transcribe", "crispy_asr_free_result",
               "crispy_asr_decode_greedy_lang_device", "crispy_asr_detect_language_device",
               "crispy_asr_transcribe_batch", "crispy_asr_decode_timestamps_device", "crispy_asr_set_precision",
               "crispy_asr_vocab_specials", "crispy_asr_stage_logits_device", "crispy_asr_language_token",
               "crispy_asr_decode_window_device", "crispy_asr_transcribe_recording", "crispy_asr_transcribe_hooks",
               "crispy_asr_align_device", "crispy_asr_dtw_device",
               "crispy_asr_set_confidence", "crispy_asr_result_token_probs", "crispy_asr_result_word_probs",
               "crispy_asr_result_language_probs", "crispy_asr_detect_language_probs_device", "crispy_asr_token_probs_device",
               "crispy_asr_set_audio_ctx", "crispy_asr_audio_ctx")
RS_SYMBOLS = ("crispy_resampler_create", "crispy_resampler_destroy", "crispy_resampler_out_len",
              "crispy_resampler_process_device", "crispy_resampler_synchronize")
DIAR_SYMBOLS = ("crispy_diar_create", "crispy_diar_destroy", "crispy_diar_cluster", "crispy_diar_cluster_device",
                "crispy_diar_affinity_device", "crispy_diar_laplacian_device", "crispy_diar_eigh_device",
                "crispy_diar_decide_device", "crispy_diar_kmeans_device", "crispy_diar_chunk_plan",
                "crispy_diar_speaker_segments", "crispy_diar_find_speaker",
                "crispy_diar_format_text", "crispy_diar_format_result")
DIAR_FRONT_SYMBOLS = ("crispy_diar_fbank_frames", "crispy_diar_speech_segments", "crispy_diar_fbank_device", "crispy_diar_fbank")
DIAR_SEG_SYMBOLS = ("crispy_diar_seg_frames", "crispy_diar_seg_windows", "crispy_diar_seg_load", "crispy_diar_seg_loaded",
                    "crispy_diar_seg_forward_device", "crispy_diar_seg_scores_device", "crispy_diar_seg_scores")
DIAR_EMB_SYMBOLS = ("crispy_diar_emb_frames", "crispy_diar_emb_tensor_spec", "crispy_diar_emb_load", "crispy_diar_emb_loaded",
                    "crispy_diar_emb_dim", "crispy_diar_emb_forward_device", "crispy_diar_embed_device", "crispy_diar_embed")
PK_SYMBOLS = ("crispy_pk_create", "crispy_pk_destroy", "crispy_pk_frames", "crispy_pk_tensor_spec", "crispy_pk_load", "crispy_pk_loaded",
              "crispy_pk_config_of", "crispy_pk_encode_device", "crispy_pk_encode")
PK_TDT_SYMBOLS = ("crispy_pk_tdt_create", "crispy_pk_tdt_destroy", "crispy_pk_tdt_tensor_spec", "crispy_pk_tdt_load", "crispy_pk_tdt_loaded",
                  "crispy_pk_tdt_config_of", "crispy_pk_tdt_max_steps", "crispy_pk_tdt_decode_device", "crispy_pk_tdt_decode", "crispy_pk_tdt_words")
PK_MEL_SYMBOLS = ("crispy_pk_feature_rows", "crispy_pk_mel_filters", "crispy_pk_set_mel_filters", "crispy_pk_features_device", "crispy_pk_features",
                  "crispy_pk_transcribe_device", "crispy_pk_transcribe")
PK_F16_SYMBOLS = ("crispy_pk_set_precision", "crispy_pk_precision", "crispy_pk_stage_gemm_device")
PK_ATTN_F16_SYMBOLS = ("crispy_pk_set_attention_precision", "crispy_pk_attention_precision", "crispy_pk_stage_attention_device")
ALL_SYMBOLS = (RN_SYMBOLS + MEL_SYMBOLS + ASR_SYMBOLS + RS_SYMBOLS + DIAR_SYMBOLS + DIAR_FRONT_SYMBOLS + DIAR_SEG_SYMBOLS + DIAR_EMB_SYMBOLS
               + PK_SYMBOLS + PK_TDT_SYMBOLS + PK_MEL_SYMBOLS + PK_F16_SYMBOLS + PK_ATTN_F16_SYMBOLS)
PK_GEMM_SCALE, PK_GEMM_SILU, PK_GEMM_RESIDUAL, PK_GEMM_GLU = 0, 1, 2, 3      # include/crispy_hip.h: CRISPY_PK_GEMM_*
PK_F16_TILE_M, PK_F16_TILE_N = 128, 128      # crispy_amd/csrc/pk_gemm_f16.hip
PK_ATTN_KEY_TILE = 32      # include/crispy_hip.h: CRISPY_PK_ATTN_KEY_TILE, the key tile of attention mode 1's soft-max
PK_ATTN_F16_Q = 128        # crispy_amd/csrc/pk_internal.h: kAttnF16Q, the queries of one workgroup of pk_attn_f16.hip
PK_MEL_SPEC, PK_MEL_MAX_BINS, PK_MEL_MAX_TAPS, PK_MEL_MIN_SAMPLES, PK_MEL_TILE_FRAMES = 257, 128, 4096, 320, 32      # crispy_amd/csrc/pk_internal.h
PK_TDT_ROWS, PK_TDT_COLS, PK_TDT_MAX_FRAMES, PK_TDT_GROUP = 16, 64, 5000, 32      # crispy_amd/csrc/pk_internal.h
PK_HEAD_DIM, PK_MAX_ROWS, PK_MAX_CLIPS, PK_ATTN_Q, PK_ATTN_K = 128, 40000, 4096, 32, 32      # crispy_amd/csrc/pk_internal.h
EMB_HEAD, EMB_XVEC, EMB_STATS, EMB_MIN_ROWS, EMB_MAX_ROWS, EMB_TENSORS = 320, 512, 1024, 3, 30000, 815      # crispy_amd/csrc/diar_internal.h
SEG_WINDOW, SEG_MIN_LEN, SEG_FRAMES, SEG_CLASSES = 160000, 991, 589, 7      # crispy_amd/csrc/diar_internal.h
SEG_MAX_SAMPLES, SEG_MAX_WINDOWS = 115200000, 4096
FBANK_BINS, FBANK_WAVE_FRAMES, FBANK_TILE_FRAMES = 80, 8, 32      # crispy_amd/csrc/diar_internal.h
FBANK_MAX_CHUNKS, FBANK_MAX_CHUNK_SAMPLES = 16384, 4800000
DIAR_MAX_N, DIAR_MAX_DIM, DIAR_MAX_BATCH, DIAR_LDS_N = 2048, 1024, 64, 192


class PkConfig(C.Structure):
    """crispy_pk_config"""
    _fields_ = [(k, C.c_int) for k in ("hidden", "layers", "heads", "ffn", "conv_kernel", "mel_bins", "sub_channels",
                                       "attention_bias", "convolution_bias", "scale_input")]


class PkTdtConfig(C.Structure):
    """crispy_pk_tdt_config"""
    _fields_ = [("hidden", C.c_int), ("decoder_hidden", C.c_int), ("decoder_layers", C.c_int), ("vocab", C.c_int), ("blank", C.c_int),
                ("n_durations", C.c_int), ("durations", C.c_int * 8), ("max_symbols_per_step", C.c_int)]


class DiarInfo(C.Structure):
    """crispy_diar_info"""
    _fields_ = [("p_star", C.c_int), ("k", C.c_int), ("ratio", C.c_float), ("gap", C.c_float), ("p_max", C.c_int)]


class AsrSpecials(C.Structure):
    """crispy_asr_specials"""
    _fields_ = [(k, C.c_int) for k in ("eot", "sot", "lang0", "n_lang", "translate", "transcribe", "solm", "prev",
                                       "nosp", "notimestamps", "beg", "multilingual")]


class AsrOpts(C.Structure):
    """crispy_asr_opts"""
    _fields_ = [("language_token", C.c_int), ("translate", C.c_int), ("max_new_tokens", C.c_int),
                ("no_timestamps", C.c_int), ("no_prev_text", C.c_int),
                ("temperature", C.c_float), ("temperature_inc", C.c_float), ("entropy_thold", C.c_float),
                ("logprob_thold", C.c_float), ("no_speech_thold", C.c_float), ("best_of", C.c_int),
                ("suppress_nst", C.c_int), ("initial_prompt", C.POINTER(C.c_int)), ("n_initial_prompt", C.c_int),
                ("carry_context", C.c_int), ("beam_size", C.c_int),
                ("dtw_token_timestamps", C.c_int), ("dtw_heads", C.POINTER(C.c_int)), ("n_dtw_heads", C.c_int)]


class AsrSegment(C.Structure):
    """crispy_asr_segment"""
    _fields_ = [("t0", C.c_float), ("t1", C.c_float), ("text", C.c_char_p)]


class AsrWindow(C.Structure):
    """crispy_asr_window"""
    _fields_ = [("seek", C.c_int), ("seek_advance", C.c_int), ("n_tokens", C.c_int), ("decoder", C.c_int),
                ("failed", C.c_int), ("no_speech", C.c_int), ("temperature", C.c_float), ("no_speech_prob", C.c_float),
                ("avg_logprob", C.c_float), ("entropy", C.c_float)]


class AsrWord(C.Structure):
    """crispy_asr_word"""
    _fields_ = [("t0", C.c_float), ("t1", C.c_float), ("text", C.c_char_p), ("first_token", C.c_int), ("n_tokens", C.c_int)]


class AsrResult(C.Structure):
    """crispy_asr_result"""
    _fields_ = [("text", C.c_char_p), ("tokens", C.POINTER(C.c_int)), ("n_tokens", C.c_int),
                ("language_token", C.c_int), ("n_segments", C.c_int), ("segments", C.POINTER(AsrSegment)),
                ("n_windows", C.c_int), ("windows", C.POINTER(AsrWindow)),
                ("token_t_dtw", C.POINTER(C.c_float)), ("n_words", C.c_int), ("words", C.c_void_p)]


ERR_CANCELLED = -7
ERR_INTERNAL = -8
# crispy_asr_progress_fn: void (*)(size_t samples_done, size_t samples_total, void *user)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_size_t, C.c_size_t, C.c_void_p)


class CrispyError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"crispy_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Load libcrispy_hip.so (built by `__graft_entry__.build()` / `make -C crispy_amd/csrc`)."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH)
    return _lib


def load_variant(name: str) -> C.CDLL:
    """Another build of the same library next to the default one: libcrispy_hip_<name>.so (`make variants`: poison = the
    checker build whose RNNoise kernels fill their LDS with NaNs first).  A separate handle with its own state."""
    return load_library(os.path.join(_HERE, f"libcrispy_hip_{name}.so"))


def load_library(path: str) -> C.CDLL:
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  crispy_amd has no CPU fallback.")
    # PyTorch wheels bundle their own libamdhip64.so.7.  If this library pulled in /opt/rocm's copy
    # first, a later `import torch` would load a second HIP runtime into the process and find no GPU.
    # Loading torch first makes both share one runtime (same SONAME), and torch tensors' device
    # pointers are then directly usable by the *_device entry points.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    f32p = C.POINTER(C.c_float)
    L.crispy_last_error.restype = C.c_char_p
    L.crispy_version.restype = C.c_char_p
    L.crispy_device_count.restype = C.c_int
    L.crispy_abi_version.restype = C.c_int
    if L.crispy_abi_version() != ABI_VERSION:      # include/crispy_hip.h: CRISPY_ABI_VERSION
        raise RuntimeError(f"{path}: ABI version {L.crispy_abi_version()}, this binding was written for {ABI_VERSION}")
    L.crispy_rn_create.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_rn_destroy.argtypes = [C.c_void_p]
    L.crispy_rn_weights_from_file.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    L.crispy_rn_create_from_file.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_selftest_exception_guard.argtypes = [C.c_int]
    L.crispy_asr_vocab_specials.argtypes = [C.c_int, C.c_void_p]
    L.crispy_asr_language_token.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    L.crispy_rn_destroy.restype = None
    L.crispy_rn_reset.argtypes = [C.c_void_p, C.c_int]
    L.crispy_rn_n_streams.argtypes = [C.c_void_p]
    L.crispy_rn_process.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.crispy_rn_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_int, C.c_void_p]
    L.crispy_rn_process_s16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.crispy_rn_process_s16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.crispy_rn_synchronize.argtypes = [C.c_void_p]
    L.crispy_host_register.argtypes = [C.c_void_p, C.c_size_t]
    L.crispy_host_unregister.argtypes = [C.c_void_p]
    L.crispy_rn_set_timing.argtypes = [C.c_void_p, C.c_int]
    L.crispy_rn_last_kernel_ms.argtypes = [C.c_void_p, f32p, f32p]
    L.crispy_rn_stage_tansig_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.crispy_rn_adapter_configure.argtypes = [C.c_void_p, C.c_float, C.c_float]
    L.crispy_rn_adapter_set_volume.argtypes = [C.c_void_p, C.c_float]
    L.crispy_rn_adapter_produced_rate_hz.argtypes = [C.c_void_p, f32p]
    L.crispy_rn_push_out_len.argtypes = [C.c_void_p, C.c_long]
    L.crispy_rn_push_out_len.restype = C.c_long
    L.crispy_rn_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long,
                                        C.c_void_p, C.POINTER(C.c_long), C.c_void_p]
    L.crispy_rn_push.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.POINTER(C.c_long)]
    L.crispy_rn_last_push_ms.argtypes = [C.c_void_p, f32p, f32p]
    L.crispy_linear_resampler_count.argtypes = [C.c_float, C.c_float, C.c_long, C.c_long]
    L.crispy_linear_resampler_count.restype = C.c_long
    L.crispy_rn_playback_configure.argtypes = [C.c_void_p, C.c_float]
    L.crispy_rn_playback_buffered.argtypes = [C.c_void_p]
    L.crispy_rn_playback_buffered.restype = C.c_long
    L.crispy_rn_pull_device.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long), C.c_void_p]
    L.crispy_rn_pull.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_long)]
    lp = C.POINTER(C.c_long)
    L.crispy_rn_record_configure.argtypes = [C.c_void_p, C.c_long]
    L.crispy_rn_record_app_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p]
    L.crispy_rn_record_app_push.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int]
    L.crispy_rn_level_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p]
    L.crispy_rn_level.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p]
    L.crispy_rn_record_buffered.argtypes = [C.c_void_p, lp, lp]
    L.crispy_rn_record_frames_ready.argtypes = [C.c_void_p]
    L.crispy_rn_record_frames_ready.restype = C.c_long
    L.crispy_rn_record_drain_device.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, lp, C.c_void_p]
    L.crispy_rn_record_drain.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, lp]
    L.crispy_record_worker_plan.argtypes = [C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_void_p, lp, lp]
    L.crispy_record_worker_plan.restype = C.c_long
    L.crispy_rn_bypass_configure.argtypes = [C.c_void_p, C.c_float]
    L.crispy_rn_capture_out_len.argtypes = [C.c_void_p, C.c_long]
    L.crispy_rn_capture_out_len.restype = C.c_long
    L.crispy_rn_capture_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long,
                                           C.c_void_p, C.c_long, C.c_void_p, lp, C.c_void_p]
    L.crispy_rn_capture.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long,
                                    C.c_void_p, lp]
    L.crispy_rn_record_app_push_at_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p]
    L.crispy_rn_record_app_push_at.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_int]
    L.crispy_rn_model_configure.argtypes = [C.c_void_p, C.c_int]
    L.crispy_rn_model.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.crispy_ns_noise_state.argtypes = [C.c_long, C.c_long, C.c_void_p]
    L.crispy_ns_noise_state.restype = C.c_long
    L.crispy_rn_debug_capture.argtypes = [C.c_void_p, C.c_int]
    L.crispy_rn_debug_read.argtypes = [C.c_void_p, C.c_int, f32p, C.c_size_t]
    L.crispy_mel_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_mel_destroy.argtypes = [C.c_void_p]
    L.crispy_mel_destroy.restype = None
    L.crispy_mel_compute.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    L.crispy_mel_compute_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    L.crispy_mel_synchronize.argtypes = [C.c_void_p]
    L.crispy_mel_stage_log10_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.crispy_asr_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_asr_set_tensor.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]
    L.crispy_asr_finalize.argtypes = [C.c_void_p]
    L.crispy_asr_free.argtypes = [C.c_void_p]
    L.crispy_asr_free.restype = None
    L.crispy_asr_hparams_get.argtypes = [C.c_void_p, C.c_void_p]
    L.crispy_asr_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    L.crispy_asr_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_asr_synchronize.argtypes = [C.c_void_p]
    L.crispy_asr_set_suppress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.crispy_asr_decode_greedy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_asr_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_asr_load_resident.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_asr_memory_info.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.crispy_asr_token_text.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
    L.crispy_asr_transcribe.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]
    L.crispy_asr_transcribe_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_asr_free_result.argtypes = [C.c_void_p]
    L.crispy_asr_transcribe_recording.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                                  PROGRESS_FN, C.c_void_p, C.POINTER(C.c_void_p)]
    L.crispy_asr_transcribe_hooks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, PROGRESS_FN,
                                              C.c_void_p, C.POINTER(C.c_void_p)]
    L.crispy_asr_free_result.restype = None
    L.crispy_asr_set_precision.argtypes = [C.c_void_p, C.c_int]
    L.crispy_asr_stage_logits_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.crispy_asr_decode_timestamps_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                      C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                      C.c_void_p]
    L.crispy_asr_decode_window_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_mel_compute_long_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p]
    L.crispy_mel_window_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_asr_decode_greedy_lang_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_asr_detect_language_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.crispy_asr_transcribe_tokens.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p,
                                               C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_asr_align_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_asr_dtw_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_asr_set_confidence.argtypes = [C.c_void_p, C.c_int]
    L.crispy_asr_result_token_probs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.POINTER(C.c_float)),
                                                C.POINTER(C.c_int)]
    L.crispy_asr_result_word_probs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]
    L.crispy_asr_result_language_probs.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_int)]
    L.crispy_asr_detect_language_probs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_asr_token_probs_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.crispy_asr_set_audio_ctx.argtypes = [C.c_void_p, C.c_int]
    L.crispy_asr_audio_ctx.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.crispy_resampler_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_resampler_destroy.argtypes = [C.c_void_p]
    L.crispy_resampler_destroy.restype = None
    L.crispy_resampler_out_len.argtypes = [C.c_long]
    L.crispy_resampler_out_len.restype = C.c_long
    L.crispy_resampler_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_float,
                                                  C.c_int, C.c_void_p, C.c_long, C.c_void_p]
    L.crispy_resampler_synchronize.argtypes = [C.c_void_p]
    f64p, i32p, szp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_size_t)
    L.crispy_diar_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_diar_destroy.argtypes = [C.c_void_p]
    L.crispy_diar_destroy.restype = None
    L.crispy_diar_cluster.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_diar_cluster_device.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_diar_affinity_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.crispy_diar_laplacian_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.crispy_diar_eigh_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_diar_decide_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.crispy_diar_kmeans_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_diar_chunk_plan.argtypes = [f64p, f64p, lp, C.c_long, C.c_int, f64p, f64p, lp, lp, lp, C.c_long]
    L.crispy_diar_chunk_plan.restype = C.c_long
    L.crispy_diar_speaker_segments.argtypes = [f64p, f64p, i32p, C.c_long, C.c_double, f64p, f64p, i32p, C.c_long]
    L.crispy_diar_speaker_segments.restype = C.c_long
    L.crispy_diar_find_speaker.argtypes = [C.c_double, f64p, f64p, i32p, C.c_long]
    L.crispy_diar_format_text.argtypes = [f64p, f64p, C.POINTER(C.c_char_p), C.c_long, f64p, f64p, i32p, C.c_long,
                                          C.c_char_p, C.c_size_t, szp]
    L.crispy_diar_format_result.argtypes = [C.c_void_p, C.c_double, f64p, f64p, i32p, C.c_long, C.c_char_p, C.c_size_t, szp]
    L.crispy_diar_fbank_frames.argtypes = [C.c_long]
    L.crispy_diar_fbank_frames.restype = C.c_long
    L.crispy_diar_speech_segments.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_long, C.c_int, C.c_double,
                                              f64p, f64p, lp, lp, C.c_long]
    L.crispy_diar_speech_segments.restype = C.c_long
    L.crispy_diar_fbank_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, lp, lp, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                           lp, C.c_void_p]
    L.crispy_diar_fbank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, lp, lp, C.c_int, C.c_float, C.c_void_p, lp]
    L.crispy_diar_seg_frames.argtypes = [C.c_long]
    L.crispy_diar_seg_frames.restype = C.c_long
    L.crispy_diar_seg_windows.argtypes = [C.c_long]
    L.crispy_diar_seg_windows.restype = C.c_long
    L.crispy_diar_seg_load.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), lp, C.c_int]
    L.crispy_diar_seg_loaded.argtypes = [C.c_void_p]
    L.crispy_diar_seg_forward_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_diar_seg_scores_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_void_p]
    L.crispy_diar_seg_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p]
    L.crispy_diar_emb_frames.argtypes = [C.c_long]
    L.crispy_diar_emb_frames.restype = C.c_long
    L.crispy_diar_emb_tensor_spec.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), lp]
    L.crispy_diar_emb_load.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), lp, C.c_int]
    L.crispy_diar_emb_loaded.argtypes = [C.c_void_p]
    L.crispy_diar_emb_dim.argtypes = [C.c_void_p]
    L.crispy_diar_emb_forward_device.argtypes = [C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_diar_embed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, lp, lp, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    L.crispy_diar_embed.argtypes = [C.c_void_p, C.c_void_p, C.c_int, lp, lp, C.c_int, C.c_float, C.c_void_p]
    L.crispy_pk_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_pk_destroy.argtypes = [C.c_void_p]
    L.crispy_pk_destroy.restype = None
    L.crispy_pk_frames.argtypes = [C.c_long]
    L.crispy_pk_frames.restype = C.c_long
    L.crispy_pk_tensor_spec.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), lp]
    L.crispy_pk_load.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), lp, C.c_int]
    L.crispy_pk_loaded.argtypes = [C.c_void_p]
    L.crispy_pk_config_of.argtypes = [C.c_void_p, C.c_void_p]
    L.crispy_pk_encode_device.argtypes = [C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_pk_encode.argtypes = [C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.crispy_pk_set_precision.argtypes = [C.c_void_p, C.c_int]
    L.crispy_pk_precision.argtypes = [C.c_void_p]
    L.crispy_pk_stage_gemm_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                              C.c_void_p, C.c_void_p]
    L.crispy_pk_set_attention_precision.argtypes = [C.c_void_p, C.c_int]
    L.crispy_pk_attention_precision.argtypes = [C.c_void_p]
    L.crispy_pk_stage_attention_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_long), C.c_int,
                                                   C.c_int, C.c_int, C.c_void_p]
    L.crispy_pk_tdt_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.crispy_pk_tdt_destroy.argtypes = [C.c_void_p]
    L.crispy_pk_tdt_destroy.restype = None
    L.crispy_pk_tdt_tensor_spec.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), lp]
    L.crispy_pk_tdt_load.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), lp, C.c_int]
    L.crispy_pk_tdt_loaded.argtypes = [C.c_void_p]
    L.crispy_pk_tdt_config_of.argtypes = [C.c_void_p, C.c_void_p]
    L.crispy_pk_tdt_max_steps.argtypes = [C.c_void_p, C.c_long]
    L.crispy_pk_tdt_max_steps.restype = C.c_long
    L.crispy_pk_tdt_decode_device.argtypes = [C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_pk_tdt_decode.argtypes = [C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_pk_tdt_words.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_long, lp]
    L.crispy_pk_tdt_words.restype = C.c_long
    L.crispy_pk_feature_rows.argtypes = [C.c_long]
    L.crispy_pk_feature_rows.restype = C.c_long
    L.crispy_pk_mel_filters.argtypes = [C.c_int, C.c_void_p]
    L.crispy_pk_set_mel_filters.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.crispy_pk_features_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_pk_features.argtypes = [C.c_void_p, C.c_int, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_pk_transcribe_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.crispy_pk_transcribe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, lp, C.c_int, C.c_void_p, C.c_void_p]
    return L


def check(rc: int, L: "C.CDLL | None" = None) -> None:
    if rc != 0:
        raise CrispyError(rc, (L or lib()).crispy_last_error().decode("utf-8", "replace"))


class Specials(C.Structure):
    """`crispy_asr_specials` (include/crispy_hip.h): special token ids of a whisper.cpp vocabulary of n_vocab entries."""
    _fields_ = [(n, C.c_int) for n in ("eot", "sot", "lang0", "n_lang", "translate", "transcribe", "solm", "prev", "nosp",
                                       "notimestamps", "beg", "multilingual")]


def vocab_specials(n_vocab: int) -> Specials:
    sp = Specials()
    check(lib().crispy_asr_vocab_specials(int(n_vocab), C.byref(sp)))
    return sp

//! Rust side of `libcrispy_hip.so` (C ABI: `include/crispy_hip.h`) for sleep3r/crispy.
//!
//! * the `extern "C"` block declares every entry point of the header, one to one (checked mechanically against
//!   the header by `tests/test_rust_binding_matches_header.py`, because this crate cannot be compiled where the
//!   library is built: no cargo / rustc in that image);
//! * [`DenoiseState`] has the surface of `nnnoiseless::DenoiseState` that crispy uses
//!   (`src-tauri/src/audio.rs:229` `DenoiseState::new()`, `audio.rs:268` `process_frame(&mut out, &in) -> f32`), so
//!   `RnnNoiseProcessor` (`audio.rs:202-315`) swaps one `use` line;
//! * [`GpuWhisperEngine`] has the surface of `transcribe_rs::whisper_cpp::WhisperEngine` behind `SpeechModel`
//!   (`src-tauri/src/managers/transcription.rs:138-141` load, `:183-185` / `:213-215` transcribe).
//!
//! Nothing here panics across the boundary and nothing unwinds out of it: every entry point of the library is a
//! function-try-block that turns C++ exceptions into status codes (the reference builds with `panic = "abort"`,
//! `src-tauri/Cargo.toml:10-20`).
#![allow(non_camel_case_types)]

use std::ffi::{c_char, c_float, c_int, c_long, c_uchar, c_void, CStr, CString};
use std::path::Path;

// ------------------------------------------------------------------------------------------------------------
// raw declarations (include/crispy_hip.h)
// ------------------------------------------------------------------------------------------------------------
pub const CRISPY_OK: c_int = 0;
pub const CRISPY_ERR_INVALID_ARG: c_int = -1;
pub const CRISPY_ERR_NO_DEVICE: c_int = -2;
pub const CRISPY_ERR_HIP: c_int = -3;
pub const CRISPY_ERR_OOM: c_int = -4;
pub const CRISPY_ERR_BAD_MODEL: c_int = -5;
pub const CRISPY_ERR_UNSUPPORTED: c_int = -6;
pub const CRISPY_ERR_CANCELLED: c_int = -7;
pub const CRISPY_ERR_INTERNAL: c_int = -8;
/// Longest clip of one transcribe call: 2 h at 16 kHz (`CRISPY_ASR_MAX_SAMPLES`).
pub const CRISPY_ASR_MAX_SAMPLES: usize = 115_200_000;

pub const CRISPY_RN_FRAME_SIZE: usize = 480;
pub const CRISPY_RN_WEIGHT_BYTES: usize = 87503;
pub const CRISPY_RN_TAPS: usize = 72;
/// The ABI this file was written against (crispy_hip.h: CRISPY_ABI_VERSION); every constructor checks it.
pub const CRISPY_ABI_VERSION: c_int = 6;
pub const CRISPY_MEL_FRAMES: usize = 3000;
pub const CRISPY_MEL_BINS: usize = 201;

/// `crispy_rn_layout`: C enums are `int`-sized on every ABI this library targets.
pub type crispy_rn_layout = c_int;
pub const CRISPY_RN_LAYOUT_TBF: crispy_rn_layout = 0;
pub const CRISPY_RN_LAYOUT_BTF: crispy_rn_layout = 1;
/// Sample formats of `crispy_rn_pull*` (the output callback's conversions, audio.rs:613-650).
pub const CRISPY_PCM_F32: c_int = 0;
pub const CRISPY_PCM_I16: c_int = 1;
pub const CRISPY_PCM_U16: c_int = 2;
/// NsState::RnnNoise / NsState::Legacy(ModelKind::Dummy) / NsState::Legacy(ModelKind::Noisy): crispy_rn_model_configure
pub const CRISPY_NS_RNNOISE: c_int = 0;
pub const CRISPY_NS_DUMMY: c_int = 1;
pub const CRISPY_NS_NOISY: c_int = 2;

#[repr(C)]
pub struct crispy_rn {
    _private: [u8; 0],
}
#[repr(C)]
pub struct crispy_mel {
    _private: [u8; 0],
}
#[repr(C)]
pub struct crispy_asr {
    _private: [u8; 0],
}
#[repr(C)]
pub struct crispy_resampler {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct crispy_asr_hparams {
    pub n_vocab: c_int,
    pub n_audio_ctx: c_int,
    pub n_audio_state: c_int,
    pub n_audio_head: c_int,
    pub n_audio_layer: c_int,
    pub n_text_ctx: c_int,
    pub n_text_state: c_int,
    pub n_text_head: c_int,
    pub n_text_layer: c_int,
    pub n_mels: c_int,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct crispy_asr_specials {
    pub eot: c_int,
    pub sot: c_int,
    pub lang0: c_int,
    pub n_lang: c_int,
    pub translate: c_int,
    pub transcribe: c_int,
    pub solm: c_int,
    pub prev: c_int,
    pub nosp: c_int,
    pub notimestamps: c_int,
    pub beg: c_int,
    pub multilingual: c_int,
}

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct crispy_asr_opts {
    pub language_token: c_int,
    pub translate: c_int,
    pub max_new_tokens: c_int,
    pub no_timestamps: c_int,
    pub no_prev_text: c_int,
    /// whisper_full's decision logic; every field reads "0 = whisper.cpp's default" (include/crispy_hip.h), so
    /// `crispy_asr_opts::default()` is `TranscribeOptions::default()`.
    pub temperature: c_float,
    pub temperature_inc: c_float,
    pub entropy_thold: c_float,
    pub logprob_thold: c_float,
    pub no_speech_thold: c_float,
    pub best_of: c_int,
    /// ABI 3: whisper_full_params.suppress_nst, prompt_tokens / prompt_n_tokens, !no_context, and beam_search.beam_size
    /// (> 1: the BEAM_SEARCH strategy, at most 8 decoders).
    pub suppress_nst: c_int,
    pub initial_prompt: *const c_int,
    pub n_initial_prompt: c_int,
    pub carry_context: c_int,
    pub beam_size: c_int,
    /// ABI 5: word-level timestamps from cross-attention alignment (openai-whisper's word_timestamps, whisper.cpp's
    /// dtw_token_timestamps); `dtw_heads` = (layer, head) pairs, NULL = every head of the last half of the layers.
    pub dtw_token_timestamps: c_int,
    pub dtw_heads: *const c_int,
    pub n_dtw_heads: c_int,
}
impl Default for crispy_asr_opts {
    /// All zero / NULL = `TranscribeOptions::default()` (a raw pointer has no derived Default).
    fn default() -> Self {
        // SAFETY: every field is an integer, a float or a raw pointer: the all-zero bit pattern is a valid value of each.
        unsafe { std::mem::zeroed() }
    }
}

#[repr(C)]
pub struct crispy_asr_segment {
    pub t0: c_float,
    pub t1: c_float,
    pub text: *const c_char,
}

/// What whisper_full decided about one window of the seek loop.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct crispy_asr_window {
    pub seek: c_int,
    pub seek_advance: c_int,
    pub n_tokens: c_int,
    pub decoder: c_int,
    pub failed: c_int,
    pub no_speech: c_int,
    pub temperature: c_float,
    pub no_speech_prob: c_float,
    pub avg_logprob: c_float,
    pub entropy: c_float,
}

#[repr(C)]
pub struct crispy_asr_result {
    pub text: *const c_char,
    pub tokens: *const c_int,
    pub n_tokens: c_int,
    pub language_token: c_int,
    pub n_segments: c_int,
    pub segments: *const crispy_asr_segment,
    pub n_windows: c_int,
    pub windows: *const crispy_asr_window,
    /// ABI 5 (NULL / 0 unless `dtw_token_timestamps`): a start time per token (-1 for timestamp tokens) and the words,
    /// `words` pointing at `n_words` `crispy_asr_word`s.
    pub token_t_dtw: *const c_float,
    pub n_words: c_int,
    pub words: *const c_void,
}

/// One word of a result (`dtw_token_timestamps`): seconds from the start of the chunk, index of its first token.
/// `crispy_diar_info`: what `crispy_diar_cluster*` decided for one recording (`info` is `crispy_diar_info[batch]`).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct crispy_diar_info {
    pub p_star: c_int,
    pub k: c_int,
    pub ratio: c_float,
    pub gap: c_float,
    pub p_max: c_int,
}
/// `crispy_pk_config`: the Parakeet encoder's shape and flags (`cfg` of `crispy_pk_tensor_spec`, `crispy_pk_load`, `crispy_pk_config_of`).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct crispy_pk_config {
    pub hidden: c_int,
    pub layers: c_int,
    pub heads: c_int,
    pub ffn: c_int,
    pub conv_kernel: c_int,
    pub mel_bins: c_int,
    pub sub_channels: c_int,
    pub attention_bias: c_int,
    pub convolution_bias: c_int,
    pub scale_input: c_int,
}
/// `crispy_pk_tdt_config`: the Parakeet TDT decoder's shape (`cfg` of `crispy_pk_tdt_tensor_spec`, `crispy_pk_tdt_load`,
/// `crispy_pk_tdt_config_of`, `crispy_pk_tdt_max_steps`); `durations` holds `n_durations` values.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct crispy_pk_tdt_config {
    pub hidden: c_int,
    pub decoder_hidden: c_int,
    pub decoder_layers: c_int,
    pub vocab: c_int,
    pub blank: c_int,
    pub n_durations: c_int,
    pub durations: [c_int; 8],
    pub max_symbols_per_step: c_int,
}
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct crispy_asr_word {
    pub t0: c_float,
    pub t1: c_float,
    pub text: *const c_char,
    pub first_token: c_int,
    pub n_tokens: c_int,
}

/// `crispy_asr_progress_fn`: called after every group of chunks with (samples done, samples total, user).
pub type crispy_asr_progress_fn = Option<unsafe extern "C" fn(samples_done: usize, samples_total: usize, user: *mut c_void)>;

extern "C" {
    pub fn crispy_last_error() -> *const c_char;
    pub fn crispy_version() -> *const c_char;
    pub fn crispy_abi_version() -> c_int;
    pub fn crispy_device_count() -> c_int;
    pub fn crispy_selftest_exception_guard(kind: c_int) -> c_int;

    pub fn crispy_rn_create(weights: *const i8, nbytes: usize, n_streams: c_int, device: c_int, out: *mut *mut crispy_rn) -> c_int;
    pub fn crispy_rn_destroy(h: *mut crispy_rn);
    pub fn crispy_rn_weights_from_file(path: *const c_char, blob: *mut i8, blob_bytes: usize) -> c_int;
    pub fn crispy_rn_create_from_file(path: *const c_char, n_streams: c_int, device: c_int, out: *mut *mut crispy_rn) -> c_int;
    pub fn crispy_rn_reset(h: *mut crispy_rn, stream: c_int) -> c_int;
    pub fn crispy_rn_n_streams(h: *const crispy_rn) -> c_int;
    pub fn crispy_rn_frames_per_launch() -> c_int;
    pub fn crispy_rn_n_launches(n_frames: c_int) -> c_int;
    pub fn crispy_rn_process(h: *mut crispy_rn, input: *const c_float, output: *mut c_float, vad: *mut c_float, n_frames: c_int, layout: crispy_rn_layout) -> c_int;
    pub fn crispy_host_register(p: *mut c_void, bytes: usize) -> c_int;
    pub fn crispy_host_unregister(p: *mut c_void) -> c_int;
    pub fn crispy_rn_process_device(h: *mut crispy_rn, d_in: *const c_float, d_out: *mut c_float, d_vad: *mut c_float, d_taps: *mut c_float, n_frames: c_int, layout: crispy_rn_layout, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_process_s16(h: *mut crispy_rn, input: *const i16, out: *mut i16, vad: *mut c_float, n_frames: c_int, layout: crispy_rn_layout) -> c_int;
    pub fn crispy_rn_process_s16_device(h: *mut crispy_rn, d_in: *const i16, d_out: *mut i16, d_vad: *mut c_float, n_frames: c_int, layout: crispy_rn_layout, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_adapter_configure(h: *mut crispy_rn, input_rate: c_float, volume: c_float) -> c_int;
    pub fn crispy_rn_adapter_set_volume(h: *mut crispy_rn, volume: c_float) -> c_int;
    pub fn crispy_rn_adapter_produced_rate_hz(h: *const crispy_rn, rate_hz: *mut c_float) -> c_int;
    pub fn crispy_rn_push_out_len(h: *const crispy_rn, n_in: c_long) -> c_long;
    pub fn crispy_rn_push_device(h: *mut crispy_rn, d_in: *const c_float, in_stride: c_long, n_in: c_long, d_out: *mut c_float, out_stride: c_long, d_frames48: *mut c_float, frames_stride: c_long, d_vad: *mut c_float, n_out: *mut c_long, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_push(h: *mut crispy_rn, input: *const c_float, in_stride: c_long, n_in: c_long, out: *mut c_float, out_stride: c_long, vad: *mut c_float, n_out: *mut c_long) -> c_int;
    pub fn crispy_rn_last_push_ms(h: *mut crispy_rn, adapt_in_ms: *mut c_float, adapt_out_ms: *mut c_float) -> c_int;
    pub fn crispy_linear_resampler_count(input_rate: c_float, output_rate: c_float, n_before: c_long, n_in: c_long) -> c_long;
    pub fn crispy_rn_playback_configure(h: *mut crispy_rn, output_rate: c_float) -> c_int;
    pub fn crispy_rn_playback_buffered(h: *const crispy_rn) -> c_long;
    pub fn crispy_rn_pull_device(h: *mut crispy_rn, n_frames: c_long, channels: c_int, format: c_int, d_out: *mut c_void, out_stride: c_long, n_live: *mut c_long, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_pull(h: *mut crispy_rn, n_frames: c_long, channels: c_int, format: c_int, out: *mut c_void, out_stride: c_long, n_live: *mut c_long) -> c_int;
    pub fn crispy_rn_record_configure(h: *mut crispy_rn, ring_samples: c_long) -> c_int;
    pub fn crispy_rn_record_app_push_device(h: *mut crispy_rn, d_in: *const c_float, in_stride: c_long, n_frames: c_long, channels: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_record_app_push(h: *mut crispy_rn, input: *const c_float, in_stride: c_long, n_frames: c_long, channels: c_int) -> c_int;
    pub fn crispy_rn_level_device(h: *mut crispy_rn, d_in: *const c_float, in_stride: c_long, n_in: c_long, d_rms: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_level(h: *mut crispy_rn, input: *const c_float, in_stride: c_long, n_in: c_long, rms: *mut c_float) -> c_int;
    pub fn crispy_rn_record_buffered(h: *const crispy_rn, mic: *mut c_long, app: *mut c_long) -> c_int;
    pub fn crispy_rn_record_frames_ready(h: *const crispy_rn) -> c_long;
    pub fn crispy_rn_record_drain_device(h: *mut crispy_rn, max_frames: c_long, format: c_int, d_out: *mut c_void, out_stride: c_long, n_frames: *mut c_long, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_record_drain(h: *mut crispy_rn, max_frames: c_long, format: c_int, out: *mut c_void, out_stride: c_long, n_frames: *mut c_long) -> c_int;
    pub fn crispy_record_worker_plan(mic_len: c_long, app_len: c_long, max_frames: c_long, mic_off: *mut c_long, app_off: *mut c_long, mic_left: *mut c_long, app_left: *mut c_long) -> c_long;
    pub fn crispy_rn_bypass_configure(h: *mut crispy_rn, raw_input_rate: c_float) -> c_int;
    pub fn crispy_rn_capture_out_len(h: *const crispy_rn, n_frames: c_long) -> c_long;
    pub fn crispy_rn_capture_device(h: *mut crispy_rn, d_in: *const c_void, in_stride: c_long, n_frames: c_long, channels: c_int, format: c_int, d_out: *mut c_float, out_stride: c_long, d_mono: *mut c_float, mono_stride: c_long, d_rms: *mut c_float, n_out: *mut c_long, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_capture(h: *mut crispy_rn, input: *const c_void, in_stride: c_long, n_frames: c_long, channels: c_int, format: c_int, out: *mut c_float, out_stride: c_long, rms: *mut c_float, n_out: *mut c_long) -> c_int;
    pub fn crispy_rn_record_app_push_at_device(h: *mut crispy_rn, d_in: *const c_float, in_stride: c_long, n_frames: c_long, channels: c_int, from_rate: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_record_app_push_at(h: *mut crispy_rn, input: *const c_float, in_stride: c_long, n_frames: c_long, channels: c_int, from_rate: c_int) -> c_int;
    pub fn crispy_rn_model_configure(h: *mut crispy_rn, model: c_int) -> c_int;
    pub fn crispy_rn_model(h: *const crispy_rn, model: *mut c_int) -> c_int;
    pub fn crispy_ns_noise_state(state: c_long, n: c_long, noise: *mut c_float) -> c_long;
    pub fn crispy_rn_synchronize(h: *mut crispy_rn) -> c_int;
    pub fn crispy_rn_set_timing(h: *mut crispy_rn, enable: c_int) -> c_int;
    pub fn crispy_rn_last_kernel_ms(h: *mut crispy_rn, frame_kernel_ms: *mut c_float, total_ms: *mut c_float) -> c_int;
    pub fn crispy_rn_stage_tansig_device(h: *mut crispy_rn, d_x: *const c_float, d_y: *mut c_float, n: usize, sigmoid: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_rn_debug_capture(h: *mut crispy_rn, enable: c_int) -> c_int;
    pub fn crispy_rn_debug_read(h: *mut crispy_rn, stream: c_int, dst: *mut c_float, n_floats: usize) -> c_int;

    pub fn crispy_mel_create(filters: *const c_float, n_mel: c_int, device: c_int, out: *mut *mut crispy_mel) -> c_int;
    pub fn crispy_mel_destroy(h: *mut crispy_mel);
    pub fn crispy_mel_compute(h: *mut crispy_mel, pcm: *const c_float, pcm_stride: c_long, n_samples: *const c_int, batch: c_int, out: *mut c_float) -> c_int;
    pub fn crispy_mel_compute_device(h: *mut crispy_mel, d_pcm: *const c_float, pcm_stride: c_long, n_samples: *const c_int, batch: c_int, d_out: *mut c_float, d_out_t: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_mel_compute_long_device(h: *mut crispy_mel, d_pcm: *const c_float, pcm_stride: c_long, n_samples: *const c_int, batch: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_mel_window_device(h: *mut crispy_mel, clip_idx: *const c_int, seek: *const c_int, n: c_int, d_out: *mut c_float, d_out_t: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_mel_synchronize(h: *mut crispy_mel) -> c_int;
    pub fn crispy_mel_stage_log10_device(h: *mut crispy_mel, d_s: *const f64, d_y: *mut c_float, n: usize, hip_stream: *mut c_void) -> c_int;

    pub fn crispy_asr_create(hp: *const crispy_asr_hparams, mel_filters: *const c_float, device: c_int, out: *mut *mut crispy_asr) -> c_int;
    pub fn crispy_asr_set_tensor(h: *mut crispy_asr, name: *const c_char, data: *const c_float, n_elems: usize) -> c_int;
    pub fn crispy_asr_finalize(h: *mut crispy_asr) -> c_int;
    pub fn crispy_asr_free(h: *mut crispy_asr);
    pub fn crispy_asr_hparams_get(h: *const crispy_asr, out: *mut crispy_asr_hparams) -> c_int;
    pub fn crispy_asr_encode(h: *mut crispy_asr, pcm: *const c_float, pcm_stride: c_long, n_samples: *const c_int, batch: c_int, out: *mut c_float) -> c_int;
    pub fn crispy_asr_encode_device(h: *mut crispy_asr, d_mel_t: *const c_float, batch: c_int, d_out: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_asr_synchronize(h: *mut crispy_asr) -> c_int;
    pub fn crispy_asr_set_precision(h: *mut crispy_asr, mode: c_int) -> c_int;
    pub fn crispy_asr_stage_logits_device(h: *mut crispy_asr, d_x: *const f32, batch: c_int, d_logits: *mut f32) -> c_int;
    pub fn crispy_asr_set_suppress(h: *mut crispy_asr, ids: *const c_int, n: c_int, first_only: c_int) -> c_int;
    pub fn crispy_asr_decode_greedy_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, prompt: *const c_int, n_prompt: c_int, max_new: c_int, tokens_out: *mut c_int, n_out: *mut c_int, logits_out: *mut c_float) -> c_int;
    pub fn crispy_asr_decode_greedy_lang_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, prompt: *const c_int, n_prompt: c_int, lang_tokens: *const c_int, max_new: c_int, tokens_out: *mut c_int, n_out: *mut c_int, logits_out: *mut c_float) -> c_int;
    pub fn crispy_asr_decode_timestamps_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, prompt: *const c_int, n_prompt: c_int, lang_tokens: *const c_int, rules: c_int, seek: *const c_int, seek_end: *const c_int, max_new: c_int, tokens_out: *mut c_int, tids_out: *mut c_int, n_out: *mut c_int) -> c_int;
    pub fn crispy_asr_detect_language_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, lang_tokens_out: *mut c_int) -> c_int;
    pub fn crispy_asr_transcribe_tokens(h: *mut crispy_asr, pcm: *const c_float, pcm_stride: c_long, n_samples: *const c_int, batch: c_int, prompt: *const c_int, n_prompt: c_int, max_new: c_int, tokens_out: *mut c_int, n_out: *mut c_int) -> c_int;
    pub fn crispy_asr_load(model_path: *const c_char, device: c_int, out: *mut *mut crispy_asr) -> c_int;
    pub fn crispy_asr_load_resident(model_path: *const c_char, device: c_int, out: *mut *mut crispy_asr) -> c_int;
    pub fn crispy_asr_memory_info(h: *const crispy_asr, weight_bytes: *mut usize, quantised_bytes: *mut usize, scratch_bytes: *mut usize) -> c_int;
    pub fn crispy_asr_vocab_specials(n_vocab: c_int, out: *mut crispy_asr_specials) -> c_int;
    pub fn crispy_asr_language_token(n_vocab: c_int, code: *const c_char, token_out: *mut c_int) -> c_int;
    pub fn crispy_asr_token_text(h: *const crispy_asr, token: c_int, text: *mut *const c_char, len: *mut usize) -> c_int;
    pub fn crispy_asr_decode_window_device(h: *mut crispy_asr, d_enc: *const c_float, rows: c_int, prompts: *const c_int, n_prompt: *const c_int, prompt_stride: c_int, rules: c_int, seek: *const c_int, seek_end: *const c_int, max_new: c_int, temperature: c_float, u: *const f64, tokens_out: *mut c_int, tids_out: *mut c_int, plog_out: *mut c_float, no_speech_prob_out: *mut c_float, n_out: *mut c_int) -> c_int;
    pub fn crispy_asr_transcribe(h: *mut crispy_asr, pcm16k: *const c_float, n: usize, opts: *const crispy_asr_opts, out: *mut *mut crispy_asr_result) -> c_int;
    pub fn crispy_asr_transcribe_batch(h: *mut crispy_asr, pcm: *const *const c_float, n: *const usize, batch: c_int, opts: *const crispy_asr_opts, results: *mut *mut crispy_asr_result) -> c_int;
    pub fn crispy_asr_free_result(r: *mut crispy_asr_result);
    pub fn crispy_asr_align_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, tokens: *const c_int, n_tokens: *const c_int, ld_tokens: c_int, n_sot: c_int, n_frames: *const c_int, heads: *const c_int, n_heads: c_int, d_probs: *mut c_float, d_matrix: *mut c_float, jump_times: *mut c_float) -> c_int;
    pub fn crispy_asr_dtw_device(h: *mut crispy_asr, d_x: *const c_float, n_rows: c_int, n_cols: c_int, ld: c_long, text_idx: *mut c_int, time_idx: *mut c_int, n_path: *mut c_int) -> c_int;
    pub fn crispy_asr_set_confidence(h: *mut crispy_asr, on: c_int) -> c_int;
    pub fn crispy_asr_set_audio_ctx(h: *mut crispy_asr, n: c_int) -> c_int;
    pub fn crispy_asr_audio_ctx(h: *const crispy_asr, n: *mut c_int) -> c_int;
    pub fn crispy_asr_result_token_probs(r: *const crispy_asr_result, plog: *mut *const c_float, p_forced: *mut *const c_float, n: *mut c_int) -> c_int;
    pub fn crispy_asr_result_word_probs(r: *const crispy_asr_result, prob: *mut *const c_float, n: *mut c_int) -> c_int;
    pub fn crispy_asr_result_language_probs(r: *const crispy_asr_result, probs: *mut *const c_float, n_lang: *mut c_int) -> c_int;
    pub fn crispy_asr_detect_language_probs_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, lang_tokens_out: *mut c_int, probs_out: *mut c_float) -> c_int;
    pub fn crispy_asr_token_probs_device(h: *mut crispy_asr, d_enc: *const c_float, batch: c_int, tokens: *const c_int, n_tokens: *const c_int, ld_tokens: c_int, n_sot: c_int, logp_out: *mut c_float) -> c_int;
    pub fn crispy_asr_transcribe_recording(h: *mut crispy_asr, pcm16k: *const c_float, n: usize, opts: *const crispy_asr_opts, max_batch: c_int, cancel_flag: *const c_int, progress: crispy_asr_progress_fn, progress_user: *mut c_void, out: *mut *mut crispy_asr_result) -> c_int;
    pub fn crispy_asr_transcribe_hooks(h: *mut crispy_asr, pcm16k: *const c_float, n: usize, opts: *const crispy_asr_opts, cancel_flag: *const c_int, progress: crispy_asr_progress_fn, progress_user: *mut c_void, out: *mut *mut crispy_asr_result) -> c_int;

    pub fn crispy_resampler_create(device: c_int, out: *mut *mut crispy_resampler) -> c_int;
    pub fn crispy_resampler_destroy(h: *mut crispy_resampler);
    pub fn crispy_resampler_out_len(n_in: c_long) -> c_long;
    pub fn crispy_resampler_process_device(h: *mut crispy_resampler, d_in: *const c_float, in_stride: c_long, n_in: c_long, batch: c_int, scale: c_float, wav_s16: c_int, d_out: *mut c_float, out_stride: c_long, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_resampler_synchronize(h: *mut crispy_resampler) -> c_int;
    // speaker clustering and diarized text (managers/diarization.rs:276-724); the handle is a `void *`
    pub fn crispy_diar_create(device: c_int, out: *mut *mut c_void) -> c_int;
    pub fn crispy_diar_destroy(h: *mut c_void);
    pub fn crispy_diar_cluster(h: *mut c_void, emb: *const c_float, n: *const c_int, batch: c_int, dim: c_int, max_speakers: c_int, labels: *mut c_int, info: *mut c_void) -> c_int;
    pub fn crispy_diar_cluster_device(h: *mut c_void, d_emb: *const c_float, n: *const c_int, batch: c_int, dim: c_int, max_speakers: c_int, d_labels: *mut c_int, info: *mut c_void, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_diar_affinity_device(h: *mut c_void, d_emb: *const c_float, n: c_int, dim: c_int, d_aff: *mut c_float) -> c_int;
    pub fn crispy_diar_laplacian_device(h: *mut c_void, d_aff: *const c_float, n: c_int, p: c_int, d_lap: *mut c_float) -> c_int;
    pub fn crispy_diar_eigh_device(h: *mut c_void, d_mats: *const c_float, n: c_int, n_mats: c_int, d_evals: *mut c_float, d_evecs: *mut c_float) -> c_int;
    pub fn crispy_diar_decide_device(h: *mut c_void, d_evals: *const c_float, n: c_int, p_max: c_int, max_speakers: c_int, info: *mut c_void) -> c_int;
    pub fn crispy_diar_kmeans_device(h: *mut c_void, d_vecs: *const c_float, n: c_int, k: c_int, d_labels: *mut c_int, d_points: *mut c_float, d_centers: *mut c_float) -> c_int;
    pub fn crispy_diar_chunk_plan(start: *const f64, end: *const f64, n_samples: *const c_long, n_segments: c_long, sample_rate: c_int, out_start: *mut f64, out_end: *mut f64, out_segment: *mut c_long, out_first: *mut c_long, out_len: *mut c_long, cap: c_long) -> c_long;
    pub fn crispy_diar_speaker_segments(start: *const f64, end: *const f64, labels: *const c_int, n: c_long, merge_gap: f64, out_start: *mut f64, out_end: *mut f64, out_speaker: *mut c_int, cap: c_long) -> c_long;
    pub fn crispy_diar_find_speaker(time: f64, seg_start: *const f64, seg_end: *const f64, seg_speaker: *const c_int, n_segments: c_long) -> c_int;
    pub fn crispy_diar_format_text(t0: *const f64, t1: *const f64, text: *const *const c_char, n_words: c_long, seg_start: *const f64, seg_end: *const f64, seg_speaker: *const c_int, n_segments: c_long, out: *mut c_char, cap: usize, needed: *mut usize) -> c_int;
    pub fn crispy_diar_format_result(r: *const crispy_asr_result, chunk_offset: f64, seg_start: *const f64, seg_end: *const f64, seg_speaker: *const c_int, n_segments: c_long, out: *mut c_char, cap: usize, needed: *mut usize) -> c_int;
    pub fn crispy_diar_fbank_frames(n_samples: c_long) -> c_long;
    pub fn crispy_diar_speech_segments(scores: *const c_float, n_windows: c_long, n_frames: c_int, n_classes: c_int, n_samples: c_long, sample_rate: c_int, merge_gap: f64, out_start: *mut f64, out_end: *mut f64, out_first: *mut c_long, out_len: *mut c_long, cap: c_long) -> c_long;
    pub fn crispy_diar_fbank_device(h: *mut c_void, d_pcm: *const c_void, pcm_format: c_int, first: *const c_long, len: *const c_long, n_chunks: c_int, scale: c_float, d_feats: *mut c_float, d_raw: *mut c_float, frame_offset: *mut c_long, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_diar_fbank(h: *mut c_void, pcm: *const c_void, pcm_format: c_int, first: *const c_long, len: *const c_long, n_chunks: c_int, scale: c_float, feats: *mut c_float, frame_offset: *mut c_long) -> c_int;
    // the segmentation network (pyannote segmentation-3.0) on a crispy_diar handle: the first session.run of run_diarization
    pub fn crispy_diar_seg_frames(len: c_long) -> c_long;
    pub fn crispy_diar_seg_windows(n_samples: c_long) -> c_long;
    pub fn crispy_diar_seg_load(h: *mut c_void, names: *const *const c_char, data: *const *const c_float, count: *const c_long, n_tensors: c_int) -> c_int;
    pub fn crispy_diar_seg_loaded(h: *mut c_void) -> c_int;
    pub fn crispy_diar_seg_forward_device(h: *mut c_void, d_x: *const c_float, n_win: c_int, len: c_long, d_scores: *mut c_float, d_sincnet: *mut c_float, d_lstm: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_diar_seg_scores_device(h: *mut c_void, d_pcm: *const c_void, pcm_format: c_int, n_samples: c_long, d_scores: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_diar_seg_scores(h: *mut c_void, pcm: *const c_void, pcm_format: c_int, n_samples: c_long, scores: *mut c_float) -> c_int;
    // the embedding network (WeSpeaker CAMPPlus) on a crispy_diar handle: EmbeddingExtractor::compute for all chunks in one call
    pub fn crispy_diar_emb_frames(rows: c_long) -> c_long;
    pub fn crispy_diar_emb_tensor_spec(i: c_int, dim: c_int, name: *mut *const c_char, count: *mut c_long) -> c_int;
    pub fn crispy_diar_emb_load(h: *mut c_void, names: *const *const c_char, data: *const *const c_float, count: *const c_long, n_tensors: c_int) -> c_int;
    pub fn crispy_diar_emb_loaded(h: *mut c_void) -> c_int;
    pub fn crispy_diar_emb_dim(h: *mut c_void) -> c_int;
    pub fn crispy_diar_emb_forward_device(h: *mut c_void, d_feats: *const c_float, frame_offset: *const c_long, n_chunks: c_int, d_emb: *mut c_float, d_head: *mut c_float, d_xvec: *mut c_float, d_stats: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_diar_embed_device(h: *mut c_void, d_pcm: *const c_void, pcm_format: c_int, first: *const c_long, len: *const c_long, n_chunks: c_int, scale: c_float, d_emb: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_diar_embed(h: *mut c_void, pcm: *const c_void, pcm_format: c_int, first: *const c_long, len: *const c_long, n_chunks: c_int, scale: c_float, emb: *mut c_float) -> c_int;
    // Parakeet encoder; `cfg` points at a `crispy_pk_config`
    pub fn crispy_pk_create(device: c_int, out: *mut *mut c_void) -> c_int;
    pub fn crispy_pk_destroy(h: *mut c_void);
    pub fn crispy_pk_frames(rows: c_long) -> c_long;
    pub fn crispy_pk_tensor_spec(cfg: *const c_void, i: c_int, name: *mut *const c_char, count: *mut c_long) -> c_int;
    pub fn crispy_pk_load(h: *mut c_void, cfg: *const c_void, names: *const *const c_char, data: *const *const c_float, count: *const c_long, n_tensors: c_int) -> c_int;
    pub fn crispy_pk_loaded(h: *mut c_void) -> c_int;
    pub fn crispy_pk_config_of(h: *mut c_void, cfg: *mut c_void) -> c_int;
    pub fn crispy_pk_encode_device(h: *mut c_void, d_feats: *const c_float, frame_offset: *const c_long, n_clips: c_int, d_out: *mut c_float, d_sub: *mut c_float, tap_layer: c_int, d_tap: *mut c_float, d_pos: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_pk_encode(h: *mut c_void, feats: *const c_float, frame_offset: *const c_long, n_clips: c_int, out: *mut c_float, sub: *mut c_float, tap_layer: c_int, tap: *mut c_float, pos: *mut c_float) -> c_int;
    // Parakeet encoder, precision mode 1 (f16 operands, f32 sums); `epilogue` is CRISPY_PK_GEMM_SCALE 0, _SILU 1, _RESIDUAL 2, _GLU 3
    pub fn crispy_pk_set_precision(h: *mut c_void, mode: c_int) -> c_int;
    pub fn crispy_pk_precision(h: *mut c_void) -> c_int;
    pub fn crispy_pk_stage_gemm_device(h: *mut c_void, mode: c_int, epilogue: c_int, d_a: *const c_float, m: c_long, k: c_int, d_w: *const c_float, d_bias: *const c_float, n: c_int, alpha: c_float, d_res: *const c_float, d_c: *mut c_float) -> c_int;
    // Parakeet encoder, attention mode 1 (f16 operands in the attention's three products, f32 sums; key tile CRISPY_PK_ATTN_KEY_TILE 32)
    pub fn crispy_pk_set_attention_precision(h: *mut c_void, mode: c_int) -> c_int;
    pub fn crispy_pk_attention_precision(h: *mut c_void) -> c_int;
    pub fn crispy_pk_stage_attention_device(h: *mut c_void, mode: c_int, d_qkv: *const c_float, d_r: *const c_float, d_bias_u: *const c_float, d_bias_v: *const c_float, frame_offset: *const c_long, n_clips: c_int, heads: c_int, tmax: c_int, d_out: *mut c_float) -> c_int;
    // Parakeet TDT decoder; `cfg` points at a `crispy_pk_tdt_config`
    pub fn crispy_pk_tdt_create(device: c_int, out: *mut *mut c_void) -> c_int;
    pub fn crispy_pk_tdt_destroy(h: *mut c_void);
    pub fn crispy_pk_tdt_tensor_spec(cfg: *const c_void, i: c_int, name: *mut *const c_char, count: *mut c_long) -> c_int;
    pub fn crispy_pk_tdt_load(h: *mut c_void, cfg: *const c_void, names: *const *const c_char, data: *const *const c_float, count: *const c_long, n_tensors: c_int) -> c_int;
    pub fn crispy_pk_tdt_loaded(h: *mut c_void) -> c_int;
    pub fn crispy_pk_tdt_config_of(h: *mut c_void, cfg: *mut c_void) -> c_int;
    pub fn crispy_pk_tdt_max_steps(cfg: *const c_void, frames: c_long) -> c_long;
    pub fn crispy_pk_tdt_decode_device(h: *mut c_void, d_frames: *const c_float, frame_offset: *const c_long, n_clips: c_int, d_steps: *mut c_int, d_n_steps: *mut c_int, d_proj_tap: *mut c_float, d_logits_tap: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_pk_tdt_decode(h: *mut c_void, frames: *const c_float, frame_offset: *const c_long, n_clips: c_int, steps: *mut c_int, n_steps: *mut c_int, proj_tap: *mut c_float, logits_tap: *mut c_float) -> c_int;
    pub fn crispy_pk_tdt_words(steps: *const c_int, n_steps: c_int, frames: c_int, blank: c_int, pieces: *const *const c_char, vocab: c_int, seconds_per_frame: f64, start_s: *mut c_float, end_s: *mut c_float, text_off: *mut c_long, max_words: c_int, text: *mut c_char, text_cap: c_long, text_needed: *mut c_long) -> c_long;

    // Parakeet front end; `h` / `h_enc` is a `crispy_pk_create` handle, `h_tdt` a `crispy_pk_tdt_create` handle
    pub fn crispy_pk_feature_rows(samples: c_long) -> c_long;
    pub fn crispy_pk_mel_filters(mel_bins: c_int, fb: *mut c_float) -> c_int;
    pub fn crispy_pk_set_mel_filters(h: *mut c_void, mel_bins: c_int, fb: *const c_float) -> c_int;
    pub fn crispy_pk_features_device(h: *mut c_void, mel_bins: c_int, d_pcm: *const c_float, sample_offset: *const c_long, n_clips: c_int, d_feats: *mut c_float, d_raw_tap: *mut c_float, d_stats_tap: *mut c_float, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_pk_features(h: *mut c_void, mel_bins: c_int, pcm: *const c_float, sample_offset: *const c_long, n_clips: c_int, feats: *mut c_float, raw_tap: *mut c_float, stats_tap: *mut c_float) -> c_int;
    pub fn crispy_pk_transcribe_device(h_enc: *mut c_void, h_tdt: *mut c_void, d_pcm: *const c_float, sample_offset: *const c_long, n_clips: c_int, d_steps: *mut c_int, d_n_steps: *mut c_int, hip_stream: *mut c_void) -> c_int;
    pub fn crispy_pk_transcribe(h_enc: *mut c_void, h_tdt: *mut c_void, pcm: *const c_float, sample_offset: *const c_long, n_clips: c_int, steps: *mut c_int, n_steps: *mut c_int) -> c_int;
}

// ------------------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------------------
/// Status code + the library's thread-local message for it.
#[derive(Debug, Clone)]
pub struct CrispyError {
    pub code: c_int,
    pub message: String,
}
impl std::fmt::Display for CrispyError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "crispy_hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for CrispyError {}

fn check(rc: c_int) -> Result<(), CrispyError> {
    if rc == CRISPY_OK {
        return Ok(());
    }
    // SAFETY: crispy_last_error returns a NUL-terminated thread-local buffer that lives as long as the thread.
    let message = unsafe { CStr::from_ptr(crispy_last_error()) }.to_string_lossy().into_owned();
    Err(CrispyError { code: rc, message })
}

/// Refuses a library built from another header: a `crispy_asr_opts` of another size would be read past its end.
fn check_abi() -> Result<(), CrispyError> {
    // SAFETY: no arguments, no state.
    let got = unsafe { crispy_abi_version() };
    if got != CRISPY_ABI_VERSION {
        return Err(CrispyError { code: CRISPY_ERR_UNSUPPORTED, message: format!("libcrispy_hip ABI {got}, binding written for {CRISPY_ABI_VERSION}") });
    }
    Ok(())
}

fn path_cstring(p: &Path) -> Result<CString, CrispyError> {
    CString::new(p.to_string_lossy().as_bytes()).map_err(|_| CrispyError {
        code: CRISPY_ERR_INVALID_ARG,
        message: "path contains a NUL byte".into(),
    })
}

// ------------------------------------------------------------------------------------------------------------
// nnnoiseless-shaped denoiser
// ------------------------------------------------------------------------------------------------------------
/// == `nnnoiseless::FRAME_SIZE` (audio.rs:4)
pub const FRAME_SIZE: usize = CRISPY_RN_FRAME_SIZE;

/// Same shape as `nnnoiseless::DenoiseState`: a constructor and `process_frame(out, in) -> f32`, one stream.
///
/// `RnnNoiseProcessor` keeps everything it does around the call: x32768 (audio.rs:264), /32768 + clamp + volume
/// (audio.rs:270-273), first-frame drop (audio.rs:275-278).
pub struct DenoiseState {
    h: *mut crispy_rn,
    failed: Option<CrispyError>,
}
// SAFETY: the handle is owned exclusively and the library allows different threads to use a handle as long as calls
// are serialised -- which `&mut self` guarantees; the reference moves the processor into the cpal closure
// (audio.rs:751) behind Arc<Mutex<..>> (audio.rs:693).
unsafe impl Send for DenoiseState {}

impl DenoiseState {
    /// `DenoiseState::new()` has no arguments upstream because the model is compiled into the crate.  That blob
    /// cannot be redistributed with this library, so the model comes from an rnnoise-nu text file (the format
    /// `nnnoiseless::RnnModel::from_read` parses) ...
    pub fn from_model_file(path: &Path) -> Result<Box<Self>, CrispyError> {
        check_abi()?;
        let c = path_cstring(path)?;
        let mut h = std::ptr::null_mut();
        // SAFETY: c outlives the call; h is a valid out-pointer.
        check(unsafe { crispy_rn_create_from_file(c.as_ptr(), 1, 0, &mut h) })?;
        Ok(Box::new(Self { h, failed: None }))
    }
    /// ... or from the flat 87 503-byte int8 blob (layer order input_dense, vad_gru, vad_output, noise_gru,
    /// denoise_gru, denoise_output).
    pub fn from_weights(weights: &[i8]) -> Result<Box<Self>, CrispyError> {
        check_abi()?;
        let mut h = std::ptr::null_mut();
        // SAFETY: the slice is valid for weights.len() bytes; the library copies it before returning.
        check(unsafe { crispy_rn_create(weights.as_ptr(), weights.len(), 1, 0, &mut h) })?;
        Ok(Box::new(Self { h, failed: None }))
    }
    /// `process_frame(&mut self, output, input) -> f32` (audio.rs:268): 480 samples each, f32 in int16 range;
    /// returns the VAD probability.  The signature is infallible like upstream's (slice lengths are asserted, as upstream
    /// does).  A device failure after construction -- which upstream cannot have -- must not turn into permanent
    /// silence in the audio callback with nobody told: the frame is passed through UNDENOISED (the microphone keeps
    /// working), VAD 0 is returned, and the error is latched for the host to poll with `take_error()` (e.g. once per
    /// second from the thread that owns `NsState`, which can then fall back to `NoiseSuppressionMode::Off`).
    pub fn process_frame(&mut self, output: &mut [f32], input: &[f32]) -> f32 {
        assert_eq!(input.len(), FRAME_SIZE);
        assert_eq!(output.len(), FRAME_SIZE);
        let mut vad = 0f32;
        // SAFETY: both slices hold exactly one frame; the call returns when `output` is complete.
        let rc = unsafe { crispy_rn_process(self.h, input.as_ptr(), output.as_mut_ptr(), &mut vad, 1, CRISPY_RN_LAYOUT_TBF) };
        if rc != CRISPY_OK {
            if self.failed.is_none() {
                self.failed = check(rc).err();       // the first failure, with the library's message for this thread
            }
            output.copy_from_slice(input);
            return 0.0;
        }
        vad
    }
    /// The first error `process_frame` met since the last call, if any (and clears it).
    pub fn take_error(&mut self) -> Option<CrispyError> {
        self.failed.take()
    }
    /// True once a `process_frame` call has failed and the error has not been taken yet.
    pub fn has_failed(&self) -> bool {
        self.failed.is_some()
    }
    /// What `set_monitoring_model` does by replacing the processor (audio.rs:955-965).
    pub fn reset(&mut self) -> Result<(), CrispyError> {
        // SAFETY: valid handle.
        check(unsafe { crispy_rn_reset(self.h, -1) })
    }
}
impl Drop for DenoiseState {
    fn drop(&mut self) {
        // SAFETY: the handle came from crispy_rn_create* and is destroyed exactly once.
        unsafe { crispy_rn_destroy(self.h) }
    }
}

/// B streams in lock step: `[n_frames][n_streams][480]` tensors from host memory (a server denoising thousands of
/// calls, or a long recording cut into independent segments).  This is where the GPU pays off.
pub struct BatchDenoiser {
    h: *mut crispy_rn,
    n_streams: usize,
}
unsafe impl Send for BatchDenoiser {}
impl BatchDenoiser {
    pub fn from_model_file(path: &Path, n_streams: usize, device: i32) -> Result<Self, CrispyError> {
        let c = path_cstring(path)?;
        let mut h = std::ptr::null_mut();
        check(unsafe { crispy_rn_create_from_file(c.as_ptr(), n_streams as c_int, device, &mut h) })?;
        Ok(Self { h, n_streams })
    }
    /// input / output: `n_frames * n_streams * 480` samples, frame-major (`CRISPY_RN_LAYOUT_TBF`); vad (optional):
    /// `n_frames * n_streams`.
    pub fn process(&mut self, input: &[f32], output: &mut [f32], vad: Option<&mut [f32]>, n_frames: usize) -> Result<(), CrispyError> {
        let n = n_frames * self.n_streams * FRAME_SIZE;
        if input.len() != n || output.len() != n || vad.as_ref().map_or(false, |v| v.len() != n_frames * self.n_streams) {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::process: slice lengths".into() });
        }
        let vp = vad.map_or(std::ptr::null_mut(), |v| v.as_mut_ptr());
        check(unsafe { crispy_rn_process(self.h, input.as_ptr(), output.as_mut_ptr(), vp, n_frames as c_int, CRISPY_RN_LAYOUT_TBF) })
    }
    /// `RnnNoiseProcessor::new(input_rate, _, volume)` (audio.rs:216-240) for every stream: a capture rate that is not
    /// within 1 Hz of 48 kHz puts the reference's `LinearResampler` in front; fresh adapter and denoiser state.
    pub fn configure_adapter(&mut self, input_rate: f32, volume: f32) -> Result<(), CrispyError> {
        // SAFETY: valid handle.
        check(unsafe { crispy_rn_adapter_configure(self.h, input_rate, volume) })
    }
    /// `NsState::set_volume` (audio.rs:337-343); holds from the next `push` on.
    pub fn set_volume(&mut self, volume: f32) -> Result<(), CrispyError> {
        check(unsafe { crispy_rn_adapter_set_volume(self.h, volume) })
    }
    /// `NsState::produced_rate_hz` (audio.rs:352-357).
    pub fn produced_rate_hz(&self) -> Result<f32, CrispyError> {
        let mut r = 0f32;
        check(unsafe { crispy_rn_adapter_produced_rate_hz(self.h, &mut r) })?;
        Ok(r)
    }
    /// Samples per stream the next `push` of `n_in` samples returns.
    pub fn push_out_len(&self, n_in: usize) -> Result<usize, CrispyError> {
        let n = unsafe { crispy_rn_push_out_len(self.h, n_in as c_long) };
        if n < 0 {
            check(n as c_int)?;
        }
        Ok(n as usize)
    }
    /// The body of one capture callback: what a loop of `RnnNoiseProcessor::push_sample` (audio.rs:242-295) over `n_in`
    /// raw samples of every stream returns, from one call.  input: `n_streams` rows of `n_in` samples (+-1, at the
    /// configured capture rate); output: `n_streams` rows of `push_out_len(n_in)` samples (resized here).  Returns the
    /// samples per stream.  (The VAD probabilities, which push_sample discards, are available through the C entry point.)
    pub fn push(&mut self, input: &[f32], n_in: usize, output: &mut Vec<f32>) -> Result<usize, CrispyError> {
        if input.len() != n_in * self.n_streams {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::push: input length".into() });
        }
        let want = self.push_out_len(n_in)?;
        output.resize(want * self.n_streams, 0.0);
        let mut got: c_long = 0;
        // SAFETY: input holds n_streams rows of n_in samples, output n_streams rows of `want` samples -- what the library
        // announced for this push; the call returns when output is complete.
        check(unsafe { crispy_rn_push(self.h, input.as_ptr(), n_in as c_long, n_in as c_long, output.as_mut_ptr(), want as c_long, std::ptr::null_mut(), &mut got) })?;
        debug_assert_eq!(got as usize, want);
        Ok(got as usize)
    }
    /// The playback side of `RnnNoiseProcessor::new(_, output_rate, _)`: an empty `output_buf` of one second and
    /// `resample_pos = 0`; from here on every `push` also feeds the ring that `pull` reads.
    pub fn configure_playback(&mut self, output_rate: f32) -> Result<(), CrispyError> {
        check(unsafe { crispy_rn_playback_configure(self.h, output_rate) })
    }
    /// `output_buf.len()`, the same for every stream.
    pub fn playback_buffered(&self) -> Result<usize, CrispyError> {
        let n = unsafe { crispy_rn_playback_buffered(self.h) };
        if n < 0 {
            check(n as c_int)?;
        }
        Ok(n as usize)
    }
    /// The body of one f32 output callback: `n_frames` calls of `next_sample` (audio.rs:297-314) per stream, each written
    /// to `channels` interleaved channels.  output: `n_streams` rows of `n_frames * channels` samples (resized here).
    /// Returns how many of the frames were real samples and not underrun zeros.  (i16 / u16 output: the C entry point.)
    pub fn pull(&mut self, n_frames: usize, channels: usize, output: &mut Vec<f32>) -> Result<usize, CrispyError> {
        let row = n_frames * channels;
        output.resize(row * self.n_streams, 0.0);
        let mut live: c_long = 0;
        // SAFETY: output holds n_streams rows of n_frames * channels f32; the call returns when output is complete.
        check(unsafe { crispy_rn_pull(self.h, n_frames as c_long, channels as c_int, CRISPY_PCM_F32, output.as_mut_ptr() as *mut c_void, row as c_long, &mut live) })?;
        Ok(live as usize)
    }
    /// `start_recording`: empty mic and app rings of `ring_samples` per stream (0 = the reference's ten seconds); from here on
    /// every `push` that returns samples also feeds the mic ring that `record_drain` reads.
    pub fn configure_recording(&mut self, ring_samples: usize) -> Result<(), CrispyError> {
        check(unsafe { crispy_rn_record_configure(self.h, ring_samples as c_long) })
    }
    /// The app-audio capture handler (recording.rs:260-369): `n_frames` interleaved frames of `channels` samples per stream,
    /// already at 48 kHz, downmixed on the device and appended to the app ring.  input: `n_streams` rows of `n_frames * channels`.
    pub fn record_app_push(&mut self, input: &[f32], n_frames: usize, channels: usize) -> Result<(), CrispyError> {
        let row = n_frames * channels;
        if input.len() != row * self.n_streams {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::record_app_push: input length".into() });
        }
        // SAFETY: input holds n_streams rows of n_frames * channels samples; the call returns when they are in the ring.
        check(unsafe { crispy_rn_record_app_push(self.h, input.as_ptr(), row as c_long, n_frames as c_long, channels as c_int) })
    }
    /// The capture callback's level meter (audio.rs:728-729, 779-781) over `n_in` samples of every stream: one rms per stream.
    pub fn level(&mut self, input: &[f32], n_in: usize, rms: &mut Vec<f32>) -> Result<(), CrispyError> {
        if input.len() != n_in * self.n_streams {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::level: input length".into() });
        }
        rms.resize(self.n_streams, 0.0);
        // SAFETY: input holds n_streams rows of n_in samples, rms n_streams values; the call returns when rms is complete.
        check(unsafe { crispy_rn_level(self.h, input.as_ptr(), n_in as c_long, n_in as c_long, rms.as_mut_ptr()) })
    }
    /// `record_app_push` for a stream at its own rate (the macOS handler's `resample_audio`, recording.rs:13-39): downmix,
    /// resampling to 48 kHz and the ring append on the device.  `from_rate` 8000...384000; 48000 is `record_app_push`.
    pub fn record_app_push_at(&mut self, input: &[f32], n_frames: usize, channels: usize, from_rate: u32) -> Result<(), CrispyError> {
        let row = n_frames * channels;
        if input.len() != row * self.n_streams {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::record_app_push_at: input length".into() });
        }
        // SAFETY: input holds n_streams rows of n_frames * channels samples; the call returns when they are in the ring.
        check(unsafe { crispy_rn_record_app_push_at(self.h, input.as_ptr(), row as c_long, n_frames as c_long, channels as c_int, from_rate as c_int) })
    }
    /// Noise suppression off, recording on (the `shared == None` arm, audio.rs:545, 697-714): from here on `capture_i16` /
    /// `capture_f32` resample the raw mono to 48 kHz instead of denoising it.  0 returns to the RNNoise arm.
    pub fn configure_bypass(&mut self, raw_input_rate: f32) -> Result<(), CrispyError> {
        check(unsafe { crispy_rn_bypass_configure(self.h, raw_input_rate) })
    }
    /// `set_monitoring_model` (audio.rs:942-967): a fresh processor of the named model at the configured rates and the current
    /// volume, also when the model is unchanged -- "rnnnoise", "noisy", anything else the dummy (`ModelKind::from_name`).
    /// From here on push, pull and capture are that processor's: for the Legacy models `SharedAudio` (audio.rs:136-200).
    pub fn set_model(&mut self, name: &str) -> Result<(), CrispyError> {
        let model = match name {
            "rnnnoise" => CRISPY_NS_RNNOISE,
            "noisy" => CRISPY_NS_NOISY,
            _ => CRISPY_NS_DUMMY,
        };
        check(unsafe { crispy_rn_model_configure(self.h, model) })
    }
    /// The handle's model, a CRISPY_NS_* code.
    pub fn model(&self) -> Result<c_int, CrispyError> {
        let mut model: c_int = 0;
        check(unsafe { crispy_rn_model(self.h, &mut model) })?;
        Ok(model)
    }
    /// Samples per stream the next capture of `n_frames` frames returns.
    pub fn capture_out_len(&self, n_frames: usize) -> Result<usize, CrispyError> {
        let n = unsafe { crispy_rn_capture_out_len(self.h, n_frames as c_long) };
        if n < 0 {
            check(n as c_int)?;
        }
        Ok(n as usize)
    }
    fn capture_raw(&mut self, input: *const c_void, n_frames: usize, channels: usize, format: c_int, output: &mut Vec<f32>, rms: &mut Vec<f32>) -> Result<usize, CrispyError> {
        let want = self.capture_out_len(n_frames)?;
        output.resize(want * self.n_streams, 0.0);
        rms.resize(self.n_streams, 0.0);
        let mut got: c_long = 0;
        // SAFETY: the callers checked that input holds n_streams rows of n_frames * channels elements of `format`; output holds
        // n_streams rows of `want` samples -- what the library announced --, rms n_streams values; the call returns when both
        // are complete.
        check(unsafe { crispy_rn_capture(self.h, input, (n_frames * channels) as c_long, n_frames as c_long, channels as c_int, format, output.as_mut_ptr(), want.max(1) as c_long, rms.as_mut_ptr(), &mut got) })?;
        debug_assert_eq!(got as usize, want);
        Ok(got as usize)
    }
    /// The whole body of one i16 capture callback (build_input_stream_i16 + push_mono_to_buffers, audio.rs:682-730, 794-855):
    /// `s as f32 / 32768.0`, the downmix of `channels` interleaved samples per frame, the level meter and the handle's arm,
    /// from the device's own samples.  input: `n_streams` rows of `n_frames * channels`; output (resized here): what the arm
    /// returned per stream; rms (resized here): one level per stream.  Returns the samples per stream.
    pub fn capture_i16(&mut self, input: &[i16], n_frames: usize, channels: usize, output: &mut Vec<f32>, rms: &mut Vec<f32>) -> Result<usize, CrispyError> {
        if input.len() != n_frames * channels * self.n_streams {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::capture_i16: input length".into() });
        }
        self.capture_raw(input.as_ptr() as *const c_void, n_frames, channels, CRISPY_PCM_I16, output, rms)
    }
    /// `capture_i16` for an f32 device (build_input_stream_f32, audio.rs:732-792).  (u16: the C entry point.)
    pub fn capture_f32(&mut self, input: &[f32], n_frames: usize, channels: usize, output: &mut Vec<f32>, rms: &mut Vec<f32>) -> Result<usize, CrispyError> {
        if input.len() != n_frames * channels * self.n_streams {
            return Err(CrispyError { code: CRISPY_ERR_INVALID_ARG, message: "BatchDenoiser::capture_f32: input length".into() });
        }
        self.capture_raw(input.as_ptr() as *const c_void, n_frames, channels, CRISPY_PCM_F32, output, rms)
    }
    /// (mic, app): samples per stream in the two recording rings.
    pub fn record_buffered(&self) -> Result<(usize, usize), CrispyError> {
        let (mut mic, mut app): (c_long, c_long) = (0, 0);
        check(unsafe { crispy_rn_record_buffered(self.h, &mut mic, &mut app) })?;
        Ok((mic as usize, app as usize))
    }
    /// 1152-sample frames a drain without a limit would write now.
    pub fn record_frames_ready(&self) -> Result<usize, CrispyError> {
        let n = unsafe { crispy_rn_record_frames_ready(self.h) };
        if n < 0 {
            check(n as c_int)?;
        }
        Ok(n as usize)
    }
    /// The recording worker's loop body (commands/recording.rs:215-264) for at most `max_frames` frames: the WAV payload,
    /// `n_streams` rows of `frames * 1152 * 2` interleaved s16 samples with L == R (output is resized here).  Returns the
    /// frames written.  (f32 channel 0 for the transcriber, device pointers: the C entry points.)
    pub fn record_drain(&mut self, max_frames: usize, output: &mut Vec<i16>) -> Result<usize, CrispyError> {
        let n = self.record_frames_ready()?.min(max_frames);
        let row = n * 1152 * 2;
        output.resize(row * self.n_streams, 0);
        if n == 0 {
            return Ok(0);
        }
        let mut got: c_long = 0;
        // SAFETY: output holds n_streams rows of n frames of 2304 i16 -- what the library announced; the call returns when
        // output is complete.
        check(unsafe { crispy_rn_record_drain(self.h, n as c_long, CRISPY_PCM_I16, output.as_mut_ptr() as *mut c_void, row as c_long, &mut got) })?;
        debug_assert_eq!(got as usize, n);
        Ok(got as usize)
    }
}
impl Drop for BatchDenoiser {
    fn drop(&mut self) {
        unsafe { crispy_rn_destroy(self.h) }
    }
}

// ------------------------------------------------------------------------------------------------------------
// transcribe-rs shaped engine
// ------------------------------------------------------------------------------------------------------------
/// One segment of a transcript: seconds relative to the start of the chunk (managers/transcription.rs:223-233).
#[derive(Debug, Clone, PartialEq)]
pub struct Segment {
    pub start: f32,
    pub end: f32,
    pub text: String,
}
/// What `engine.transcribe(..)` returns as far as the reference reads it (`.text`, `.segments`).
#[derive(Debug, Clone, Default, PartialEq)]
pub struct Transcript {
    pub text: String,
    pub segments: Option<Vec<Segment>>,
    pub tokens: Vec<i32>,
    pub language_token: i32,
    /// Per window of whisper_full's seek loop: temperature accepted, no_speech_prob, avg_logprob, entropy, dropped / failed.
    pub windows: Vec<crispy_asr_window>,
    /// With `dtw_token_timestamps`: the start of every token in seconds (-1 for timestamp tokens), parallel to `tokens`.
    pub token_times: Option<Vec<f32>>,
    /// With `dtw_token_timestamps`: the words, seconds relative to the chunk.
    pub words: Vec<Word>,
    /// Timestamp mode: the log-probability of every token under the distribution it was picked from (whisper.cpp's `plog`),
    /// parallel to `tokens` -- the addends of its window's `avg_logprob`.  `None` with `no_timestamps`.
    pub token_logprobs: Option<Vec<f32>>,
    /// `set_confidence(true)` + `dtw_token_timestamps`: openai-whisper's `text_token_probs`, the probability of every token in
    /// the teacher-forced alignment pass (-1 for timestamp tokens), parallel to `tokens`.
    pub token_probs_forced: Option<Vec<f32>>,
    /// `set_confidence(true)` + `dtw_token_timestamps`: openai-whisper's word `probability`, parallel to `words`.
    pub word_probs: Option<Vec<f32>>,
    /// `set_confidence(true)` + auto-detection: whisper.cpp's `lang_probs`; entry i belongs to language token `lang0 + i`.
    pub language_probs: Option<Vec<f32>>,
}
/// One word of a transcript (`dtw_token_timestamps`).
#[derive(Debug, Clone, PartialEq)]
pub struct Word {
    pub start: f32,
    pub end: f32,
    pub text: String,
    pub first_token: i32,
    pub n_tokens: i32,
}

/// `transcribe_rs::whisper_cpp::WhisperEngine`: `load(&path)` + `transcribe(&audio, &TranscribeOptions::default())`.
pub struct GpuWhisperEngine {
    h: *mut crispy_asr,
}
// SAFETY: as for DenoiseState; the reference keeps the engine in Mutex<Option<Box<dyn SpeechModel>>>
// (managers/transcription.rs:27) and calls it from a per-request thread (commands/transcription.rs:63).
unsafe impl Send for GpuWhisperEngine {}

impl GpuWhisperEngine {
    /// `WhisperEngine::load(&model_path)` (managers/transcription.rs:138-141): a whisper.cpp GGML model file.
    pub fn load(model_path: &Path) -> Result<Self, CrispyError> {
        check_abi()?;
        let c = path_cstring(model_path)?;
        let mut h = std::ptr::null_mut();
        // resident load: a quantised catalog file (managers/model.rs:99,137) stays quantised in HBM (file-sized) and runs in
        // precision mode 1 only; an f32 / f16 file (ggml-small.bin, large-v3-turbo) loads exactly as crispy_asr_load loads it
        // -- dense, every precision mode available.  Either way the engine is in precision mode 1 afterwards
        check(unsafe { crispy_asr_load_resident(c.as_ptr(), 0, &mut h) })?;
        // whisper.cpp, the engine this one stands in for, multiplies f16 operands with f32 accumulation and keeps its
        // K|V caches in f16: precision mode 1 is that arithmetic (and 2.3 x the f32 mode's speed).  The library's own
        // default stays f32 -- the mode its 1e-4 parity against the float64 oracle is stated in.
        let engine = Self { h };
        check(unsafe { crispy_asr_set_precision(engine.h, 1) })?;
        Ok(engine)
    }
    /// Vocabulary size of the loaded model (51864 English-only, 51865 multilingual, 51866 large-v3).
    pub fn n_vocab(&self) -> c_int {
        let mut hp = crispy_asr_hparams::default();
        if unsafe { crispy_asr_hparams_get(self.h, &mut hp) } == CRISPY_OK { hp.n_vocab } else { 0 }
    }
    /// 0: exact f32 products (parity mode; refused with CRISPY_ERR_UNSUPPORTED for a quantised file, which `load` keeps
    /// resident as ggml blocks); 1: whisper.cpp's f16-operand arithmetic (the default of `load`); 2: mode 1 plus ggml's
    /// remaining rounding points (LayerNorm outputs of the decode step, queries and normalised probabilities inside every
    /// attention), opt-in and slower.
    pub fn set_precision(&mut self, mode: i32) -> Result<(), CrispyError> {
        check(unsafe { crispy_asr_set_precision(self.h, mode as c_int) })
    }
    /// From the next transcribe call on, transcripts carry `language_probs` and -- with `dtw_token_timestamps` --
    /// `token_probs_forced` and `word_probs` (`token_logprobs` needs no switch).  Off (the default): nothing extra runs.
    pub fn set_confidence(&mut self, on: bool) -> Result<(), CrispyError> {
        check(unsafe { crispy_asr_set_confidence(self.h, on as c_int) })
    }
    /// `crispy_asr_detect_language_probs_device` on `batch` encoder outputs in device memory: the language token per clip
    /// and the distribution over the vocabulary's `n_lang` languages, `[batch][n_lang]` (empty for an English-only model).
    /// SAFETY: `d_enc` is a device pointer to `batch` encoder outputs of this model (`crispy_asr_encode_device`).
    pub unsafe fn detect_language_probs_device(&mut self, d_enc: *const f32, batch: usize) -> Result<(Vec<i32>, Vec<f32>), CrispyError> {
        let mut sp = crispy_asr_specials::default();
        check(crispy_asr_vocab_specials(self.n_vocab(), &mut sp))?;
        let mut tok = vec![0 as c_int; batch];
        let mut probs = vec![0f32; batch * sp.n_lang as usize];
        let pp = if probs.is_empty() { std::ptr::null_mut() } else { probs.as_mut_ptr() };
        check(crispy_asr_detect_language_probs_device(self.h, d_enc, batch as c_int, tok.as_mut_ptr(), pp))?;
        Ok((tok, probs))
    }
    /// `crispy_asr_token_probs_device`: `rows[b]` = clip b's token rows (sot sequence of `n_sot` ids, `<|notimestamps|>`, text,
    /// `<|endoftext|>`); returns per clip the LOG-probability of every text token given the rows before it.
    /// SAFETY: `d_enc` is a device pointer to `rows.len()` encoder outputs of this model.
    pub unsafe fn token_probs_device(&mut self, d_enc: *const f32, rows: &[Vec<i32>], n_sot: usize) -> Result<Vec<Vec<f32>>, CrispyError> {
        let ld = rows.iter().map(|r| r.len()).max().unwrap_or(0);
        let mut tok = vec![0 as c_int; rows.len() * ld];
        for (b, r) in rows.iter().enumerate() {
            tok[b * ld..b * ld + r.len()].copy_from_slice(r);
        }
        let n_tok: Vec<c_int> = rows.iter().map(|r| r.len() as c_int).collect();
        let mut lp = vec![0f32; rows.len() * ld];
        check(crispy_asr_token_probs_device(self.h, d_enc, rows.len() as c_int, tok.as_ptr(), n_tok.as_ptr(), ld as c_int, n_sot as c_int,
                                            lp.as_mut_ptr()))?;
        Ok(rows.iter().enumerate().map(|(b, r)| lp[b * ld..b * ld + r.len().saturating_sub(n_sot + 2)].to_vec()).collect())
    }
    /// Audio of any length up to `CRISPY_ASR_MAX_SAMPLES` (16 kHz, f32 in +-1) through ONE `whisper_full`: the log-mel of
    /// the whole recording, then 30 s windows that advance to the last closed timestamp pair and carry the text so far --
    /// what `SpeechModel::transcribe(&mut self, &[f32], ..)` means for a whisper.cpp engine, and not the hard 30 s cuts of
    /// `transcribe_recording`.  `opts = None` is `TranscribeOptions::default()`.  Segment, word and window times count from
    /// the start of `audio`.
    pub fn transcribe(&mut self, audio: &[f32], opts: Option<&crispy_asr_opts>) -> Result<Transcript, CrispyError> {
        self.transcribe_chunk(audio, opts)
    }
    /// One chunk (16 kHz, f32 in +-1) as the reference's chunker hands it over: at most 480 000 samples there, though the
    /// engine takes what `transcribe` takes; `opts = None` is `TranscribeOptions::default()`:
    /// language auto-detected, transcribe task, timestamps on.  Empty audio gives an empty transcript
    /// (managers/transcription.rs:175-177).
    pub fn transcribe_chunk(&mut self, audio: &[f32], opts: Option<&crispy_asr_opts>) -> Result<Transcript, CrispyError> {
        let mut r: *mut crispy_asr_result = std::ptr::null_mut();
        let o = opts.map_or(std::ptr::null(), |o| o as *const crispy_asr_opts);
        let p = if audio.is_empty() { std::ptr::null() } else { audio.as_ptr() };
        check(unsafe { crispy_asr_transcribe(self.h, p, audio.len(), o, &mut r) })?;
        Ok(unsafe { take_result(r) })
    }
    /// `TranscriptionManager::transcribe_with_timestamps` (managers/transcription.rs:200-249) with WORD times for the
    /// diarization path (`format_diarized_text` gives each word to a speaker by its midpoint, managers/diarization.rs:656-700):
    /// one `(offset + start, offset + end, word)` per word of the chunk, from cross-attention alignment over `heads`
    /// ((layer, head) pairs of the model; empty = every head of the last half of the decoder layers).  Empty audio or
    /// blank text gives no words.
    pub fn transcribe_with_timestamps_words(&mut self, audio: &[f32], chunk_offset_seconds: f32, heads: &[(i32, i32)])
                                            -> Result<Vec<(f32, f32, String)>, CrispyError> {
        if audio.is_empty() {
            return Ok(Vec::new());
        }
        let flat: Vec<c_int> = heads.iter().flat_map(|&(l, h)| [l as c_int, h as c_int]).collect();
        let mut o = crispy_asr_opts::default();
        o.dtw_token_timestamps = 1;
        if !flat.is_empty() {
            o.dtw_heads = flat.as_ptr();
            o.n_dtw_heads = heads.len() as c_int;
        }
        let t = self.transcribe_chunk(audio, Some(&o))?;
        if t.text.trim().is_empty() {
            return Ok(Vec::new());
        }
        Ok(t.words.into_iter().map(|w| (chunk_offset_seconds + w.start, chunk_offset_seconds + w.end, w.text)).collect())
    }
    /// `run_transcription`'s chunk loop (commands/transcription.rs:249-302, 363-400, 468) over a whole 16 kHz recording in
    /// ONE call: 30 s chunks decoded `max_batch` at a time (0 = 128), chunk texts trimmed and joined with a space.
    /// `cancel`: the reference's `Arc<AtomicBool>` (polled before every group and between windows; a set flag gives
    /// `Err` with `code == CRISPY_ERR_CANCELLED`, where the reference returns without saving).  `progress(done, total)` in
    /// samples after every group -- what the reference emits as "transcription-progress" (:285-299).
    pub fn transcribe_recording(&mut self, audio: &[f32], opts: Option<&crispy_asr_opts>, max_batch: usize,
                                cancel: Option<&std::sync::atomic::AtomicBool>, mut progress: Option<&mut dyn FnMut(usize, usize)>)
                                -> Result<Transcript, CrispyError> {
        unsafe extern "C" fn tramp(done: usize, total: usize, user: *mut c_void) {
            // SAFETY: `user` is the `&mut Option<&mut dyn FnMut>` of the enclosing call, alive for its whole duration.
            let f = &mut *(user as *mut Option<&mut dyn FnMut(usize, usize)>);
            if let Some(f) = f.as_mut() { f(done, total) }
        }
        // AtomicBool has the layout of a u8; the library reads an int.  A relay thread-free way: mirror the flag into an
        // AtomicI32 the callback refreshes would miss cancels between groups, so the flag the library polls is an i32 the
        // host sets directly when it can (`cancel_i32`); for an AtomicBool the mirror is refreshed by a watcher thread.
        let mirror = std::sync::Arc::new(std::sync::atomic::AtomicI32::new(0));
        let stop = std::sync::Arc::new(std::sync::atomic::AtomicBool::new(false));
        let watcher = cancel.map(|c| {
            let (m, st) = (mirror.clone(), stop.clone());
            let c_ptr = c as *const std::sync::atomic::AtomicBool as usize;
            std::thread::spawn(move || {
                // SAFETY: the AtomicBool outlives this call (borrowed for it); the thread is joined before it returns.
                let c = unsafe { &*(c_ptr as *const std::sync::atomic::AtomicBool) };
                while !st.load(std::sync::atomic::Ordering::Relaxed) {
                    if c.load(std::sync::atomic::Ordering::Relaxed) { m.store(1, std::sync::atomic::Ordering::Relaxed); break; }
                    std::thread::sleep(std::time::Duration::from_millis(2));
                }
            })
        });
        let mut r: *mut crispy_asr_result = std::ptr::null_mut();
        let o = opts.map_or(std::ptr::null(), |o| o as *const crispy_asr_opts);
        let p = if audio.is_empty() { std::ptr::null() } else { audio.as_ptr() };
        let cb: crispy_asr_progress_fn = if progress.is_some() { Some(tramp) } else { None };
        let rc = unsafe {
            crispy_asr_transcribe_recording(self.h, p, audio.len(), o, max_batch as c_int, mirror.as_ptr() as *const c_int, cb,
                                            &mut progress as *mut Option<&mut dyn FnMut(usize, usize)> as *mut c_void, &mut r)
        };
        stop.store(true, std::sync::atomic::Ordering::Relaxed);
        if let Some(w) = watcher { let _ = w.join(); }
        check(rc)?;
        Ok(unsafe { take_result(r) })
    }
}

/// Copies a library-owned result out and frees it.
/// SAFETY: `r` is a result a successful transcribe call returned and nobody has freed.
unsafe fn take_result(r: *mut crispy_asr_result) -> Transcript {
    let res = &*r;
    let text = if res.text.is_null() { String::new() } else { CStr::from_ptr(res.text).to_string_lossy().into_owned() };
    let tokens = if res.n_tokens > 0 { std::slice::from_raw_parts(res.tokens, res.n_tokens as usize).to_vec() } else { Vec::new() };
    let segments = if res.n_segments > 0 {
        Some(std::slice::from_raw_parts(res.segments, res.n_segments as usize).iter().map(|s| Segment {
            start: s.t0,
            end: s.t1,
            text: if s.text.is_null() { String::new() } else { CStr::from_ptr(s.text).to_string_lossy().into_owned() },
        }).collect())
    } else {
        None
    };
    let windows = if res.n_windows > 0 { std::slice::from_raw_parts(res.windows, res.n_windows as usize).to_vec() } else { Vec::new() };
    let token_times = if res.token_t_dtw.is_null() { None } else if res.n_tokens > 0 {
        Some(std::slice::from_raw_parts(res.token_t_dtw, res.n_tokens as usize).to_vec())
    } else {
        Some(Vec::new())
    };
    let words = if res.n_words > 0 && !res.words.is_null() {
        std::slice::from_raw_parts(res.words as *const crispy_asr_word, res.n_words as usize).iter().map(|w| Word {
            start: w.t0,
            end: w.t1,
            text: if w.text.is_null() { String::new() } else { CStr::from_ptr(w.text).to_string_lossy().into_owned() },
            first_token: w.first_token,
            n_tokens: w.n_tokens,
        }).collect()
    } else {
        Vec::new()
    };
    // the confidence arrays live behind the public prefix: NULL = not computed in this call (a present, empty array is non-NULL)
    let copy = |p: *const c_float, n: c_int| if p.is_null() { None } else if n > 0 { Some(std::slice::from_raw_parts(p, n as usize).to_vec()) } else { Some(Vec::new()) };
    let (mut plog, mut forced, mut wprob, mut lprob) = (std::ptr::null(), std::ptr::null(), std::ptr::null(), std::ptr::null());
    let (mut n_tok, mut n_word, mut n_lang) = (0 as c_int, 0 as c_int, 0 as c_int);
    let ok = crispy_asr_result_token_probs(r, &mut plog, &mut forced, &mut n_tok) == CRISPY_OK
        && crispy_asr_result_word_probs(r, &mut wprob, &mut n_word) == CRISPY_OK
        && crispy_asr_result_language_probs(r, &mut lprob, &mut n_lang) == CRISPY_OK;
    let (token_logprobs, token_probs_forced, word_probs, language_probs) =
        if ok { (copy(plog, n_tok), copy(forced, n_tok), copy(wprob, n_word), copy(lprob, n_lang)) } else { (None, None, None, None) };
    let out = Transcript { text, segments, tokens, language_token: res.language_token, windows, token_times, words, token_logprobs,
                           token_probs_forced, word_probs, language_probs };
    crispy_asr_free_result(r);
    out
}
impl Drop for GpuWhisperEngine {
    fn drop(&mut self) {
        unsafe { crispy_asr_free(self.h) }
    }
}

/// `impl SpeechModel for GpuWhisperEngine`, so that `TranscriptionManager::load_model`
/// (managers/transcription.rs:137-141) can box it as `LoadedEngine` for `EngineType::Whisper`.
/// The trait's exact item list lives in transcribe-rs 0.3.11, which is not vendored with the reference; the shape
/// below is what the reference's call sites require of it (`transcribe(&mut self, &[f32], &TranscribeOptions) ->
/// Result<R, E: Display>` with `R.text: String`, `R.segments: Option<Vec<S>>`, `S.{start, end, text}`:
/// managers/transcription.rs:183-187, 223-233).
#[cfg(feature = "speech-model")]
mod speech_model {
    use super::*;
    use transcribe_rs::{SpeechModel, TranscribeOptions, TranscriptionResult, TranscriptionSegment};

    impl SpeechModel for GpuWhisperEngine {
        // `TranscribeOptions { language: Option<String>, translate: bool }` [UPSTREAM-RECALL: transcribe-rs 0.3.11; the
        // reference only ever passes `TranscribeOptions::default()`, managers/transcription.rs:184,214 -- language unset,
        // transcribe]: a set language becomes its token, an unset one is detected per chunk, as whisper.cpp does.
        // (What transcribe-rs may set on whisper.cpp beyond these two -- suppress_nst, an initial prompt, no_context = false --
        // has a field in `crispy_asr_opts` since ABI 3; a host that knows the engine's settings passes them through
        // `transcribe_chunk(audio, Some(&opts))`; so does `beam_size` for an engine configured for BeamSearch.)
        fn transcribe(&mut self, audio: &[f32], options: &TranscribeOptions) -> Result<TranscriptionResult, Box<dyn std::error::Error + Send + Sync>> {
            let mut o = crispy_asr_opts::default();
            if let Some(code) = options.language.as_deref() {
                let c = std::ffi::CString::new(code)?;
                let mut tok: c_int = 0;
                check(unsafe { crispy_asr_language_token(self.n_vocab(), c.as_ptr(), &mut tok) })?;
                o.language_token = tok;
            }
            o.translate = options.translate as c_int;
            let t = GpuWhisperEngine::transcribe(self, audio, Some(&o))?;      // any length, as the trait's &[f32] promises
            Ok(TranscriptionResult {
                text: t.text,
                segments: t.segments.map(|v| v.into_iter().map(|s| TranscriptionSegment { start: s.start, end: s.end, text: s.text }).collect()),
            })
        }
    }
}

#[cfg(test)]
mod tests {
    use super::*;

    #[test]
    fn exception_guard_is_status_codes() {
        // needs no device
        unsafe {
            assert_eq!(crispy_selftest_exception_guard(0), CRISPY_OK);
            assert_eq!(crispy_selftest_exception_guard(1), CRISPY_ERR_OOM);
            assert_eq!(crispy_selftest_exception_guard(3), CRISPY_ERR_HIP);
        }
    }

    #[test]
    fn specials_of_the_three_vocabularies() {
        let mut sp = crispy_asr_specials::default();
        unsafe { assert_eq!(crispy_asr_vocab_specials(51864, &mut sp), CRISPY_OK) };
        assert_eq!((sp.eot, sp.sot, sp.translate, sp.notimestamps, sp.beg), (50256, 50257, 50357, 50362, 50363));
        unsafe { assert_eq!(crispy_asr_vocab_specials(51865, &mut sp), CRISPY_OK) };
        assert_eq!((sp.eot, sp.sot, sp.translate, sp.notimestamps, sp.beg), (50257, 50258, 50358, 50363, 50364));
    }

    #[test]
    fn missing_model_file_is_an_error_not_a_panic() {
        let e = DenoiseState::from_model_file(Path::new("/nonexistent/model.txt")).err().unwrap();
        assert_eq!(e.code, CRISPY_ERR_BAD_MODEL);
    }
}

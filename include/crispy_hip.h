/*
 * crispy_hip.h -- C ABI of libcrispy_hip.so: the MI355X (gfx950) implementation of crispy's
 * audio compute hot path.  Plain pointers and sizes only; no C++/torch types cross this line.
 *
 * Every entry point names the reference interface it replaces (paths are into sleep3r/crispy):
 *
 *   RNNoise   nnnoiseless::DenoiseState::{new, process_frame}
 *               ctor       src-tauri/src/audio.rs:229
 *               call site  src-tauri/src/audio.rs:268   (480-sample f32 frames, int16 range)
 *               state reset on model hot-swap          src-tauri/src/audio.rs:942-967
 *   ASR       transcribe_rs::SpeechModel::transcribe (whisper_cpp::WhisperEngine)
 *               load       src-tauri/src/managers/transcription.rs:138-141
 *               call sites src-tauri/src/managers/transcription.rs:183-185, 213-215
 *
 * Conventions
 *   - every function returns CRISPY_OK (0) or a negative crispy_status; nothing throws or
 *     aborts across the boundary (the reference builds with panic=abort, Cargo.toml:10-20);
 *     crispy_last_error() returns a thread-local message for the last failure.
 *   - a handle is not re-entrant: the caller serialises calls on one handle, exactly as the
 *     reference does with Arc<Mutex<NsState>> (audio.rs:693) / Mutex<Option<engine>>
 *     (managers/transcription.rs:27).  Different handles may be used from different threads.
 *   - there is NO CPU fallback: without a gfx950 device every create/load call fails with
 *     CRISPY_ERR_NO_DEVICE.
 *   - ABI version: CRISPY_ABI_VERSION below is bumped whenever a struct grows, an entry point goes away or an argument
 *     changes meaning; a binding compares it with crispy_abi_version() when it loads the library and refuses a
 *     mismatch (a caller built against an older crispy_asr_opts would have the library read past its struct).
 *
 * Environment.  The release library reads exactly these three variables -- test hooks that choose between forms whose
 * results are bit-identical (the test that uses one asserts that); nothing else in a host's environment changes what runs,
 * and nothing in it changes a result.  Developer A/B knobs exist only in the `make dev` build, libcrispy_hip_dev.so
 * (crispy_amd/csrc/api_util.h: dev_env) -- among them CRISPY_ASR_DECODE=stages, the decode step as one launch per stage,
 * whose results are NOT bit-identical to the fused step kernels' (tests/test_gpu_fused_decode.py compares the two builds).
 *     CRISPY_RN_WAVES=1|3        frame-kernel form of a crispy_rn handle (default: 3 up to 1280 streams, 1 above);
 *                                read by crispy_rn_create*            (tests/test_gpu_rnnoise.py)
 *     CRISPY_ASR_PREFILL=seq     prompt one position per step instead of multi-position steps; read per decode call
 *                                                                     (tests/test_gpu_prefill.py)
 *     CRISPY_ASR_TILE_ROWS=192|256  tile height of the mode-1 encoder GEMMs; read once per process
 *                                                                     (tests/test_gpu_mode1.py)
 */
#ifndef CRISPY_HIP_H
#define CRISPY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum crispy_status {
  CRISPY_OK = 0,
  CRISPY_ERR_INVALID_ARG = -1,
  CRISPY_ERR_NO_DEVICE = -2,
  CRISPY_ERR_HIP = -3,
  CRISPY_ERR_OOM = -4,
  CRISPY_ERR_BAD_MODEL = -5,
  CRISPY_ERR_UNSUPPORTED = -6,
  CRISPY_ERR_CANCELLED = -7, /* crispy_asr_transcribe_recording / _hooks: the caller's cancel flag was set; no result */
  CRISPY_ERR_INTERNAL = -8   /* crispy_diar_*: the eigensolver did not converge within its sweep cap; no result */
} crispy_status;

#define CRISPY_RN_FRAME_SIZE 480      /* nnnoiseless::FRAME_SIZE (audio.rs:4) */
#define CRISPY_RN_WEIGHT_BYTES 87503  /* SURVEY.md Appendix A.5 */
#define CRISPY_RN_TAPS 72

/* Sample layouts of the batched frame tensors handed to crispy_rn_process*. */
typedef enum crispy_rn_layout {
  CRISPY_RN_LAYOUT_TBF = 0, /* [n_frames][n_streams][480]: one 10 ms tick of every stream is contiguous */
  CRISPY_RN_LAYOUT_BTF = 1  /* [n_streams][n_frames][480]: one stream's audio is contiguous */
} crispy_rn_layout;

typedef struct crispy_rn crispy_rn;

/* Message for the most recent failure on the calling thread ("" if none). */
const char *crispy_last_error(void);
/* "crispy_hip <version> gfx950" */
const char *crispy_version(void);
/* The ABI this header describes; crispy_abi_version() returns the one the library was built with.
 *   1: rounds 1 - 3.   2: round 4 (crispy_asr_opts 20 -> 44 bytes, crispy_asr_result gained windows, the staged RNNoise
 *   pipeline entry points removed).   3: round 5.   4: round 6 (this header: crispy_asr_transcribe_recording and its
 *   CRISPY_ERR_CANCELLED, the int16 sample transport crispy_rn_process_s16*).   5: word-level timestamps
 *   (crispy_asr_opts::dtw_token_timestamps / dtw_heads / n_dtw_heads, crispy_asr_result::token_t_dtw / n_words / words,
 *   crispy_asr_word, crispy_asr_align_device, crispy_asr_dtw_device).   6: the capture-rate adapter on the device
 *   (crispy_rn_adapter_*, crispy_rn_push*, crispy_linear_resampler_count). */
#define CRISPY_ABI_VERSION 6
int crispy_abi_version(void);
/* Number of usable gfx950 devices (0 when there is none; never fails). */
int crispy_device_count(void);
/* Self-test of the boundary's exception guard: every entry point is a function-try-block, so a C++ exception
 * (std::bad_alloc from a std::vector, std::system_error from a std::thread ...) becomes a status code and a
 * crispy_last_error() message instead of unwinding into a panic=abort host.  kind: 0 nothing, 1 std::bad_alloc,
 * 2 std::length_error, 3 std::runtime_error, 4 a non-standard exception, 5 a real failing std::vector::resize.
 * Returns what the guard made of it (CRISPY_ERR_OOM for 1, 2, 5; CRISPY_ERR_HIP for 3, 4; CRISPY_OK for 0). */
int crispy_selftest_exception_guard(int kind);

/*
 * DenoiseState::new() for n_streams independent streams (audio.rs:229).
 * weights: flat int8 blob of CRISPY_RN_WEIGHT_BYTES bytes, layer order input_dense, vad_gru,
 * vad_output, noise_gru, denoise_gru, denoise_output; per layer input weights [in][out]
 * (GRU [in][3N], gates z,r,h), recurrent weights [N][3N], bias.  The blob built into
 * nnnoiseless is not redistributable from here, so weights are always explicit.
 * All state starts at zero, as DenoiseState::new() does.
 */
int crispy_rn_create(const int8_t *weights, size_t nbytes, int n_streams, int device,
                     crispy_rn **out);
void crispy_rn_destroy(crispy_rn *h);

/*
 * Weights from an "rnnoise-nu model file version 1" text file -- the format nnnoiseless' RnnModel::from_read
 * parses [UPSTREAM-RECALL] -- so that a host without a weight blob of its own (the reference constructs
 * DenoiseState::new() with the model built into the crate, audio.rs:229; that blob cannot be redistributed from
 * here) can point the library at a model file instead.  crispy_rn_weights_from_file fills `blob`
 * (CRISPY_RN_WEIGHT_BYTES bytes, the layout crispy_rn_create takes) without touching a device; the topology is
 * fixed, so a file whose layer sizes or activation ids differ, that is truncated, or that holds a value outside
 * int8 is CRISPY_ERR_BAD_MODEL.  crispy_rn_create_from_file = parse + crispy_rn_create.
 */
int crispy_rn_weights_from_file(const char *path, int8_t *blob, size_t blob_bytes);
int crispy_rn_create_from_file(const char *path, int n_streams, int device, crispy_rn **out);

/* Fresh DenoiseState for one stream (stream >= 0) or all of them (stream == -1):
 * what audio.rs:955-965 does by replacing the processor. */
int crispy_rn_reset(crispy_rn *h, int stream);

int crispy_rn_n_streams(const crispy_rn *h);

/* Frames each rn_frame_kernel launch covers: a call of n frames is enqueued as ceil(n / this) launches
 * whose high-pass runs one launch ahead on a helper stream (bench.py's per-launch roofline uses it). */
int crispy_rn_frames_per_launch(void);
/* Number of rn_frame_kernel launches one call of n_frames makes: a segment (<= 250 frames) starts with short
 * sub-chunks (3, 4, 5, 7, 10 frames) so that the sequential high-pass of the first one is the only exposed one, then 12
 * (94 MB of high-passed signal at 4096 streams: still in the Infinity Cache when the frame kernel reads it). */
int crispy_rn_n_launches(int n_frames);

/*
 * process_frame for every stream, n_frames consecutive frames each (audio.rs:268).
 * in/out are HOST pointers to n_frames*n_streams*480 floats in `layout`; samples are f32 in
 * int16 range (the x32768 / /32768, clamp, volume and first-frame drop of audio.rs:261-278 stay
 * with the caller; crispy_rn_push below does them on the device).  vad (nullable) receives the value process_frame returns,
 * [n_frames][n_streams].  Copies through a device staging buffer; returns when `out` is complete.
 * Calls above 8 MB are pipelined in pieces of frames: copy-in of piece i+1, the kernels of piece i and
 * copy-out of piece i-1 overlap (the copy-out side on its own host thread, because copies from pageable
 * memory block the calling thread), so a call costs about one direction of PCIe traffic.  Buffers registered
 * with crispy_host_register are copied by DMA without the runtime's staging.
 */
int crispy_rn_process(crispy_rn *h, const float *in, float *out, float *vad, int n_frames,
                      crispy_rn_layout layout);

/*
 * Page-lock (and later release) a host buffer the caller keeps across calls -- the ring buffers of
 * RnnNoiseProcessor (audio.rs:205-207) or a recording the transcriber reads -- so that crispy_rn_process and
 * crispy_asr_transcribe* copy it by DMA.  Thin wrappers over hipHostRegister / hipHostUnregister: a Rust host
 * does not need to link HIP for them.  Optional: unregistered (pageable) buffers work everywhere.
 */
int crispy_host_register(void *p, size_t bytes);
int crispy_host_unregister(void *p);

/*
 * Same, with DEVICE pointers (HBM-resident audio, no PCIe in the call).  Work is enqueued on
 * hip_stream (a hipStream_t, NULL = the handle's own stream) and the call returns without
 * waiting.  taps (nullable) receives CRISPY_RN_TAPS floats per frame and stream
 * [n_frames][n_streams][72]: features[42], gains[22], pitch_index, pitch_gain, vad, silence.
 */
int crispy_rn_process_device(crispy_rn *h, const float *d_in, float *d_out, float *d_vad,
                             float *d_taps, int n_frames, crispy_rn_layout layout,
                             void *hip_stream);

/*
 * Integer sample transport: the same call with int16 PCM in and out -- half the bytes of the f32 form across PCIe, and the
 * formats the reference's capture and recording paths actually hold (cpal i16 / u16 input streams, audio.rs:794-855; the
 * s16 WAV the transcriber reads back, commands/transcription.rs:306-313).
 *   in : sample s enters process_frame as (float)s -- the reference's s as f32 / 32768.0 (audio.rs:814) x 32768.0
 *        (audio.rs:264), both exact;  a u16 stream is the host's (s - 32768) first, as audio.rs:872 does.
 *   out: trunc(clamp(y / 32768, -1, 1) x 32767) for process_frame's output y -- the adapter's / 32768 and clamp
 *        (audio.rs:270-273, volume 1) followed by the WAV writer's quantisation, `(s.clamp(-1.0, 1.0) * 32767.0) as i16`
 *        (recording.rs:109-110), fused into the frame kernel's store.  Bit-exact with crispy_rn_process followed by that
 *        arithmetic on the host (tests/test_gpu_rnnoise.py).
 * State, layouts, vad, the first-frame drop (caller side) and the pipelining of large host calls are those of the f32
 * entry points; one handle may mix f32 and int16 calls.  Device pointers 16-byte aligned.
 */
int crispy_rn_process_s16(crispy_rn *h, const int16_t *in, int16_t *out, float *vad, int n_frames,
                          crispy_rn_layout layout);
int crispy_rn_process_s16_device(crispy_rn *h, const int16_t *d_in, int16_t *d_out, float *d_vad, int n_frames,
                                 crispy_rn_layout layout, void *hip_stream);

/*
 * RnnNoiseProcessor (audio.rs:202-295) for all streams of a handle at once: raw capture samples at any rate in, denoised
 * samples out, every arithmetic step on the device -- the input LinearResampler (audio.rs:73-134), the assembly of
 * 480-sample frames from whatever arrives, x32768, process_frame, /32768, clamp, volume, the dropped first frame.  One
 * crispy_rn_push per capture callback replaces the callback's per-sample push_sample loop.  The streams of a handle share
 * one capture rate and are pushed in lock step (the same n_in for all).  The crispy_rn_process* entry points never touch
 * the adapter's state (carry, resampler, first-frame flag); both share the DenoiseState of the streams.
 *
 * The resampler's position arithmetic is the reference's own f64 recurrence, run once per push on the host for all
 * streams (the positions do not depend on the samples) from the first sample of a stream on; the interpolation, with its
 * separately rounded multiply and add, and everything else run in two streaming kernels around the frame kernels.  Device
 * workspace: 2 x n_streams x frames x 480 floats for the largest push so far, 2 x (n_streams x 481) floats of state.
 */
/* RnnNoiseProcessor::new(input_rate, _, volume) on an existing handle: |input_rate - 48000| >= 1 inserts the
 * LinearResampler(input_rate, 48000); volume is clamped to [0, 1].  Resets the adapter state (carry, resampler,
 * first-frame flag) and the DenoiseState of every stream (what audio.rs:955-965 does by replacing the processor).
 * A handle that was never configured behaves as 48 kHz with volume 1. */
int crispy_rn_adapter_configure(crispy_rn *h, float input_rate, float volume);
int crispy_rn_adapter_set_volume(crispy_rn *h, float volume);          /* NsState::set_volume; holds from the next push on */
/* NsState::produced_rate_hz (audio.rs:352-357): 48000 with the resampler, else the configured rate.  (Through an
 * out-pointer: every entry point returns a status.) */
int crispy_rn_adapter_produced_rate_hz(const crispy_rn *h, float *rate_hz);
/* samples the NEXT push of n_in samples will return per stream (a function of the adapter state), < 0 = error */
long crispy_rn_push_out_len(const crispy_rn *h, long n_in);
/* DEVICE pointers. d_in [n_streams][in_stride], n_in raw capture samples in +-1 per stream (at most 2^24 per push).
 * d_out [n_streams][out_stride] receives *n_out = 480 x (completed frames, minus the dropped first one) samples per stream:
 * clamp(y / 32768, -1, 1) x volume.  d_frames48 (nullable) [n_streams][frames_stride]: the frames exactly as they entered
 * process_frame (48 kHz, x32768), all completed ones including the dropped first.  d_vad (nullable) [frames][n_streams].
 * Enqueued on hip_stream (NULL = own stream); n_out is known on return.  n_in == 0 is a no-op.  CRISPY_ERR_INVALID_ARG:
 * n_in < 0, a stride shorter than its data, NULL d_in / d_out / n_out, d_out overlapping d_in; CRISPY_ERR_OOM: the
 * workspace could not grow -- in both cases the handle's state is as it was. */
int crispy_rn_push_device(crispy_rn *h, const float *d_in, long in_stride, long n_in, float *d_out, long out_stride,
                          float *d_frames48, long frames_stride, float *d_vad, long *n_out, void *hip_stream);
/* the same with HOST pointers; returns when out is complete */
int crispy_rn_push(crispy_rn *h, const float *in, long in_stride, long n_in, float *out, long out_stride,
                   float *vad, long *n_out);
/* With crispy_rn_set_timing: device time of rn_adapt_in_kernel and rn_adapt_out_kernel of the last push that returned
 * samples, from hipEvents around each (tools/rn_push_timing.py). */
int crispy_rn_last_push_ms(crispy_rn *h, float *adapt_in_ms, float *adapt_out_ms);
/* Pure, no device: how many samples a fresh LinearResampler(input_rate, output_rate) emits for its inputs
 * n_before ... n_before + n_in - 1 (audio.rs:108-133; n_in when the rates are within 1 Hz).  Runs the recurrence:
 * time proportional to n_before + n_in.  < 0 = error (negative count, rate not a positive number). */
long crispy_linear_resampler_count(float input_rate, float output_rate, long n_before, long n_in);

/*
 * The playback half of RnnNoiseProcessor: `output_buf`, the deque of at most one second that push_sample appends to
 * (audio.rs:280-285), and next_sample (audio.rs:297-314), the linear-interpolating read at input_rate / output_rate that
 * the output callback makes once per output frame before it converts the sample to the device's format and writes it to
 * every channel (audio.rs:610-657).  One crispy_rn_pull per playback callback, as there is one crispy_rn_push per capture
 * callback; every result is bit for bit that of the per-sample loop.
 *
 * The ring is a device buffer [n_streams][max_output_len] f32 (max_output_len = the effective input rate `as usize`: 48000
 * with the input resampler, else the configured rate), filled by a copy kernel at the end of every push; its head, its
 * length and resample_pos live on the host, the same for every stream.  A pull runs the reference's f64 recurrence on the
 * host, frame by frame (step = input_rate as f64 / output_rate as f64), uploads one (offset, fraction) pair per output frame,
 * and one kernel gathers, interpolates -- s0 + (s1 - s0) * frac, three separately rounded f32 operations --, converts and
 * fans out.  No volume is applied (it was at the push).  Fewer than two samples buffered: the frame is 0.0.
 *
 * A push and a pull on one handle must be ordered by the caller: enqueue both on the same stream, or order the streams
 * with events.  A handle never configured for playback has no ring, its pushes run as before, crispy_rn_pull* on it is
 * CRISPY_ERR_INVALID_ARG and crispy_rn_playback_buffered 0.
 */
#define CRISPY_PCM_F32 0   /* float: the sample */
#define CRISPY_PCM_I16 1   /* int16_t: (s.clamp(-1, 1) * 32767.0) as i16, truncated toward zero */
#define CRISPY_PCM_U16 2   /* uint16_t: ((s.clamp(-1, 1) * 0.5 + 0.5) * 65535.0) as u16; silence is 32767 */
/* (An underrun's 0.0 is converted like any sample.  A NaN converts to integer 0, as Rust's `as` does; a finite input never
 * produces one.) */
/* Sets the output rate (a positive number of Hz), allocates the ring for the handle's current effective input rate, empties
 * it and sets resample_pos = 0.  Touches neither the DenoiseState nor the adapter's carry, resampler or first-frame flag.
 * crispy_rn_adapter_configure on a handle with playback configured is the new processor of audio.rs:955-965 here too: the
 * ring is emptied and sized for the new rate, resample_pos = 0; the output rate stays.  The two may come in either order. */
int crispy_rn_playback_configure(crispy_rn *h, float output_rate);
/* output_buf.len(): samples per stream in the ring (0 on a handle without playback), < 0 = error */
long crispy_rn_playback_buffered(const crispy_rn *h);
/* n_frames calls of next_sample per stream.  DEVICE pointer d_out [n_streams][out_stride] elements of `format`
 * (CRISPY_PCM_*): n_frames x channels valid elements per stream, frame-major, every channel of a frame the same value;
 * nothing else is written.  Rows whose pointer and stride are 16-byte aligned are written with 16-byte stores.  n_live
 * (nullable): how many frames of this pull were real samples and not underrun zeros, known on return.  Enqueued on
 * hip_stream (NULL = own stream).  n_frames == 0 is a no-op.  CRISPY_ERR_INVALID_ARG: playback not configured, n_frames < 0
 * or above 2^24, channels outside 1...8, an unknown format, out_stride < n_frames x channels, NULL h / d_out;
 * CRISPY_ERR_OOM: the position upload buffers could not grow -- in both cases the handle's state is as it was. */
int crispy_rn_pull_device(crispy_rn *h, long n_frames, int channels, int format, void *d_out, long out_stride,
                          long *n_live, void *hip_stream);
/* the same with a HOST pointer; returns when out is complete */
int crispy_rn_pull(crispy_rn *h, long n_frames, int channels, int format, void *out, long out_stride, long *n_live);

/*
 * The recording leg of the live path for all streams of a handle: the 48 kHz recording ring that push_mono_to_buffers
 * appends push_sample's output to (audio.rs:701-726), the app-audio ring of the capture handlers, the recording worker that
 * pops 1152-sample frames from both, keeps them within 50 ms of each other and adds them (commands/recording.rs:196-264),
 * WavWriter::write_samples' quantisation to interleaved s16 (recording.rs:101-118), and the callback's level meter
 * (audio.rs:728-729, 779-781).  Every result is bit for bit that of the per-sample loops.
 *
 * For the RNNoise arm the recording resampler always passes through (produced_rate_hz is within 1 Hz of 48000), so the mic
 * ring receives exactly the bits a push returned: on a handle that records, every crispy_rn_push* that returns samples
 * appends them to the mic ring on the same stream.  There is no entry point for it, and the bytes a push or a pull returns
 * do not change.  Both rings are device buffers [n_streams][cap] f32 with the eviction of audio.rs:719-724 (the oldest
 * sample goes for each one that does not fit; of a block of cap samples or more only the last cap survive).  Heads, lengths,
 * the worker's trims and the frame count live on the host, the same for every stream.
 *
 * Push, app push and drain on one handle must be ordered by the caller: the same stream, or events.  A handle never
 * configured for recording has no rings and pushes as before; app push and drain on it are CRISPY_ERR_INVALID_ARG, the
 * buffered lengths and crispy_rn_record_frames_ready 0.
 */
/* start_recording: allocates both rings with cap = ring_samples (0 = the reference's 48000 * 10; otherwise 2 * 1152 ... 2^28)
 * and empties them; again: empties them and, for another cap, replaces them -- the new ones are allocated before the old
 * ones go, CRISPY_ERR_OOM leaves the handle as it was.  The default is 3.84 MB per stream for the two rings.  Touches
 * neither the DenoiseState, the adapter state nor the playback ring; crispy_rn_adapter_configure (a model switch,
 * audio.rs:955-965) and crispy_rn_reset leave the rings alone. */
int crispy_rn_record_configure(crispy_rn *h, long ring_samples);
/* The app-audio capture handlers (recording.rs:260-369): DEVICE pointer d_in [n_streams][in_stride], n_frames interleaved
 * frames of `channels` (1...8) samples per stream, already at 48 kHz.  Downmix -- 1: the sample; 2: (f0 + f1) / 2.0; more:
 * (0.0 + f0 + f1 + ...) / channels as f32, every add rounded, the division correctly rounded -- and append to the app ring.
 * Enqueued on hip_stream (NULL = own stream).  n_frames == 0 is a no-op.  CRISPY_ERR_INVALID_ARG: recording not configured,
 * n_frames < 0 or above 2^24, channels outside 1...8, in_stride < n_frames x channels, NULL h / d_in: the state is unchanged. */
int crispy_rn_record_app_push_device(crispy_rn *h, const float *d_in, long in_stride, long n_frames, int channels,
                                     void *hip_stream);
/* the same with a HOST pointer; returns when the ring holds the frames */
int crispy_rn_record_app_push(crispy_rn *h, const float *in, long in_stride, long n_frames, int channels);
/* The capture callback's level meter, stateless: per stream sum = 0.0, then sum = sum + mono * mono in sample order over the
 * n_in samples of d_in [n_streams][in_stride] (multiply and add rounded separately), d_rms[stream] = (sum / n_in as f32).sqrt().
 * DEVICE pointers; enqueued on hip_stream (NULL = own stream).  n_in == 0 is a no-op that leaves d_rms untouched; n_in is at
 * most 2^24, so the f32 count is exact.  Needs no recording configured. */
int crispy_rn_level_device(crispy_rn *h, const float *d_in, long in_stride, long n_in, float *d_rms, void *hip_stream);
/* the same with HOST pointers; returns when rms is complete */
int crispy_rn_level(crispy_rn *h, const float *in, long in_stride, long n_in, float *rms);
/* both ring lengths in samples per stream (either pointer may be NULL; 0 on a handle that does not record) */
int crispy_rn_record_buffered(const crispy_rn *h, long *mic, long *app);
/* how many 1152-sample frames a drain without a limit would write now, < 0 = error */
long crispy_rn_record_frames_ready(const crispy_rn *h);
/* The worker loop body (commands/recording.rs:215-264), while the mic ring holds 1152 samples and fewer than max_frames
 * frames are done: align (a ring more than 2400 samples longer than the other loses the excess at its head), pop 1152 mic
 * samples, pop 1152 app samples if there are as many, else take zeros and leave the app ring alone, mixed = mic + app,
 * q = (mixed.clamp(-1, 1) * 32767.0) as i16 (truncated toward zero, a NaN is 0).  DEVICE pointer d_out
 * [n_streams][out_stride] elements of `format`:
 *   CRISPY_PCM_I16  the WAV payload: *n_frames x 1152 x 2 int16_t per stream, L and R equal
 *   CRISPY_PCM_F32  channel 0 as run_transcription reads it back (commands/transcription.rs:306-313): q as f32 / 32768.0,
 *                   *n_frames x 1152 floats per stream -- usable as d_in of crispy_resampler_process_device (scale 1, wav_s16 0)
 * Nothing else is written; rows whose pointer and stride are 16-byte aligned are written with 16-byte stores.  *n_frames is
 * known on return; the work is enqueued on hip_stream (NULL = own stream).  CRISPY_ERR_INVALID_ARG: recording not configured,
 * max_frames < 0, an unknown format, NULL h / d_out / n_frames, out_stride shorter than the elements of this drain;
 * CRISPY_ERR_OOM: the offset upload buffers could not grow -- in both cases the handle's state is as it was. */
int crispy_rn_record_drain_device(crispy_rn *h, long max_frames, int format, void *d_out, long out_stride, long *n_frames,
                                  void *hip_stream);
/* the same with a HOST pointer; returns when out is complete */
int crispy_rn_record_drain(crispy_rn *h, long max_frames, int format, void *out, long out_stride, long *n_frames);
/* Pure, no device: the worker loop above on lengths alone.  Returns the number of frames (< 0 = error: a negative argument).
 * Per frame f (arrays of at least min(max_frames, mic_len / 1152) entries, nullable): mic_off[f] = samples popped from the mic
 * deque before the frame's own 1152, counted from its front at the start; app_off[f] likewise, or -1 for a frame whose app
 * half is zeros.  mic_left / app_left (nullable): the lengths afterwards. */
long crispy_record_worker_plan(long mic_len, long app_len, long max_frames, long *mic_off, long *app_off, long *mic_left,
                               long *app_left);

/*
 * The capture callbacks themselves, for all streams of a handle: build_input_stream_f32 / _i16 / _u16 (audio.rs:732-921) and
 * push_mono_to_buffers (audio.rs:682-730).  One crispy_rn_capture per capture callback is the whole callback, from the
 * device's bytes to the rings; every result is bit for bit that of the per-sample loops.  Three steps, in order, on one stream:
 *   1. mono      per frame of `channels` interleaved samples of `format`: each sample converted -- f32: s; i16:
 *                s as f32 / 32768.0 (audio.rs:817); u16: (s as f32 - 32768.0) / 32768.0 (audio.rs:882) --, then
 *                iter().sum::<f32>() / input_channels as f32: the sum starts from 0.0 and adds in channel order, every add
 *                rounded, the division correctly rounded.  For EVERY channel count: the mic path has no special case for one
 *                or two channels (the app handlers have), so a -0.0 in a mono f32 stream becomes +0.0.
 *   2. level     the callback's level meter over the mono: crispy_rn_level_device.
 *   3. the arm   a property of the handle (crispy_rn_bypass_configure):
 *      RNNoise arm (default, `Some(shared)`): exactly crispy_rn_push_device on the mono -- d_out and *n_out are the push's, the
 *                playback and recording rings are fed as a push feeds them, and every later call on the handle behaves as if
 *                the caller had converted on the host and called crispy_rn_level and crispy_rn_push.
 *      bypass arm (`shared == None`, noise suppression off, audio.rs:545, 697-699): the mono goes through the callback's own
 *                LinearResampler(raw_input_rate, 48000); d_out / *n_out receive the 48 kHz samples it emitted (the `out`
 *                vector of audio.rs:711-714: unscaled, no clamp, no volume); on a handle that records the same samples are
 *                appended to the mic ring with the ring's eviction (audio.rs:716-725).  It is the only arm in which the
 *                recording resampler does not pass through.  Positions are the reference's f64 recurrence, run on the host
 *                and carried across captures; the interpolation last + (sample - last) * t is three separately rounded f32
 *                operations; the last capture sample per stream stays on the device.
 */
/* Enters the bypass arm with a fresh LinearResampler(raw_input_rate, 48000) -- it passes through when the rate is within
 * 1 Hz of 48000 --, or, with 0, leaves it.  Only crispy_rn_capture* consults the arm: crispy_rn_push*, crispy_rn_pull*, the
 * DenoiseState, the adapter's carry and the playback ring are never touched by a bypassed capture, and pushes on a bypassed
 * handle run as before.  crispy_rn_record_configure and crispy_rn_reset leave this resampler alone; every
 * crispy_rn_bypass_configure resets it.  CRISPY_ERR_INVALID_ARG: a negative rate, a NaN, an infinity; CRISPY_ERR_OOM: the
 * state (2 x n_streams floats) could not be allocated -- in both cases the handle is as it was. */
int crispy_rn_bypass_configure(crispy_rn *h, float raw_input_rate);
/* samples the NEXT capture of n_frames frames will return per stream: crispy_rn_push_out_len in the RNNoise arm, the
 * resampler's count in the bypass arm; < 0 = error */
long crispy_rn_capture_out_len(const crispy_rn *h, long n_frames);
/* DEVICE pointers.  d_in [n_streams][in_stride] elements of `format` (CRISPY_PCM_F32 / _I16 / _U16): n_frames interleaved
 * frames of `channels` (1...8) samples per stream, at most 2^24 frames per call.  Rows whose pointer and byte stride are
 * 16-byte aligned and whose frame divides 16 bytes are read with 16-byte loads; the bits do not depend on it.  d_out
 * [n_streams][out_stride] receives *n_out samples per stream (see the arms above; known on return).  d_mono (nullable)
 * [n_streams][mono_stride] receives the n_frames mono samples; without it they go to a workspace of the handle.  d_rms
 * (nullable) [n_streams]: the level meter.  Enqueued on hip_stream (NULL = own stream).  n_frames == 0 is a no-op.
 * CRISPY_ERR_INVALID_ARG: n_frames < 0 or above 2^24, channels outside 1...8, an unknown format, a stride shorter than its
 * data, NULL h / d_in / d_out / n_out, d_out overlapping d_mono, and whatever the push rejects; CRISPY_ERR_OOM: a workspace or
 * an upload buffer could not grow -- in both cases the handle's state is as it was (after CRISPY_ERR_OOM d_mono and d_rms
 * may have been written). */
int crispy_rn_capture_device(crispy_rn *h, const void *d_in, long in_stride, long n_frames, int channels, int format,
                             float *d_out, long out_stride, float *d_mono, long mono_stride, float *d_rms, long *n_out,
                             void *hip_stream);
/* the same with HOST pointers: uploads the raw bytes as they are (an i16 mono microphone is half the bytes crispy_rn_push
 * takes), downloads out and rms (nullable); returns when they are complete */
int crispy_rn_capture(crispy_rn *h, const void *in, long in_stride, long n_frames, int channels, int format, float *out,
                      long out_stride, float *rms, long *n_out);
/* crispy_rn_record_app_push_device for a stream at its own rate (the macOS handler, recording.rs:13-39, 260-369): downmix as
 * there (1: the sample; 2: (f0 + f1) / 2.0; more: the sum from 0.0 / channels), resample_audio(mono, from_rate, 48000) and the
 * ring append in one kernel.  resample_audio is stateless per buffer and a closed form in the reference itself: ratio =
 * from_rate as f64 / 48000 as f64, output_len = ceil(n as f64 / ratio), output i at src_pos = i as f64 * ratio with idx =
 * floor(src_pos), frac = (src_pos - idx) as f32: s[idx] + (s[idx + 1] - s[idx]) * frac (three rounded f32 operations) while
 * idx + 1 < n, s[idx] while idx < n, else nothing.  The discontinuity at buffer boundaries is the reference's.  from_rate ==
 * 48000 is crispy_rn_record_app_push_device.  CRISPY_ERR_INVALID_ARG: what that one rejects, from_rate outside 8000...384000,
 * more than 2^24 resampled samples: the state is unchanged. */
int crispy_rn_record_app_push_at_device(crispy_rn *h, const float *d_in, long in_stride, long n_frames, int channels,
                                        int from_rate, void *hip_stream);
/* the same with a HOST pointer; returns when the ring holds the samples */
int crispy_rn_record_app_push_at(crispy_rn *h, const float *in, long in_stride, long n_frames, int channels, int from_rate);

/*
 * The other variant of NsState, Legacy(SharedAudio) (audio.rs:47-71, 136-200, 317-358), and the model switch of
 * set_monitoring_model (audio.rs:942-967).  A handle is one of three models; the existing calls dispatch on it as NsState's
 * methods do, so a host keeps its one push (or capture) per capture callback and its one pull per playback callback.  A handle
 * whose model was never configured, or is CRISPY_NS_RNNOISE, takes exactly the paths described above.
 *
 * In a Legacy model (SharedAudio; every result bit for bit that of the per-sample loops):
 *   crispy_rn_push*     *n_out = n_in, no first-frame drop: d_out[k] = x * volume, CRISPY_NS_NOISY: + noise * 0.05, where
 *                       rng = rng * 1664525 + 1013904223 (wrapping u32) per sample and noise = (rng as f32 / 2^32) * 2.0 - 1.0
 *                       -- every multiply and add rounded on its own.  The RAW x goes to the playback ring, which holds
 *                       `rate as usize` samples at the raw capture rate.  What was returned goes through the capture callback's
 *                       LinearResampler(rate, 48000) -- the one resampler state that the bypass arm uses, reset by
 *                       crispy_rn_bypass_configure; do not push to a handle while it is bypassed -- and from there to the mic
 *                       ring if the handle records; its positions and last sample advance on every Legacy push whether or
 *                       not it records.  It is reset, as push_mono_to_buffers does (audio.rs:701-709), when the rate produced
 *                       is 1 Hz or more off the rate of the last push that returned samples: RNNoise at 44.1 kHz (produces
 *                       48000) followed by a Legacy model (produces 44100) resets it at the first Legacy sample; dummy <->
 *                       noisy at one rate does not.  d_frames48, d_vad and vad must be NULL.  crispy_rn_push_out_len is n_in,
 *                       crispy_rn_adapter_produced_rate_hz the configured rate.
 *   crispy_rn_pull*     SharedAudio::next_sample: step = raw rate / output rate, s0 + (s1 - s0) * frac, NOISY: + noise * 0.05
 *                       from the same LCG, then * the CURRENT volume (applied at the push and again here, as the reference
 *                       does), conversion and fan-out as above.  A dry frame is 0.0 and advances neither the LCG nor the position.
 *   crispy_rn_capture*  mono, level, then the Legacy push; a configured bypass still wins.
 *   crispy_rn_adapter_configure   a fresh processor of the same Legacy kind at the new rate and volume;
 *   crispy_rn_playback_configure  sizes the ring from the raw rate.
 * The LCG state lives on the host, one for all streams: noise comes in the order of the calls, a Noisy push advances it by
 * n_in, a Noisy pull by *n_live.
 */
#define CRISPY_NS_RNNOISE 0   /* NsState::RnnNoise */
#define CRISPY_NS_DUMMY 1     /* NsState::Legacy, ModelKind::Dummy: "Select suppressor", suppression off */
#define CRISPY_NS_NOISY 2     /* NsState::Legacy, ModelKind::Noisy */
/* set_monitoring_model: a fresh processor of that model at the handle's configured capture rate, its current volume and (if
 * configured) output rate -- also when the model is unchanged.  CRISPY_NS_RNNOISE: exactly crispy_rn_adapter_configure(rate,
 * volume) with the current values.  Legacy: SharedAudio::new -- on a handle with playback the ring is emptied and sized
 * `rate as usize`, resample_pos = 0 --, rng_state = 0x1234abcd.  The recording rings and the callback's resampler stay as
 * they are.  Allocates before it changes anything: CRISPY_ERR_INVALID_ARG (NULL h, an unknown model) and CRISPY_ERR_OOM leave
 * the handle as it was. */
int crispy_rn_model_configure(crispy_rn *h, int model);
/* the handle's model, a CRISPY_NS_*; CRISPY_NS_RNNOISE on a handle never configured */
int crispy_rn_model(const crispy_rn *h, int *model);
/* Pure, no device: SharedAudio's LCG.  Returns the state after n steps from `state` (0 ... 2^32 - 1; a long so that bindings
 * need no unsigned type), < 0 = error: a negative argument, a state out of range.  noise (nullable) receives the n noise
 * values of those steps; without it the call is O(log n): 2^j steps are one affine map, as in the kernels. */
long crispy_ns_noise_state(long state, long n, float *noise);

/* Block until everything enqueued on the handle's own stream has finished. */
int crispy_rn_synchronize(crispy_rn *h);

/*
 * Time the frame kernels of the next crispy_rn_process_device call with hipEvents recorded on
 * the launch stream (bench.py's roofline leg).  After that call and a synchronize,
 * crispy_rn_last_kernel_ms returns the device time of the dominant kernel (rn_frame_kernel) and
 * of the whole enqueue (high-pass + frame + history roll) in milliseconds.
 */
int crispy_rn_set_timing(crispy_rn *h, int enable);
int crispy_rn_last_kernel_ms(crispy_rn *h, float *frame_kernel_ms, float *total_ms);

/* Stage entry point (parity tests): the activation functions of the gain network exactly as the frame kernel
 * evaluates them (201-entry tanh table + interpolation, |x| >= 8 clamps; sigmoid != 0: 0.5 + 0.5 tansig(0.5 x)) on n
 * arbitrary f32 arguments, DEVICE pointers.  Bit-compared with the oracle over every table cell and both clamps. */
int crispy_rn_stage_tansig_device(crispy_rn *h, const float *d_x, float *d_y, size_t n, int sigmoid,
                                  void *hip_stream);

/* Developer aid for parity debugging: copy the per-stage debug capture of stream `stream`
 * for the LAST frame of the most recent call (layout mirrors oracle RNO_DBG_*). */
int crispy_rn_debug_capture(crispy_rn *h, int enable);
int crispy_rn_debug_read(crispy_rn *h, int stream, float *dst, size_t n_floats);

/* ------------------------------------------------------------------------------------------
 * Log-mel front end of the ASR path: whisper.cpp `log_mel_spectrogram`, the first stage of
 * transcribe_rs::SpeechModel::transcribe (managers/transcription.rs:183-185, 213-215).
 * 16 kHz f32 PCM in +-1 -> [n_mel][3000] f32 per clip (the frames the encoder consumes):
 * reflect-pad 200, periodic Hann 400, hop 160, power spectrum, mel filters, log10,
 * clamp to (clip max - 8), (x + 4) / 4.  
 * ------------------------------------------------------------------------------------------ */
#define CRISPY_MEL_FRAMES 3000
#define CRISPY_MEL_BINS 201

typedef struct crispy_mel crispy_mel;

/* filters: [n_mel][201] f32, the mel filter bank whisper.cpp reads from the model file
 * (n_mel = 80, or 128 for large-v3). */
int crispy_mel_create(const float *filters, int n_mel, int device, crispy_mel **out);
void crispy_mel_destroy(crispy_mel *h);

/* HOST pointers: pcm [batch][pcm_stride], n_samples[batch] (1..480000 each, the 30 s chunking of
 * commands/transcription.rs:249-302 stays with the caller), out [batch][n_mel][3000].
 * Returns when `out` is complete. */
int crispy_mel_compute(crispy_mel *h, const float *pcm, long pcm_stride, const int *n_samples,
                       int batch, float *out);

/* DEVICE pcm / outputs (n_samples stays a host array); enqueued on hip_stream (NULL = the handle's
 * stream) without waiting.  d_out [batch][n_mel][3000] and/or d_out_t [batch][3002][n_mel]
 * (frame-major, one zero frame of padding on both sides: the layout the encoder's first
 * convolution consumes); either may be NULL. */
int crispy_mel_compute_device(crispy_mel *h, const float *d_pcm, long pcm_stride,
                              const int *n_samples, int batch, float *d_out, float *d_out_t,
                              void *hip_stream);
/* Clips of any length, as whisper.cpp computes the log-mel of a whole recording ONCE before whisper_full's seek loop:
 * reflect-pad 200 in front, 30 s of zeros + 200 behind, (n + 480000) / 160 frames, one maximum over all of them.
 * DEVICE pcm rows, n_samples[batch] a host array with 1 .. CRISPY_ASR_MAX_SAMPLES each (2 h at 16 kHz: the sample
 * indices stay below 2^31).  The call keeps the un-normalised frames and the maximum of every clip in the handle and
 * writes no window itself: crispy_mel_window_device reads them.  One clip at the cap holds 230 MB (80 mel bins) or
 * 369 MB (128) of frames; on CRISPY_ERR_OOM the handle still holds what it held.  A clip of <= 480000 samples gives
 * the same window bits here as through crispy_mel_compute_device, whatever its neighbours. */
#define CRISPY_ASR_MAX_SAMPLES 115200000
int crispy_mel_compute_long_device(crispy_mel *h, const float *d_pcm, long pcm_stride, const int *n_samples,
                                   int batch, void *hip_stream);
/* 30 s windows of the clips of the LAST crispy_mel_compute_device or crispy_mel_compute_long_device call
 * (whisper_full's seek loop): output k is clip clip_idx[k] starting at mel frame seek[k] (both host arrays), clamped to
 * that clip's maximum - 8, then (x + 4) / 4; frames past the audio are the zero padding.  seek[k] is 0..3000 after
 * crispy_mel_compute[_device] (clips of <= 30 s) and 0 .. n_len_org = 1 + (n - 200) / 160 of the clip after
 * crispy_mel_compute_long_device.  Same output layouts. */
int crispy_mel_window_device(crispy_mel *h, const int *clip_idx, const int *seek, int n, float *d_out,
                             float *d_out_t, void *hip_stream);
int crispy_mel_synchronize(crispy_mel *h);
/* Stage entry point (parity tests): d_y[i] = the float the frame kernel stores for the filter sum d_s[i] (DEVICE, n
 * values): d_s[i] > 1e-10 ? (float) log10(d_s[i]) by the kernel's own series : -10.f.  Enqueued on hip_stream (NULL =
 * the handle's stream) without waiting. */
int crispy_mel_stage_log10_device(crispy_mel *h, const double *d_s, float *d_y, size_t n, void *hip_stream);

/* ------------------------------------------------------------------------------------------
 * Whisper engine: replaces transcribe_rs::whisper_cpp::WhisperEngine behind `SpeechModel`
 *   load        managers/transcription.rs:138-141   WhisperEngine::load(&model_path)
 *   transcribe  managers/transcription.rs:183-185   engine.transcribe(&audio, &TranscribeOptions::default())
 * Architecture: SURVEY.md Appendix B.2 (pre-LN transformer, head dim 64, 1500 audio positions).
 * Round-1 numerics are f32 end to end on the f32-input matrix cores.
 * ------------------------------------------------------------------------------------------ */
typedef struct crispy_asr crispy_asr;

/* The hyper-parameter block of a whisper.cpp model file, minus ftype. */
typedef struct crispy_asr_hparams {
  int n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels;
} crispy_asr_hparams;

/* Model container.  Tensors are set by their model-file names ("encoder.conv1.weight",
 * "decoder.blocks.3.cross_attn.query.bias", ...) as f32 host arrays in PyTorch layout
 * ([out][in], conv [out][in][3]); crispy_asr_finalize checks completeness and builds the fused
 * device layouts.  mel_filters: [n_mels][201]. */
int crispy_asr_create(const crispy_asr_hparams *hp, const float *mel_filters, int device,
                      crispy_asr **out);
int crispy_asr_set_tensor(crispy_asr *h, const char *name, const float *data, size_t n_elems);
int crispy_asr_finalize(crispy_asr *h);
void crispy_asr_free(crispy_asr *h);
int crispy_asr_hparams_get(const crispy_asr *h, crispy_asr_hparams *out);

/* Stage entry points (parity tests): PCM (host, <= 30 s per clip) -> encoder output
 * [batch][1500][n_audio_state] (host), and the device-resident variant that starts from the
 * frame-major padded log-mel produced by crispy_mel_compute_device (d_out_t). */
int crispy_asr_encode(crispy_asr *h, const float *pcm, long pcm_stride, const int *n_samples,
                      int batch, float *out);
int crispy_asr_encode_device(crispy_asr *h, const float *d_mel_t, int batch, float *d_out,
                             void *hip_stream);
int crispy_asr_synchronize(crispy_asr *h);

/* Encoder GEMM operand precision.  0 (default): f32 operands on the f32-input matrix cores -- what the parity tests
 * against the float64 oracle pin to 1e-4.  1: f16 operands with f32 accumulation (weights stored as f16, activations
 * rounded to f16 on the way into LDS) -- the numerics of whisper.cpp's ggml matrix products [UPSTREAM-RECALL], on
 * v_mfma_f32_32x32x16_f16, activations that only feed a matrix product kept in f16, the whole convolution stem and the
 * encoder attention on the f16 matrix cores.  Decoder in this mode: cross K|V and the self-attention K|V cache kept in
 * f16 (as whisper.cpp's kv_self / kv_cross are), logits =
 * f16(LayerNorm(x)) . f16(token embedding)^T with f32 accumulation (whisper.cpp's f16 embedding under ggml's mul_mat),
 * and the projections with no LayerNorm in front of them (attention outputs, the MLP's second product) with f16
 * weights and the activation rounded to f16; the LayerNorm-folded projections (q | k | v, cross q, the MLP's first
 * product), LayerNorm and soft-max stay f32; GELU is ggml's (the f16-indexed table of the tanh form, evaluated on the fly).
 * oracle/whisper_oracle.py: encoder_forward_f16, DecoderCache(f16=True).
 * 2 (opt-in): mode 1 plus ggml's remaining rounding points [UPSTREAM-RECALL]: the decoder's LayerNorm output rounded to
 * f16 in front of q | k | v, cross q and the MLP's first product, which then run against f16 weights (the LayerNorm
 * becomes a launch of its own: three more launches per layer and step); and inside every attention -- encoder, decoder
 * self and cross -- the query rounded to f16 in front of K.q and the soft-max taken in full, normalised, and only then
 * rounded to f16 in front of P.V (the encoder runs a statistics pass over K first; a decode step two more hand-offs
 * between the waves of a row).  Not available for resident quantised models.
 * Oracle: encoder_forward_f16(attn16=True), DecoderCache(f16=True, ln16=True, attn16=True). */
int crispy_asr_set_precision(crispy_asr *h, int mode);

/* The audio context: whisper.cpp's whisper_full_params.audio_ctx (`-ac N`; whisper-rs set_audio_ctx) [UPSTREAM-RECALL:
 * everything said about upstream here is recalled, not checked against its source].  With n, 1 <= n <= n_audio_ctx, every
 * encoder pass of the handle from the next call on runs over the first n of the model's 1500 positions and every decoder
 * cross-attention reads n keys:
 *   - the encoder's input is the 2 n mel frames [seek, seek + 2 n) of the window's log-mel, normalised as without the
 *     setting; conv1 sees its own zero padding at frame 2 n, not the real frame that follows; conv2 yields n rows, rows
 *     0 .. n - 1 of encoder.positional_embedding are added, all layers and ln_post run over n rows.  This is NOT rows
 *     0 .. n - 1 of the full-context output (attention is over n keys);
 *   - crispy_asr_encode writes, and crispy_asr_encode_device's d_out and every d_enc argument of this header carry,
 *     [batch][n][n_audio_state] while the setting is on (wherever a comment says [batch][1500][..] or [batch][n_audio_ctx][..]);
 *   - every decode form attends over n keys: greedy, timestamp-rule, fallback and beam passes, prompts, language detection
 *     (the setting holds for every encoder pass of the handle; whether upstream's first call on a state detects the language
 *     at the full context is not pinned), crispy_asr_token_probs_device and the alignment pass;
 *   - crispy_asr_align_device: F = min(n_frames / 2, n) keys are aligned; n_frames may still be up to 2 * n_audio_ctx, and
 *     d_probs / d_matrix keep their n_audio_ctx leading dimension.  In a transcribe call a window with F < 4 gets no
 *     alignment (times -1, no words), as a window beyond the DTW limits does;
 *   - unchanged: log-mel, the seek loop, timestamp rules, thresholds, the no-speech rule, segment and word times (a key is
 *     still 20 ms).  A timestamp beyond 2 n frames is the model's business, as upstream.
 * n = 0 or n = n_audio_ctx: not set -- the launches and the bits of a handle that never saw this call.  Every n from 1 on is
 * supported, in every precision mode and decode form; the batch contract (a clip's result is its solo result bit for bit)
 * holds at every n.  Switching waits for the handle's stream and drops the captured decode steps; workspaces stay sized for
 * n_audio_ctx.  CRISPY_ERR_INVALID_ARG: n < 0 or n > n_audio_ctx, NULL h; CRISPY_ERR_BAD_MODEL: not finalized.
 * crispy_asr_audio_ctx: the effective value, never 0 (n_audio_ctx while not set). */
int crispy_asr_set_audio_ctx(crispy_asr *h, int n);
int crispy_asr_audio_ctx(const crispy_asr *h, int *n);

/* Stage entry point (parity tests): the last step of the decoder alone -- final LayerNorm and vocabulary projection
 * of d_x [batch][n_text_state] (device, f32) into d_logits [batch][n_vocab] (device, f32), in the current precision
 * mode.  Mode 1: LayerNorm output rounded to f16 against the f16 token embedding, f32 accumulation (ggml's mul_mat
 * over whisper.cpp's f16 `decoder.token_embedding.weight`).  batch <= 512. */
int crispy_asr_stage_logits_device(crispy_asr *h, const float *d_x, int batch, float *d_logits);

/* Greedy decoding (north_star: greedy; the sampling strategy transcribe-rs 0.3.11 selects is
 * unverifiable here).  Token ids listed with first_only = 0 are never
 * emitted; those with first_only = 1 only at the first sampled position (whisper's suppress_blank).
 * Nothing is suppressed until this is called. */
int crispy_asr_set_suppress(crispy_asr *h, const int *ids, int n, int first_only);

/* d_enc: DEVICE encoder output [batch][1500][n_text_state]; prompt: host token ids fed to every
 * clip (<|startoftranscript|>, language, <|transcribe|>, <|notimestamps|>); up to max_new tokens
 * are picked by argmax over f32 logits (ties: lowest id).  tokens_out [batch][max_new] (host),
 * n_out[b] = number of tokens before the first EOT (host, nullable), logits_out (host, nullable)
 * the logit of every pick. */
int crispy_asr_decode_greedy_device(crispy_asr *h, const float *d_enc, int batch, const int *prompt,
                                    int n_prompt, int max_new, int *tokens_out, int *n_out,
                                    float *logits_out);

/* SpeechModel::transcribe up to token ids: PCM (host) -> log-mel -> encoder -> greedy decoder.
 * batch == 0 is the empty-audio no-op of managers/transcription.rs:175-177.  Detokenisation needs
 * the vocabulary of a real model file and stays with the caller in this round. */
/* Same with a per-clip token for prompt position 1 (lang_tokens[batch], host, nullable). */
int crispy_asr_decode_greedy_lang_device(crispy_asr *h, const float *d_enc, int batch, const int *prompt,
                                         int n_prompt, const int *lang_tokens, int max_new,
                                         int *tokens_out, int *n_out, float *logits_out);

/* One decoding window per clip under the timestamp rules (whisper.cpp `whisper_process_logits`, which ports
 * openai-whisper's ApplyTimestampRules): <|notimestamps|> suppressed, timestamps in pairs except before EOT,
 * non-decreasing, first one <= 1.00 s, and a timestamp is forced once the probability mass of all timestamps
 * exceeds the most probable text token.  rules: 0 = whisper.cpp flavour [UPSTREAM-RECALL] (the window also
 * ends at a timestamp within 100 ms of seek_end), 1 = openai / HuggingFace flavour (forced first timestamp,
 * strictly later after a closed pair; pinned by tests/golden/whisper_tiny_ts_golden.npz).  prompt without
 * <|notimestamps|>; seek / seek_end [batch] (host, nullable): window start and audio length in mel frames.
 * tokens_out / tids_out [batch][max_new] (tids: the most probable timestamp token at every step, nullable),
 * n_out[b] = picks up to and including the one that ended the window.  Uses the crispy_asr_set_suppress masks. */
int crispy_asr_decode_timestamps_device(crispy_asr *h, const float *d_enc, int batch, const int *prompt,
                                        int n_prompt, const int *lang_tokens, int rules, const int *seek,
                                        const int *seek_end, int max_new, int *tokens_out, int *tids_out,
                                        int *n_out);

/* Stage entry point (parity tests): one pass of whisper_full's temperature ladder over one window per row -- what the
 * transcribe calls run per window and temperature.  Every row has its own prompt (prompts [rows][prompt_stride],
 * n_prompt[rows]; rows of different length decode in lock step, each bit-identical to the row decoded alone), the
 * suppression masks are whisper.cpp's own (specials never, " " and EOT not first).  u == NULL: greedy at temperature 0.
 * u [max_new][rows] (host doubles in [0, 1)): the sampling pick of whisper_sample_token at `temperature` > 0 -- logits /
 * temperature, std::discrete_distribution with u as its uniform variate.  Outputs [rows][max_new]: tokens, the most
 * probable timestamp token of every step (nullable), the log-probability of every pick (nullable; log-softmax over
 * everything allowed before the probability-mass rule); no_speech_prob_out [rows] (nullable); n_out as above. */
int crispy_asr_decode_window_device(crispy_asr *h, const float *d_enc, int rows, const int *prompts,
                                    const int *n_prompt, int prompt_stride, int rules, const int *seek,
                                    const int *seek_end, int max_new, float temperature, const double *u,
                                    int *tokens_out, int *tids_out, float *plog_out, float *no_speech_prob_out,
                                    int *n_out);

/* whisper.cpp language auto-detection: <|startoftranscript|> alone, arg-max over the language tokens.
 * lang_tokens_out[batch] (host).  English-only vocabularies -> CRISPY_ERR_UNSUPPORTED. */
int crispy_asr_detect_language_device(crispy_asr *h, const float *d_enc, int batch, int *lang_tokens_out);

int crispy_asr_transcribe_tokens(crispy_asr *h, const float *pcm, long pcm_stride,
                                 const int *n_samples, int batch, const int *prompt, int n_prompt,
                                 int max_new, int *tokens_out, int *n_out);

/* WhisperEngine::load(&model_path) (managers/transcription.rs:138-141): parse a whisper.cpp GGML
 * model file (hparams, mel filters, vocabulary, tensors) and build a finalized engine.  f32 / f16 tensors are
 * taken as they are; q4_0 / q4_1 / q5_0 / q5_1 / q8_0 blocks (catalog entries managers/model.rs:99,137) are
 * de-quantised to f32 at load time. */
int crispy_asr_load(const char *model_path, int device, crispy_asr **out);

/* The same, for the quantised files the reference's catalog ships (managers/model.rs:99 whisper-medium-q4_1.bin,
 * :137 ggml-large-v3-q5_0.bin; `size_mb` 492 / 1100 at :101, :139): the 2-D tensors STAY in HBM as the file's ggml
 * blocks (q4_0 / q4_1 / q5_0 / q5_1 / q8_0) and are de-quantised at the point of use -- to f16 operands in front of
 * every matrix product, f32 x gamma for the LayerNorm-folded decode projections -- into one scratch slot the size of the
 * largest layer matrix.  Resident weight bytes ~= file size (+ the token embedding once more as f16 in matrix-core
 * operand order for the logits).  The engine runs in precision mode 1 (whisper.cpp's f16-operand arithmetic); 
 * crispy_asr_set_precision(h, 0) is refused with CRISPY_ERR_UNSUPPORTED.  Results equal those of crispy_asr_load +
 * crispy_asr_set_precision(h, 1) on the same file bit for bit.  Only the matrices the engine consumes as blocks stay
 * quantised (attention and MLP weights, the token embedding); any other quantised tensor is inflated.  A file with no
 * quantised matrix at all (f32 / f16: ggml-small.bin, ggml-large-v3-turbo.bin, managers/model.rs:80,118) loads exactly
 * as crispy_asr_load does -- dense tensors, every precision mode available, crispy_asr_memory_info reports no quantised
 * bytes and no scratch slot.  crispy_asr_encode_device on a caller's stream is ordered against the handle's own stream
 * around the scratch slot (the encode starts after the work enqueued on the handle so far; the handle continues after it). */
int crispy_asr_load_resident(const char *model_path, int device, crispy_asr **out);

/* Device memory held by the model itself (not the per-call workspaces): every weight tensor, fused / folded / f16 copy
 * and resident quantised block (`weight_bytes`), the part of it that is quantised blocks (`quantised_bytes`), and the
 * de-quantisation scratch slot of a resident model (`scratch_bytes`).  Any out-pointer may be NULL. */
int crispy_asr_memory_info(const crispy_asr *h, size_t *weight_bytes, size_t *quantised_bytes, size_t *scratch_bytes);

/* Special-token ids of a whisper.cpp vocabulary of n_vocab entries [UPSTREAM-RECALL: whisper_vocab]: English-only
 * (51864): eot 50256, sot 50257, translate 50357, transcribe 50358, solm 50359, prev 50360, nosp 50361,
 * notimestamps 50362, first timestamp 50363, no language in the prompt; multilingual (51865, 51866 = large-v3):
 * everything one higher, and the tokens behind the language block one more per extra language.  Pure function,
 * no device needed. */
typedef struct crispy_asr_specials {
  int eot, sot, lang0, n_lang, translate, transcribe, solm, prev, nosp, notimestamps, beg, multilingual;
} crispy_asr_specials;
int crispy_asr_vocab_specials(int n_vocab, crispy_asr_specials *out);

/* Language token of an ISO code as whisper.cpp's `whisper_lang_id` table orders them [UPSTREAM-RECALL: g_lang, the
 * order of openai/whisper's LANGUAGES]: "en" -> lang0, "zh" -> lang0 + 1, ... "yue" -> lang0 + 99 (large-v3 only).
 * For hosts that hold the language as a string (`TranscribeOptions.language`); the result goes into
 * crispy_asr_opts::language_token.  English-only vocabularies have no language token: "en" gives 0 (= none),
 * anything else CRISPY_ERR_UNSUPPORTED; an unknown code, or one the vocabulary has no token for, CRISPY_ERR_INVALID_ARG.
 * "auto" and "" give 0 (auto-detect).  Pure function, no device needed. */
int crispy_asr_language_token(int n_vocab, const char *code, int *token_out);

/* Byte string of one vocabulary entry of a loaded model file (not NUL-terminated). */
int crispy_asr_token_text(const crispy_asr *h, int token, const char **text, size_t *len);

/* TranscribeOptions::default() (managers/transcription.rs:184): language unset, transcribe task, and whisper.cpp's
 * whisper_full_default_params(GREEDY) for everything else.  A zeroed struct IS that default: every field reads
 * "0 = whisper.cpp's default". */
typedef struct crispy_asr_opts {
  int language_token;  /* 0 = auto-detect (what TranscribeOptions::default() leaves to whisper.cpp); else the token id */
  int translate;       /* 0 = transcribe */
  int max_new_tokens;  /* 0 = whisper.cpp's per-window limit (n_text_ctx / 2 - 4; n_text_ctx / 2 without timestamps) */
  int no_timestamps;   /* 0 = whisper.cpp's default: timestamp tokens, 30 s windows advancing to the last closed
                          timestamp pair (whisper_full's seek loop), segments in the result.
                          1 = <|notimestamps|> prompt, one window, plain greedy arg-max, no segments, none of the
                          decision logic below. */
  int no_prev_text;    /* 0 = whisper.cpp's behaviour inside one whisper_full call [UPSTREAM-RECALL]: from the second
                          window on the decoder is conditioned on the text so far -- prompt <|startofprev|> + the last
                          <= n_text_ctx / 2 tokens of the previous windows (their timestamp tokens included) + the
                          usual <|startoftranscript|> ...; not when fewer than 5 s of audio are left, and not in a
                          re-decode at a temperature >= 0.5.  1 = every window starts from the bare prompt. */
  /* whisper_full's decision logic [UPSTREAM-RECALL: whisper_full_with_state, whisper_sequence_score].  A window is
   * decoded greedily at `temperature`; if its decoder failed (end of text before any timestamp away from the end of the
   * audio, no end within the token limit while less than half the window was covered, entropy of the last 32 tokens
   * below entropy_thold), or its average log-probability is below logprob_thold while no_speech_prob <
   * no_speech_thold, it is decoded again at temperature + temperature_inc, ... up to 1.0 -- above 0 with `best_of`
   * sampling decoders (std::mt19937(j) + std::discrete_distribution, decoder j seeded j at the start of every call),
   * the best-scoring one that did not fail wins; the last temperature is accepted as it is.  A window whose
   * no_speech_prob > no_speech_thold and whose average log-probability < logprob_thold yields no text. */
  float temperature;     /* first temperature of the ladder (0) */
  float temperature_inc; /* 0 = 0.2; < 0: no fallback (one pass at `temperature`, accepted as it is) */
  float entropy_thold;   /* 0 = 2.4; < 0: never fails on entropy */
  float logprob_thold;   /* 0 = -1.0 */
  float no_speech_thold; /* 0 = 0.6; >= 1: no window is ever dropped as silence */
  int best_of;           /* 0 = 5 */
  /* ---- appended with ABI 3 (zero / NULL = the behaviour before): the other whisper_full parameters a host may set ---- */
  int suppress_nst;      /* whisper_full_params.suppress_nst [UPSTREAM-RECALL]: 1 = the non-speech tokens -- whisper.cpp's list
                            of punctuation runs, brackets and music notes, each looked up in the MODEL'S vocabulary as it
                            stands and with a leading space, plus " -" and " '" -- are never picked.  Needs a model loaded
                            from a file (the vocabulary's text); a model without one has nothing to look up. */
  const int *initial_prompt;   /* whisper_full_params.prompt_tokens: token ids placed in FRONT of the conditioning text of every
                                  chunk of the call (whisper.cpp rotates them in front of prompt_past); the first window's prompt is
                                  then <|startofprev|> + the last <= n_text_ctx / 2 of them + the usual prompt.  The host
                                  tokenises (the reference's engine does: transcribe-rs hands whisper.cpp text).  NULL: none. */
  int n_initial_prompt;
  int carry_context;     /* 1 = whisper_full_params.no_context = false: the conditioning text the previous call on this handle
                            ended with is where this call's first window starts (a recording transcribed chunk by chunk
                            through one engine).  Single-chunk calls only (batch == 1); 0 = whisper.cpp's default
                            (no_context = true: every call starts clean). */
  int beam_size;         /* > 1: whisper.cpp's BEAM_SEARCH strategy [UPSTREAM-RECALL: whisper_full_with_state,
                            whisper_sample_token_topk] -- beam_size decoders per window at temperature 0 (best_of above), every
                            live decoder drawing beam_size candidate ids per step from its distribution, candidates sorted by
                            the sum of their log-probabilities and dealt to the decoders without repeating a sequence.  One
                            host round trip per token.  0 | 1: the GREEDY strategy.  At most 8 (WHISPER_MAX_DECODERS); needs
                            timestamps (no_timestamps = 1 with beam_size > 1: CRISPY_ERR_UNSUPPORTED). */
  /* ---- appended with ABI 5 (zero / NULL = the behaviour before): word-level timestamps ---- */
  int dtw_token_timestamps;  /* 1 = token and word start times from cross-attention alignment: openai-whisper's
                                word_timestamps=True (timing.py: find_alignment, add_word_timestamps), whisper.cpp's
                                dtw_token_timestamps [UPSTREAM-RECALL].  Per kept window one teacher-forced decoder pass over
                                sot sequence + <|notimestamps|> + the window's text tokens + <|endoftext|> (the previous-text
                                prompt is not part of it), the soft-maxed cross-attention of the alignment heads over the
                                window's n_frames / 2 keys, standardised per frame over the tokens, a width-7 median filter
                                along the frames, the mean over the heads, dynamic time warping on minus that matrix; each
                                token starts where the warping path enters its row (crispy_asr_result::token_t_dtw, words).
                                The diarization path gives each word to a speaker by its midpoint (managers/diarization.rs:
                                656-700, format_diarized_text) from transcribe_with_timestamps (managers/transcription.rs:
                                200-249).  Segments, tokens, text and windows are the same with or without it.  Needs
                                timestamps (no_timestamps = 1: CRISPY_ERR_UNSUPPORTED). */
  const int *dtw_heads;      /* the alignment heads as (layer, head) pairs, n_dtw_heads of them (a model's own
                                `alignment_heads`; the host passes them, the library has no per-model table).  NULL: every
                                head of the last n_text_layer - n_text_layer / 2 decoder layers (openai's default mask). */
  int n_dtw_heads;
} crispy_asr_opts;

/* One segment of the result (managers/transcription.rs:223-233: `seg.start`, `seg.end`, `seg.text`),
 * seconds relative to the start of the chunk. */
typedef struct crispy_asr_segment {
  float t0, t1;
  const char *text;    /* UTF-8, NUL-terminated, untrimmed */
} crispy_asr_segment;

/* What whisper_full decided about one window of the seek loop (timestamp mode only). */
typedef struct crispy_asr_window {
  int seek;              /* window start, mel frames (10 ms) from the start of the chunk */
  int seek_advance;      /* frames the loop moved on by */
  int n_tokens;          /* tokens of this window that went into the result (0 when dropped) */
  int decoder;           /* which of the best_of decoders won (0 at temperature 0) */
  int failed;            /* 1 = the decoder failed and was accepted all the same (last temperature of the ladder) */
  int no_speech;         /* 1 = dropped by the no-speech rule */
  float temperature;     /* the temperature the accepted pass ran at */
  float no_speech_prob;  /* softmax of the last prompt position's unfiltered logits at <|nospeech|> (whisper.cpp takes it
                            there: the prompt pass yields the logits of its last position only) */
  float avg_logprob;     /* mean log-probability of the kept tokens (-inf for a decoder that failed before scoring) */
  float entropy;         /* entropy of the token histogram of the last 32 kept tokens */
} crispy_asr_window;

/* One word of the result (opts.dtw_token_timestamps): openai's split_tokens_on_spaces (split_tokens_on_unicode only for
 * zh / ja / th / lo / my / yue) and merge_punctuations with its default sets.  t0 = the alignment entry time of its first
 * token, t1 = that of the token after its last (the window's <|endoftext|> closes the last word); a punctuation mark
 * merged into a neighbour leaves the neighbour's times as they were (openai's order).  Seconds from the start of the
 * chunk, as segments are. */
typedef struct crispy_asr_word {
  float t0, t1;
  const char *text;    /* UTF-8, NUL-terminated, with its leading space */
  int first_token;     /* index into crispy_asr_result::tokens */
  int n_tokens;        /* tokens of the word (timestamp tokens never are) */
} crispy_asr_word;

/* Library-owned result of one transcribe call; release with crispy_asr_free_result. */
typedef struct crispy_asr_result {
  const char *text;    /* UTF-8, NUL-terminated, untrimmed (the caller trims: transcription.rs:187) */
  const int *tokens;   /* the kept token ids (timestamp tokens included in timestamp mode), without <|endoftext|> */
  int n_tokens;
  int language_token;  /* the language token used (detected or given); 0 for English-only vocabularies */
  int n_segments;      /* 0 with no_timestamps (the reference then falls back to one segment, transcription.rs:236-249) */
  const crispy_asr_segment *segments;
  int n_windows;       /* windows of the seek loop, in order (0 with no_timestamps) */
  const crispy_asr_window *windows;
  /* ---- appended with ABI 5: word-level timestamps (NULL / 0 unless opts.dtw_token_timestamps) ---- */
  const float *token_t_dtw;  /* [n_tokens], parallel to tokens: start time of a text token in seconds from the start of the
                                chunk (window seek x 0.01 + its alignment entry time); -1 for timestamp tokens */
  int n_words;
  const void *words;         /* crispy_asr_word[n_words], in order (typed `const void *` so that the struct stays within the
                                scalar / pointer field types every binding of this header mirrors) */
} crispy_asr_result;

/* engine.transcribe(&audio, &TranscribeOptions::default()) for ONE recording of any length up to
 * CRISPY_ASR_MAX_SAMPLES (16 kHz f32, host): ONE whisper_full over all of it -- the log-mel of the whole recording with
 * one maximum, then 30 s windows that advance to the last closed timestamp pair and carry the text so far; what
 * whisper.cpp does with audio of more than 30 s, and NOT the hard 30 s cuts of crispy_asr_transcribe_recording below.
 * Language detection and the first window's no-speech probability see the first 30 s, as upstream.  With
 * opts->no_timestamps (one window by definition) more than 480000 samples are CRISPY_ERR_UNSUPPORTED.  n == 0 returns an empty result (transcription.rs:175-177), and so does a chunk of fewer than
 * 10 mel frames (100 ms; the frame count is 1 + (n - 200) / 160, i.e. 2999 for a full chunk): whisper.cpp's whisper_full
 * refuses it and yields no segments [UPSTREAM-RECALL: delta_min, n_len_org].  Needs a model
 * loaded from a file (vocabulary) for text; tokens are always returned.  opts == NULL is
 * TranscribeOptions::default(): language auto-detected, transcribe, timestamps on. */
int crispy_asr_transcribe(crispy_asr *h, const float *pcm16k, size_t n, const crispy_asr_opts *opts,
                          crispy_asr_result **out);
/* The same for `batch` clips at once (pcm[i]: host pointer to n[i] <= CRISPY_ASR_MAX_SAMPLES samples, n[i] == 0 allowed;
 * lengths may be mixed, a clip that has run out of audio leaves the lock step):
 * one log-mel + encoder + language-detection + decoder pass over all clips (more than 512: in turns of 512).  results[batch]
 * receives one library-owned result per clip (free each); on failure every results[i] is NULL.  A clip's result is the result
 * of crispy_asr_transcribe on it alone, bit for bit, whatever the batch (every precision mode, every model width). */
int crispy_asr_transcribe_batch(crispy_asr *h, const float *const *pcm, const size_t *n, int batch,
                                const crispy_asr_opts *opts, crispy_asr_result **results);
void crispy_asr_free_result(crispy_asr_result *r);

/* `run_transcription`'s chunk loop (commands/transcription.rs:249-302, 363-400, 468) for a whole recording already at
 * 16 kHz: n samples are cut into 480 000-sample chunks (the last, partial one passed as it is), every chunk goes through
 * engine.transcribe(&chunk, opts), the chunk texts are trimmed (Rust's str::trim: Unicode white space), the non-blank ones
 * joined with ONE space -> result.text.  Where the reference's loop is serial (one chunk per engine call), the chunks here
 * are decoded in groups of `max_batch` (0 = 128) by one crispy_asr_transcribe_batch each -- they are independent:
 * TranscribeOptions::default() carries no context between chunks -- and the text is byte for byte what the chunk-by-chunk
 * loop gives (tests/test_gpu_recording.py).  Also in the result: the tokens of all chunks, the segments with their times
 * shifted by the chunk's start (chunk index x 30 s: `chunk_start_seconds`), the windows with `seek` shifted by 3000
 * frames per chunk; language_token = the first chunk's.
 *   cancel_flag (nullable): polled before every group and between the windows of the seek loop, as the reference polls its
 *     AtomicBool before every chunk (:251, :359, :402); once it reads non-zero the call returns CRISPY_ERR_CANCELLED and no
 *     result (the reference returns without saving anything).  The host sets it from another thread.
 *   progress (nullable): called on the calling thread after every group with (samples done, n, progress_user) -- what the
 *     reference turns into its "transcription-progress" event (:285-299).  It must not call into this handle.
 * n == 0: an empty result (:190-194).  opts->carry_context is refused (a single-chunk option). */
/* With opts.dtw_token_timestamps the words and token times of every chunk are shifted by its start like the segments. */
typedef void (*crispy_asr_progress_fn)(size_t samples_done, size_t samples_total, void *user);
int crispy_asr_transcribe_recording(crispy_asr *h, const float *pcm16k, size_t n, const crispy_asr_opts *opts,
                                    int max_batch, const volatile int *cancel_flag, crispy_asr_progress_fn progress,
                                    void *progress_user, crispy_asr_result **out);
/* crispy_asr_transcribe (ONE whisper_full over the whole audio, any length) with the same two hooks, as whisper.cpp's
 * whisper_full has them [UPSTREAM-RECALL: whisper_full_params abort_callback / progress_callback]: cancel_flag is polled
 * before every window of the seek loop (non-zero: CRISPY_ERR_CANCELLED, no result), progress is called on the calling
 * thread after every window with (samples behind the seek position, n, progress_user) and once more with (n, n) when the
 * audio is used up.  Both nullable; with both NULL this is crispy_asr_transcribe. */
int crispy_asr_transcribe_hooks(crispy_asr *h, const float *pcm16k, size_t n, const crispy_asr_opts *opts,
                                const volatile int *cancel_flag, crispy_asr_progress_fn progress, void *progress_user,
                                crispy_asr_result **out);

/* Stage entry points of the word-level alignment (crispy_asr_opts::dtw_token_timestamps), for tests and profiling.
 *   crispy_asr_align_device: one teacher-forced decoder pass and the alignment matrix of `batch` clips.
 *     d_enc       device, the encoder output of the clips [batch][n_audio_ctx][n_audio_state] (crispy_asr_encode_device)
 *     tokens      host [batch][ld_tokens]: clip b's first n_tokens[b] ids are its token rows -- the sot sequence (n_sot ids:
 *                 1, or 3 with a multilingual vocabulary), <|notimestamps|>, the text tokens, <|endoftext|>; at most
 *                 n_text_ctx, and n_tokens[b] >= n_sot + 2
 *     n_frames    host [batch]: mel frames of each clip's window, 8 ... 2 * n_audio_ctx; F = n_frames / 2 keys are used
 *     heads       host (layer, head) pairs, n_heads of them; NULL = the default of crispy_asr_opts::dtw_heads
 *     d_probs     (nullable) device f32 [batch][n_heads][ld_tokens][n_audio_ctx]: softmax(q.K^T / 8) over the first F keys
 *                 of every head, columns >= F and rows >= n_tokens[b] left as they were
 *     d_matrix    (nullable) device f32 [batch][ld_tokens][n_audio_ctx]: the standardised, median-filtered, head-averaged
 *                 matrix of ALL token rows (the DTW takes rows n_sot ... n_tokens[b] - 2)
 *     jump_times  (nullable) host f32 [batch][ld_tokens]: entries 0 ... n_tokens[b] - n_sot - 2 -- seconds into the window at
 *                 which the warping path enters each row of the cropped matrix (<|notimestamps|>, then the text tokens)
 *   Operands as the decoder's own cross-attention in the current precision mode (mode 0: f32 q and K; 1: f32 q, f16 K;
 *   2: q rounded to f16 too).  A clip's outputs do not depend on the other clips of the batch.
 *   crispy_asr_dtw_device: dynamic time warping (openai's dtw_cpu, ties: diagonal only when strictly below both, up only
 *     when strictly below both, else left) of a caller's device cost matrix d_x [n_rows][ld] (n_cols <= ld used), f32
 *     costs.  The path from (0, 0) to (n_rows - 1, n_cols - 1): text_idx / time_idx host [n_rows + n_cols], *n_path of
 *     them.  n_rows <= 512, n_cols <= 4096 and n_rows x ceil(n_cols / 16) <= 35 000 (the trace lives in LDS at 2 bits
 *     per cell, beside the last two anti-diagonals and the path's row entries: 226 rows x 1500 columns take 83 KB).
 *     In the seek loop a window beyond these limits (possible only with max_new_tokens above ~370) gets no alignment:
 *     its token times are -1 and it has no words. */
int crispy_asr_align_device(crispy_asr *h, const float *d_enc, int batch, const int *tokens, const int *n_tokens, int ld_tokens,
                            int n_sot, const int *n_frames, const int *heads, int n_heads, float *d_probs, float *d_matrix,
                            float *jump_times);
int crispy_asr_dtw_device(crispy_asr *h, const float *d_x, int n_rows, int n_cols, long ld, int *text_idx, int *time_idx,
                          int *n_path);

/* Confidence: how sure the model was of a token, a word, the detected language.  New entry points only -- no public struct
 * grew, CRISPY_ABI_VERSION is unchanged: a switch on the handle and accessors on the library-owned result.
 *   crispy_asr_set_confidence(h, on): default 0; holds from the next transcribe call on.  It gates the two things that
 *     cost device work: the language distribution of the auto-detection, and the teacher-forced token / word
 *     probabilities of a call with opts.dtw_token_timestamps (the alignment pass then also projects its rows onto the
 *     vocabulary; a scratch of 512 logits rows, 106 MB, is made the first time and kept).  Off: a call runs the launches it
 *     ran before this switch existed and gives the same results.
 *   crispy_asr_result_token_probs: *n = n_tokens entries each, parallel to result->tokens, owned by the result.
 *     plog      the log-probability of the token under the distribution it was picked from (whisper.cpp's
 *               whisper_token_data::plog), for the decoder whisper_full accepted for the window -- greedy, temperature ladder
 *               or beam.  Present in timestamp mode whatever the switch (it is computed anyway): the addends of the window's
 *               avg_logprob (which also counts a kept <|endoftext|>, never part of tokens).  With opts.no_timestamps the
 *               plain arg-max takes no log-soft-max: *plog = NULL, *n = 0.
 *     p_forced  openai-whisper's text_token_probs [UPSTREAM-RECALL: timing.py find_alignment]: the probability of the token
 *               in the teacher-forced alignment pass (sot sequence, <|notimestamps|>, the window's text), soft-max over the
 *               ids below <|endoftext|> of the unfiltered logits; -1 for timestamp tokens and for a window that got no
 *               alignment, as token_t_dtw.  NULL unless the switch was on and the call had dtw_token_timestamps.
 *   crispy_asr_result_word_probs: *n = n_words entries parallel to result->words: the mean of p_forced over the word's
 *     tokens as split, BEFORE merge_punctuations -- a word that absorbed a punctuation mark keeps its own probability, as
 *     it keeps its times (openai's order).  NULL / 0 under the conditions of p_forced.
 *   crispy_asr_result_language_probs: whisper.cpp's lang_probs [UPSTREAM-RECALL: whisper_lang_auto_detect] -- the soft-max
 *     of the detection logits over the language tokens only; entry i belongs to token lang0 + i (crispy_asr_vocab_specials).
 *     *n_lang = 99, 100 for large-v3's vocabulary; NULL / 0 when the switch was off, the language was given in the options,
 *     or the vocabulary is English-only.  crispy_asr_transcribe_recording: the first chunk's, as language_token.
 *   The accessors need no device; a NULL result or out-pointer is CRISPY_ERR_INVALID_ARG.  The arrays live as long as the
 *   result; NULL always means "not computed in this call" (an array that is present but empty -- a call that kept no token --
 *   is a non-NULL pointer with a count of 0).  crispy_asr_transcribe_batch's
 *   "a clip's result is that of the call on it alone, bit for bit" covers all of these numbers. */
int crispy_asr_set_confidence(crispy_asr *h, int on);
int crispy_asr_result_token_probs(const crispy_asr_result *r, const float **plog, const float **p_forced, int *n);
int crispy_asr_result_word_probs(const crispy_asr_result *r, const float **prob, int *n);
int crispy_asr_result_language_probs(const crispy_asr_result *r, const float **probs, int *n_lang);
/* Stage entry points of the above (no switch needed), for tests and profiling.
 *   crispy_asr_detect_language_probs_device: crispy_asr_detect_language_device plus the distribution, probs_out host
 *     [batch][n_lang].  An English-only vocabulary has n_lang = 0: nothing runs, the tokens are 0, the status is OK.
 *   crispy_asr_token_probs_device: the teacher-forced pass of crispy_asr_align_device -- the same `tokens` rows (sot
 *     sequence, <|notimestamps|>, text, <|endoftext|>), limits and left padding; at most 512 clips -- with every row projected
 *     onto the vocabulary as a decode step projects it, in the current precision mode.  logp_out host [batch][ld_tokens]:
 *     entry i = the LOG-probability of tokens[n_sot + 1 + i] given the rows before it, i = 0 ... n_tokens[b] - n_sot - 3,
 *     soft-max over the ids below <|endoftext|> (the text tokens must be such ids).  The exponential is taken only where a
 *     probability is published, so a probability that underflows still has a finite logarithm here.  A clip's numbers do
 *     not depend on the other clips of the batch. */
int crispy_asr_detect_language_probs_device(crispy_asr *h, const float *d_enc, int batch, int *lang_tokens_out, float *probs_out);
int crispy_asr_token_probs_device(crispy_asr *h, const float *d_enc, int batch, const int *tokens, const int *n_tokens,
                                  int ld_tokens, int n_sot, float *logp_out);

/* ------------------------------------------------------------------------------------------
 * 48 kHz -> 16 kHz resampler between the denoiser and the ASR front end:
 * rubato FftFixedIn::<f32>::new(48000, 16000, 1024, 1, 1) as driven by
 * commands/transcription.rs:198-208, 314-357 (1024-sample chunks, last one zero-padded, the tail
 * shorter than one 1026-sample FFT block is never flushed), optionally preceded by the s16 WAV
 * hand-off of recording.rs:101-118 / commands/transcription.rs:306-313.
 * ------------------------------------------------------------------------------------------ */
typedef struct crispy_resampler crispy_resampler;
int crispy_resampler_create(int device, crispy_resampler **out);
void crispy_resampler_destroy(crispy_resampler *h);
/* 16 kHz samples produced for n_in 48 kHz samples: floor(ceil(n_in/1024)*1024 / 1026) * 342. */
long crispy_resampler_out_len(long n_in);
/* DEVICE pointers: d_in [batch][in_stride] (n_in valid samples each), d_out [batch][out_stride].
 * Every input sample is multiplied by `scale` first (1/32768 after the denoiser).  wav_s16: 0 = nothing
 * else, 1 = clamp(-1,1) (audio.rs:272), 2 = clamp, x32767 truncated to s16, /32768 (the WAV hand-off).
 * A NaN sample is treated as the reference treats it: mode 2 reads it as 0 (Rust's `as i16`), modes 0 and 1 keep it
 * (f32::clamp), and it makes NaN of the 684 outputs its 1026-sample block feeds (its own 342 and the next block's 342).
 * Enqueued on hip_stream (NULL = own stream). */
int crispy_resampler_process_device(crispy_resampler *h, const float *d_in, long in_stride, long n_in,
                                    int batch, float scale, int wav_s16, float *d_out,
                                    long out_stride, void *hip_stream);
int crispy_resampler_synchronize(crispy_resampler *h);

/* ------------------------------------------------------------------------------------------
 * Speaker clustering and diarized text: src-tauri/src/managers/diarization.rs:276-724 from "embeddings + chunk times"
 * on -- nme_sc (cosine_similarity, pruned_normalized_laplacian, max_eigengap, kmeans), the relabel / sort / merge tail of
 * run_diarization, find_speaker_at_time and format_diarized_text.  No neural network: the segmentation and embedding
 * models stay with the host, which hands over one embedding row per speech chunk.
 *
 * The handle is a `void *` (as crispy_asr_result::words is): the set of opaque types every binding mirrors is closed.
 * It owns a stream and a scratch that grows on demand and is kept; it is not re-entrant.
 *
 * Device work of crispy_diar_cluster for a recording of n > 2 chunks (p_max = min(n-1, 2*max(floor(sqrt(n)), 2)),
 * kmax = min(max(max_speakers, 1), n-1)):
 *   affinity     f32, each pair's dot / norms summed in index order over dim without fused multiply-adds, correctly
 *                rounded division and square root: bit for bit cosine_similarity.
 *   ranking      rank[i][j] = neighbours of row i that a stable descending sort puts before j (ties: lower index
 *                first), once per recording; "j is among the p largest of row i or i among those of row j" is then
 *                min(rank[i][j], rank[j][i]) < p for every p of the sweep.
 *   Laplacians   all p = 1 ... p_max side by side, bit for bit pruned_normalized_laplacian.
 *   eigenvalues  cyclic Jacobi in the round-robin ordering (floor(n/2) disjoint rotations per step, every 2x2 block of a
 *                step updated independently), all Laplacians of all recordings of a call side by side, in one of two
 *                forms chosen by n alone:  n <= 192: one workgroup per matrix, the matrix in LDS (147 KB of the 160);
 *                193 ... 2048: the matrix in global memory, one launch pair per rotation set for all matrices.
 *                The off-diagonal norm is tested before every sweep (squares summed in double, so no scale of the
 *                matrix overflows or underflows the test); once it is <= n * 2^-24 * the diagonal's norm the
 *                matrix gets one last sweep (the convergence is quadratic: that sweep leaves rounding only) and is
 *                done.  40 sweeps without passing the test fail the call with CRISPY_ERR_INTERNAL.  Rotations are
 *                worked out in double and applied in f32.  A matrix's result does not depend on what else is in
 *                the launch.
 *   decision     max_eigengap over the kmax + 1 smallest eigenvalues (first maximum), ratio = (p/n) / max(gap, 1e-6)
 *                in f32, the first smallest ratio gives p* and k; k <= 1: all labels 0 and no second solve.
 *   vectors      one more solve at p* with the rotations accumulated, the k vectors of the smallest eigenvalues,
 *                rows normalised when their norm is > 1e-9.
 *   k-means      one workgroup per recording: farthest-point seeding from point 0, at most 50 Lloyd iterations, sums in
 *                point order, strict comparisons, empty clusters keep their centre.
 * Scratch: recordings are taken in turns whose device scratch stays below 2 GB; per recording n*n*(4+2+2) bytes for the
 * affinity and the rankings plus 4*n*n per Laplacian of the sweep (n = 2048: 91 Laplacians, 1.6 GB; n = 300: 13 MB).
 *
 * Limits: 0 <= n[i] <= 2048, 1 <= dim <= 1024, 1 <= batch <= 64; max_speakers < 1 counts as 1 (:292, :550);
 * n[i] <= 2 gives zeros (:367, :547).  A non-finite embedding value is CRISPY_ERR_INVALID_ARG (the reference's
 * partial_cmp(..).unwrap_or(Equal) leaves the order of NaNs unspecified).  Limits are checked before any launch.
 * A recording's labels and info are the same bytes alone and in any batch.
 * ------------------------------------------------------------------------------------------ */
typedef struct crispy_diar_info {
  int p_star;   /* the pruning parameter that minimised the ratio (0 for n <= 2) */
  int k;        /* speakers: clamp(eigengap position, 1, kmax) (1 for n <= 2, 0 for n == 0) */
  float ratio;  /* (p_star / n) / max(gap, 1e-6) */
  float gap;    /* the largest eigengap at p_star */
  int p_max;    /* p ran over 1 ... p_max (0 for n <= 2) */
} crispy_diar_info;

int crispy_diar_create(int device, void **out);
void crispy_diar_destroy(void *h);
/* nme_sc for `batch` recordings.  emb: host f32, the recordings' rows concatenated [sum n][dim]; n: host [batch];
 * labels: host [sum n], the raw nme_sc labels (not yet in order of appearance: crispy_diar_speaker_segments does that);
 * info: nullable, crispy_diar_info[batch].  Returns when the labels are there. */
int crispy_diar_cluster(void *h, const float *emb, const int *n, int batch, int dim, int max_speakers, int *labels, void *info);
/* The same with d_emb and d_labels on the device (n and info stay host arrays); the work is enqueued on hip_stream
 * (NULL = the handle's own) and the call returns after it is complete -- the solver reads its convergence flags back. */
int crispy_diar_cluster_device(void *h, const float *d_emb, const int *n, int batch, int dim, int max_speakers, int *d_labels,
                               void *info, void *hip_stream);
/* Stage entry points, for tests and profiling; device pointers, the handle's stream, complete on return.
 *   affinity   d_emb [n][dim] -> d_aff [n][n] (zero diagonal); 1 <= n <= 2048, 1 <= dim <= 1024
 *   laplacian  d_aff [n][n] (symmetric, as affinity writes it) and p >= 1 -> d_lap [n][n]
 *   eigh       n_mats symmetric f32 matrices d_mats [n_mats][n][n] (left as they are) -> d_evals [n_mats][n] ascending and,
 *              unless d_evecs is NULL, d_evecs [n_mats][n][n]: column c of a matrix belongs to its eigenvalue c.
 *              1 <= n <= 2048, n_mats >= 1, n_mats * n * n * 4 bytes (x 2 with vectors) <= 2 GB.  Any finite entries:
 *              the convergence test sums its squares in double, so it reads the same at every scale.  The eigenvalues
 *              are within n * 2^-24 * |A|_2 where that bound is a normal f32 (|A|_2 above about 1e-30 / n) and |A|_2 * n
 *              stays below the f32 maximum; a NaN or infinite entry ends in CRISPY_ERR_INTERNAL after the 40 sweeps.
 *   decide     the decision of crispy_diar_cluster on given eigenvalues: d_evals [p_max][n], row p - 1 the ascending
 *              eigenvalues at p (read as they are: nothing is sorted here) -> *info (host, one crispy_diar_info).
 *              0 <= n <= 2048, 0 <= p_max <= 2048, kmax from max_speakers as above; n <= 2 or p_max == 0 gives the
 *              zero info (k = 1, or 0 for n == 0) without a launch.
 *   kmeans     the spectral rows and k-means of crispy_diar_cluster on given vectors: d_vecs [n][n], of which the first
 *              k columns are read -> d_labels [n]; d_points [n][k] (the rows, normalised where their norm is > 1e-9) and
 *              d_centers [k][k] (the final centres) are nullable.  0 <= n <= 2048 (0 writes nothing), k >= 1; k == 1
 *              gives zeros and k >= n gives 0 ... n-1 (kmeans, :476-481), and neither reads d_vecs or writes points
 *              or centres.
 *   decide and kmeans launch the kernels of crispy_diar_cluster themselves, on one recording. */
int crispy_diar_affinity_device(void *h, const float *d_emb, int n, int dim, float *d_aff);
int crispy_diar_laplacian_device(void *h, const float *d_aff, int n, int p, float *d_lap);
int crispy_diar_eigh_device(void *h, const float *d_mats, int n, int n_mats, float *d_evals, float *d_evecs);
int crispy_diar_decide_device(void *h, const float *d_evals, int n, int p_max, int max_speakers, void *info);
int crispy_diar_kmeans_device(void *h, const float *d_vecs, int n, int k, int *d_labels, float *d_points, float *d_centers);

/* Host functions: no device, no handle.  Speakers are numbers: s >= 1 is "Speaker s", 0 is "Speaker ?".
 *   crispy_diar_chunk_plan: run_diarization's split of speech segments into ~4 s chunks (:311-338).  Segment i spans
 *     start[i] ... end[i] seconds and holds n_samples[i] samples; a segment longer than 4 s becomes ceil(dur / 4) chunks of
 *     n_samples / chunks samples (the last takes the rest).  Chunk c is out_start / out_end[c] seconds and the samples
 *     out_first[c] ... out_first[c] + out_len[c] of its segment out_segment[c].  Returns the number of chunks; entries
 *     beyond `cap` are not written (call with cap 0 to size).  Non-finite times or sample_rate <= 0: INVALID_ARG.
 *   crispy_diar_speaker_segments: :373-400 -- labels renumbered in order of first appearance (the first to speak is
 *     Speaker 1), a stable sort by start, then merge_consecutive_segments: same speaker and max(start - last.end, 0) <=
 *     merge_gap extends the last segment to max(end, last.end).  Returns the number of merged segments (cap as above).
 *   crispy_diar_find_speaker: find_speaker_at_time (:703-724) -- the first segment with start <= time <= end, else the
 *     segment at the smallest distance (first of equals), 0 for an empty list; a negative status for NULL segments.
 *   crispy_diar_format_text: format_diarized_text (:657-700), byte for byte.  Words (t0, t1, text) whose text is blank
 *     after Rust's trim are skipped; a word belongs to the speaker at (t0 + t1) / 2; a change of speaker starts
 *     "\n[Speaker s|t0]" with t0 as Rust's {:.1} (the exact decimal value, half to even), the lines are joined with "\n"
 *     and the whole is trimmed.  Without segments or without words: the texts, untrimmed, joined with one space.
 *     Writes at most cap bytes including the NUL; *needed (nullable) = the bytes the full text takes with its NUL;
 *     a result that does not fit is CRISPY_ERR_INVALID_ARG with *needed set (call with out NULL / cap 0 to size).
 *   crispy_diar_format_result: the same over the words of a crispy_asr_result (opts.dtw_token_timestamps), their
 *     times as f64 plus chunk_offset seconds: from crispy_asr_transcribe to diarized text in two calls. */
long crispy_diar_chunk_plan(const double *start, const double *end, const long *n_samples, long n_segments, int sample_rate,
                            double *out_start, double *out_end, long *out_segment, long *out_first, long *out_len, long cap);
long crispy_diar_speaker_segments(const double *start, const double *end, const int *labels, long n, double merge_gap,
                                  double *out_start, double *out_end, int *out_speaker, long cap);
int crispy_diar_find_speaker(double time, const double *seg_start, const double *seg_end, const int *seg_speaker, long n_segments);
int crispy_diar_format_text(const double *t0, const double *t1, const char *const *text, long n_words, const double *seg_start,
                            const double *seg_end, const int *seg_speaker, long n_segments, char *out, size_t cap, size_t *needed);
int crispy_diar_format_result(const crispy_asr_result *r, double chunk_offset, const double *seg_start, const double *seg_end,
                              const int *seg_speaker, long n_segments, char *out, size_t cap, size_t *needed);

/* ------------------------------------------------------------------------------------------
 * Diarization front end: what run_diarization (managers/diarization.rs:276-409) computes between the 16 kHz audio and its
 * two networks, so that a host supplies the networks alone.  New entry points only: no struct grew, the ABI version is
 * unchanged.
 *
 *   crispy_diar_fbank_frames: rows the fbank gives for n samples: n < 400 ? 0 : 1 + (n - 400) / 160.
 *
 *   crispy_diar_speech_segments (host, no device): the post-network half of pyannote_get_segments_fixed (:146-271).
 *     scores [n_windows][n_frames][n_classes] are the segmentation network's outputs on the zero-padded 10 s windows of
 *     :103-128 (the samples as i16 / 32768, padded to a multiple of 160000 plus one more window).  Per frame the f32
 *     soft-max with the maximum subtracted, summed in class order; p_sil = e[0] / sum; speech unless p_sil > 0.5.  The
 *     11-frame median filter (speech where count_speech > count_total / 2, integer division, the window shortened at a
 *     window's edges).  A change of state at frame i of window w falls at sample w * 160000 + 721 + 270 i; the state is
 *     carried from window to window; a start below 1600 snaps to 0; starts and ends are clamped to n_samples and empty
 *     spans dropped; speech still open at the end closes at n_samples.  Sorted by start (stable), merged while start <=
 *     last.end + (usize)(sample_rate * merge_gap), kept from (usize)(sample_rate * 1.5) samples on; if none is left, the
 *     longest merged span (the last of equals).  Outputs as crispy_diar_chunk_plan takes them: start and end in seconds
 *     (index as f64 / rate), first sample, sample count.  Returns the number of segments; entries beyond `cap` are not
 *     written.  sample_rate != 16000, a non-finite merge_gap, n_classes < 1, n_frames < 1: INVALID_ARG; n_samples == 0 or
 *     n_windows == 0: 0.
 *
 *   crispy_diar_fbank_device / crispy_diar_fbank: the features the embedding network reads (EmbeddingExtractor::compute,
 *     :53-75, knf_rs::compute_fbank): an 80-bin Kaldi fbank with per-chunk mean subtraction, every chunk of a call in one
 *     launch pair on a crispy_diar handle.  d_pcm is one 16 kHz mono buffer of pcm_format CRISPY_PCM_I16 (the reference's
 *     &[i16]) or CRISPY_PCM_F32; chunk c is its samples first[c] ... first[c] + len[c] (crispy_diar_chunk_plan's arrays,
 *     the segment's own first sample added; overlapping and out-of-order chunks are fine).  With f32 the kernel applies
 *     f32_to_i16 itself ((s.clamp(-1, 1) * 32767.0) as i16, truncating, NaN -> 0), so the result is bit for bit that
 *     of the i16 form.  x = i16 as f32 / 32768 * scale: scale 1 is what knf-rs hands over, 32768 the Kaldi / WeSpeaker
 *     convention; the mel floor is absolute, so the choice changes results.
 *     Per frame (snip_edges: 400 samples at hop 160, a chunk of fewer than 400 samples has no rows): frame mean removed,
 *     pre-emphasis 0.97 from the back (x[0] -= 0.97 x[0]), Povey window (0.5 - 0.5 cos(2 pi i / 399))^0.85, zero padding to
 *     512, power spectrum (f32; a 256-point complex transform plus the real-input pass), 80 filters triangular in mel
 *     space (1127 ln(1 + f / 700)) between 20 and 8000 Hz over bins 0 ... 255 (501 taps, f32 sums in tap order),
 *     log(max(e, 1.1920929e-07)).  Per chunk every column's mean (the f32 sum in frame order / the frame count) is
 *     subtracted.  d_feats [rows][80]; d_raw (nullable) receives the rows before the subtraction; frame_offset (host,
 *     [n_chunks + 1]) receives each chunk's first row and the total, from the lengths alone: with d_feats NULL the call
 *     only fills it (no device is touched), which sizes the buffers.  A chunk's rows are the same bytes alone and in
 *     any call.  The work is enqueued on hip_stream (NULL: the handle's own) and complete on return.  crispy_diar_fbank
 *     is the same with pcm and feats on the host.
 *     Limits, checked before any launch: 1 <= n_chunks <= 16384, 0 <= len[c] <= 4 800 000, first[c] >= 0, rows x 320
 *     bytes <= 2 GB, scale finite and > 0.  There is no CPU path.
 * ------------------------------------------------------------------------------------------ */
long crispy_diar_fbank_frames(long n_samples);
long crispy_diar_speech_segments(const float *scores, long n_windows, int n_frames, int n_classes, long n_samples, int sample_rate,
                                 double merge_gap, double *out_start, double *out_end, long *out_first, long *out_len, long cap);
int crispy_diar_fbank_device(void *h, const void *d_pcm, int pcm_format, const long *first, const long *len, int n_chunks,
                             float scale, float *d_feats, float *d_raw, long *frame_offset, void *hip_stream);
int crispy_diar_fbank(void *h, const void *pcm, int pcm_format, const long *first, const long *len, int n_chunks, float scale,
                      float *feats, long *frame_offset);

/* ------------------------------------------------------------------------------------------
 * Segmentation network: the first `session.run` of run_diarization (pyannote_get_segments_fixed, :103-145) on a crispy_diar
 * handle -- pyannote segmentation-3.0 ("PyanNet": SincNet, a 4-layer bidirectional LSTM, three linear layers), 16 kHz
 * samples in, log-probabilities [frames][7] out, f32 operands and f32 sums throughout.  New entry points only: no struct
 * grew, the ABI version is unchanged.  The embedding network follows below.
 *
 * The network on one window x[len] (samples as i16 / 32768):
 *   wav_norm1d   InstanceNorm1d(1, affine) over the window: mean and biased variance over len, eps 1e-5, gamma, beta.
 *   conv1d.0     80 filters x 251 taps, stride 10, no bias, no padding (the evaluated sinc filter bank, a plain
 *                [80][1][251] tensor), abs, MaxPool1d(3, 3) (floor), InstanceNorm1d(80, affine) over time, leaky_relu(0.01).
 *   conv1d.1     Conv1d(80, 60, 5) with bias, pool 3, InstanceNorm1d(60, affine), leaky_relu.
 *   conv1d.2     Conv1d(60, 60, 5) with bias, pool 3, InstanceNorm1d(60, affine), leaky_relu -> [frames][60].
 *   lstm         4 layers, bidirectional, hidden 128 (input 60, then 256), torch layout and gate order i, f, g, o; a
 *                layer's output is forward | reverse, [frames][256].
 *   head         Linear(256, 128) + leaky_relu, Linear(128, 128) + leaky_relu, Linear(128, 7), log_softmax.
 *   frames(len) = ((((len - 251) / 10 + 1) / 3 - 4) / 3 - 4) / 3 in integer division: 589 at 160000, 1 at 991.
 *
 * Device work: every instance norm is a two-pass reduction about the row's first value (a constant row normalises to
 * beta exactly); each convolution is one kernel with the previous norm and leaky_relu applied in its load and abs or bias
 * and the max over 3 in its store, so that no pre-pool value reaches memory; per LSTM layer the input projection of all
 * frames, windows and both directions is one GEMM, and the recurrence is one workgroup of 512 threads per (window,
 * direction) with row g of weight_hh in thread g's registers, h and the four gates of a cell in LDS and c in registers,
 * exp and tanh in their accurate forms; the head takes 8 frame rows per workgroup.  The order of every sum depends on
 * the window's own length alone: a window's scores are the same bytes alone and in any batch or turn.
 * Scratch is the handle's (grow and keep): 6.6 MB per full window, windows taken in turns below 2 GB.
 *
 *   crispy_diar_seg_frames   the formula above; 0 below 991 samples.  No device.
 *   crispy_diar_seg_windows  windows crispy_diar_seg_scores gives for n samples: 0 for 0, else ceil(n / 160000) + 1.
 *   crispy_diar_seg_load     host tensors by name (pyannote's state-dict keys), data[i] holding count[i] floats:
 *       sincnet.wav_norm1d.{weight,bias} [1]; sincnet.conv1d.0.filters [80][1][251]; sincnet.conv1d.1.{weight,bias}
 *       [60][80][5], [60]; sincnet.conv1d.2.{weight,bias} [60][60][5], [60]; sincnet.norm1d.{0,1,2}.{weight,bias} [80],
 *       [60], [60]; lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0..3}[_reverse] [512][in], [512][128], [512], [512];
 *       linear.0.{weight,bias} [128][256], [128]; linear.1.{weight,bias} [128][128], [128]; classifier.{weight,bias}
 *       [7][128], [7] -- 51 tensors.  A missing, repeated or unknown name, a count that is not the tensor's size, a NULL
 *       pointer or a non-finite value is CRISPY_ERR_INVALID_ARG with the tensor's name in the message, before the device is
 *       touched.  A second load replaces the first; the handle owns the device copy.
 *   crispy_diar_seg_loaded   1 after a successful load, else 0 (NULL handle: 0).
 *   crispy_diar_seg_forward_device  the network on n_win windows d_x [n_win][len] of one length 991 <= len <= 160000,
 *       1 <= n_win <= 4096 -> d_scores [n_win][frames(len)][7]; stage outputs for tests and profiling: d_sincnet
 *       (nullable) [n_win][frames][60], d_lstm (nullable) [n_win][frames][256], the last layer's.  Enqueued on hip_stream
 *       (NULL: the handle's own), complete on return.  Before a load: CRISPY_ERR_INVALID_ARG.
 *   crispy_diar_seg_scores_device / crispy_diar_seg_scores  a whole recording: d_pcm is CRISPY_PCM_I16 or CRISPY_PCM_F32
 *       (f32_to_i16 on the device, as the fbank does); the zero padding to a multiple of 160000 plus one more window and the
 *       / 32768 are formed on the device -> d_scores [crispy_diar_seg_windows(n_samples)][589][7], what
 *       crispy_diar_speech_segments takes.  1 <= n_samples <= 115 200 000 (2 h); checked before any launch.  The second
 *       form takes pcm and scores on the host.  There is no CPU path.
 * ------------------------------------------------------------------------------------------ */
long crispy_diar_seg_frames(long len);
long crispy_diar_seg_windows(long n_samples);
int crispy_diar_seg_load(void *h, const char *const *names, const float *const *data, const long *count, int n_tensors);
int crispy_diar_seg_loaded(void *h);
int crispy_diar_seg_forward_device(void *h, const float *d_x, int n_win, long len, float *d_scores, float *d_sincnet, float *d_lstm,
                                   void *hip_stream);
int crispy_diar_seg_scores_device(void *h, const void *d_pcm, int pcm_format, long n_samples, float *d_scores, void *hip_stream);
int crispy_diar_seg_scores(void *h, const void *pcm, int pcm_format, long n_samples, float *scores);

/* ------------------------------------------------------------------------------------------
 * Embedding network: the `session.run` of EmbeddingExtractor::compute (:53-75) on a crispy_diar handle -- WeSpeaker CAMPPlus
 * ("CAM++", wespeaker_en_voxceleb_CAM++.onnx: input "feats" [1][T][80], output "embs" [dim]), the fbank rows of
 * crispy_diar_fbank in, one embedding per chunk out, f32 operands and f32 sums throughout.  New entry points only: no
 * struct grew, the ABI version is unchanged.  With it run_diarization needs no network from the host.
 *
 * The network on one chunk [T][80] (every BatchNorm at inference, eps 1e-5; "BR" = BatchNorm, ReLU):
 *   head (FCM)   on [1][80][T], frequency strided, time never: Conv2d(1, 32, 3x3, pad 1) BR; layer1 and layer2, each two
 *                BasicResBlocks of 32 channels (conv 3x3 stride (s, 1) BR, conv 3x3 B, + shortcut, ReLU; block .0 has s = 2
 *                and a 1x1 stride (2, 1) convolution + B as shortcut, block .1 s = 1 and the identity): 80 -> 40 -> 20;
 *                Conv2d(32, 32, 3x3, stride (2, 1)) BR -> [32][10][T] -> [T][320], channel c * 10 + f.
 *   tdnn         Conv1d(320, 128, 5, stride 2, pad 2) BR -> T2 = (T - 1) / 2 + 1 positions.
 *   blocks       12 layers at dilation 1, 24 at 2, 16 at 2, growth 32; a layer with Cin inputs: BR, Conv1d(Cin, 128, 1), BR = h;
 *                y = Conv1d(128, 32, 3, dilation d, pad d)(h); ctx = mean over time of h + mean of h over consecutive
 *                segments of 100 positions (the last one over its own count); out = y * sigmoid(Conv1d(64, 32, 1)(relu(
 *                Conv1d(128, 64, 1)(ctx)))), appended.  After each block a transit: BR, Conv1d(C, C / 2, 1).  Channels
 *                128 -> 512 -> 256 -> 1024 -> 512 -> 1024 -> 512.
 *   pooling      BR, then mean and sqrt(unbiased variance + 1e-7) over time -> [1024]; Conv1d(1024, dim, 1); BatchNorm
 *                without affine terms -> [dim].
 * The unbiased variance needs T2 >= 2: a chunk of fewer than 3 rows is refused (CRISPY_ERR_INVALID_ARG) before any launch;
 * run_diarization drops such chunks as it drops chunks without rows.
 *
 * Device work: every BatchNorm is folded at load into a (scale, shift) pair in double, rounded once.  Rows are time-major
 * from the tdnn on; a block is one buffer whose layers append in place.  Every 1x1 convolution (linear1 of the 52 dense
 * layers, the transits) is one kernel on the f32 matrix instruction (v_mfma_f32_32x32x2_f32, exact f32) with the BatchNorm
 * and ReLU in front in its operand load and those behind in its store, k ascending in blocks of 64 that are added in order.
 * The context sums are formed per chunk in a fixed order without atomics.  A chunk's embedding and taps are the same bytes
 * alone, at any position of any batch and in any turn.  Scratch is the handle's (grow and keep): 33 KB per feature row,
 * chunks taken in turns below 2 GB.
 *
 *   crispy_diar_emb_frames       T2 for `rows` feature rows; 0 for rows < 1.  No device.
 *   crispy_diar_emb_tensor_spec  the i-th tensor crispy_diar_emb_load expects for an embedding width `dim`: its state-dict key
 *       (*name, nullable; static storage) and element count (*count, nullable), in the order of wespeaker's state dict
 *       without the num_batches_tracked entries.  Returns the number of tensors (815); CRISPY_ERR_INVALID_ARG for i out of
 *       range or dim outside 1 ... 1024.  No device, no handle.
 *   crispy_diar_emb_load         host tensors by name, data[i] holding count[i] floats; dim = count of
 *       xvector.dense.linear.weight / 1024, 1 <= dim <= 1024.  A missing, repeated or unknown name, a count that is not
 *       the tensor's size, a NULL pointer, a non-finite value or a running_var below 0 is CRISPY_ERR_INVALID_ARG with the
 *       tensor's name in the message, before the device is touched.  A second load replaces the first; the handle owns
 *       the device copy.
 *   crispy_diar_emb_loaded / crispy_diar_emb_dim  1 / the width after a successful load, else 0 (NULL handle: 0).
 *   crispy_diar_emb_forward_device  d_feats [rows][80] with host frame_offset [n_chunks + 1] (frame_offset[0] = 0), exactly
 *       what crispy_diar_fbank_device produces -> d_emb [n_chunks][dim]; stage outputs for tests and profiling, each
 *       nullable: d_head [rows][320], d_xvec [sum T2][512] (after the last BatchNorm and ReLU), d_stats [n_chunks][1024].
 *       1 <= n_chunks <= 16384; 3 <= rows of a chunk <= 30000 (5 min; the fbank gives at most 29998 for its longest
 *       chunk; one such chunk takes 1.0 GB of scratch); checked before any launch.  Enqueued on hip_stream (NULL: the
 *       handle's own), complete on return.  Before a load: CRISPY_ERR_INVALID_ARG.
 *   crispy_diar_embed_device / crispy_diar_embed  EmbeddingExtractor::compute for all chunks of a recording in one call:
 *       pcm, first, len, n_chunks and scale as crispy_diar_fbank takes them -> embeddings [n_chunks][dim]; the feature rows
 *       never leave the device.  A chunk with fewer than 3 rows is CRISPY_ERR_INVALID_ARG (filter with
 *       crispy_diar_fbank_frames).  The result equals crispy_diar_emb_forward_device on crispy_diar_fbank_device's rows bit
 *       for bit.  The second form takes pcm and the embeddings on the host.  There is no CPU path.
 * ------------------------------------------------------------------------------------------ */
long crispy_diar_emb_frames(long rows);
int crispy_diar_emb_tensor_spec(int i, int dim, const char **name, long *count);
int crispy_diar_emb_load(void *h, const char *const *names, const float *const *data, const long *count, int n_tensors);
int crispy_diar_emb_loaded(void *h);
int crispy_diar_emb_dim(void *h);
int crispy_diar_emb_forward_device(void *h, const float *d_feats, const long *frame_offset, int n_chunks, float *d_emb, float *d_head,
                                   float *d_xvec, float *d_stats, void *hip_stream);
int crispy_diar_embed_device(void *h, const void *d_pcm, int pcm_format, const long *first, const long *len, int n_chunks, float scale,
                             float *d_emb, void *hip_stream);
int crispy_diar_embed(void *h, const void *pcm, int pcm_format, const long *first, const long *len, int n_chunks, float scale, float *emb);

/* ------------------------------------------------------------------------------------------
 * Parakeet encoder: the FastConformer encoder of parakeet-tdt-0.6b (v2 and v3), the model the reference recommends first
 * (commands/models.rs:145, managers/model.rs:150-186) -- log-mel feature rows in, encoder frames out, f32 operands and f32
 * sums throughout.  The log-mel front end and the TDT decoder have sections of their own below.  New entry points only: no struct of an
 * existing entry point grew, the ABI version is unchanged.  State-dict keys are those of transformers' ParakeetEncoder; all
 * of it is inference.
 *
 * The network on one clip [T][M] (crispy_pk_config: hidden H = 128 x heads, layers, heads, ffn, conv_kernel K (odd), mel_bins M
 * (a multiple of 8), sub_channels C, and the flags attention_bias, convolution_bias, scale_input, each 0 or 1; a flag at 0
 * means those bias tensors are absent from the load):
 *   subsampling  the clip as a 1-channel image (time x mel): Conv2d(1, C, 3, stride 2, pad 1), ReLU; twice depthwise
 *                Conv2d(C, C, 3, stride 2, pad 1, groups C), Conv2d(C, C, 1), ReLU; then [T'][C * M / 8] (index c * M / 8 + f),
 *                Linear to H, times sqrt(H) with scale_input.  T' is L -> (L - 1) / 2 + 1 applied three times.
 *   block        x += 0.5 FF1(LN(x)); x += Attn(LN(x)); x += Conv(LN(x)); x += 0.5 FF2(LN(x)); x = LN_out(x); LayerNorm eps 1e-5,
 *                FF = linear2(silu(linear1(.))) (its biases follow attention_bias).
 *   attention    q, k, v, o projections, relative_k_proj without bias, bias_u and bias_v [heads][128];
 *                score(i, j) = ((q_i + u) . k_j + (q_i + v) . r_{i - j}) / sqrt(128) with r_d = relative_k_proj(pos(d)); soft-max
 *                over the clip's own T' keys.  pos(d)[2k] = f32(sin(arg)), pos(d)[2k + 1] = f32(cos(arg)) in double, arg the one
 *                f32 product f32(d) * f32(1 / 10000^(2k / H)).
 *   convolution  pointwise_conv1 (H -> 2H), GLU over channels, depthwise Conv1d(H, H, K, pad (K - 1) / 2) zero-padded at the
 *                clip's own edges, BatchNorm (eps 1e-5), SiLU, pointwise_conv2.
 *
 * Device work: clips are ragged and lie end to end, [sum T'][H] with the host's frame_offset.  The subsampling is three
 * kernels (the first convolution; each depthwise + pointwise + ReLU pair in one, the depthwise image never stored).  Every
 * Linear and 1x1 convolution is one GEMM kernel on the f32 matrix instruction (v_mfma_f32_32x32x2_f32, exact f32), k ascending
 * in chains of 64 that are added in order; its store carries bias, SiLU, GLU, the residual with its factor or the input scale.
 * LayerNorm is a row pass.  Attention is one workgroup per (clip, head, 32 queries) over key tiles of 32 with a running maximum
 * and sum and no [T'][T'] buffer; the position term of a tile pair is one product with the 63-row band of R it needs.  The
 * BatchNorm and the depthwise bias are folded at load into a (scale, shift) pair in double.  No atomics: a clip's frames are
 * the same bytes alone, at any position of any batch and in any call.
 *
 *   crispy_pk_create / crispy_pk_destroy   a handle on `device` with its own stream; the workspace grows on demand and is kept.
 *   crispy_pk_frames       T' for `rows` feature rows; 0 for rows < 1.  No device.
 *   crispy_pk_tensor_spec  the i-th tensor crispy_pk_load expects for `cfg` (a const crispy_pk_config *): its state-dict key
 *       (*name, nullable; valid until the calling thread's next call) and element count (*count, nullable), in state-dict
 *       order without the num_batches_tracked entries.  Returns the number of tensors; CRISPY_ERR_INVALID_ARG for i out of
 *       range or a config outside the supported set (heads 1 ... 16, hidden = 128 x heads, layers 1 ... 64, ffn a multiple of
 *       128 up to 16384, conv_kernel odd 3 ... 31, mel_bins a multiple of 8 up to 256, sub_channels a multiple of 32 up to
 *       512, flags 0 or 1), naming the field.  No device, no handle.
 *   crispy_pk_load         host tensors by name, data[i] holding count[i] floats.  A missing, repeated or unknown name, a count
 *       that is not the tensor's size, a NULL pointer, a non-finite value, a running_var below 0 or an unsupported config is
 *       CRISPY_ERR_INVALID_ARG with the tensor's or field's name in the message, before the device is touched.  A second
 *       load replaces the first; the handle owns the device copy.
 *   crispy_pk_loaded / crispy_pk_config_of   1 after a successful load, else 0 (NULL handle: 0) / the loaded config into
 *       *cfg (a crispy_pk_config *); CRISPY_ERR_INVALID_ARG before a load.
 *   crispy_pk_encode_device  d_feats [rows][M] with host frame_offset [n_clips + 1] (frame_offset[0] = 0) -> d_out [sum T'][H].
 *       Stage outputs, each nullable: d_sub [sum T'][H] the subsampling output after the scale, d_tap [sum T'][H] the output
 *       of block tap_layer (0 ... layers - 1, checked when d_tap is given), d_pos [2 Tmax - 1][H] the position table, row p
 *       for d = p - (Tmax - 1), Tmax the longest clip's T'.  1 <= rows of a clip <= 40000 (T' <= 5000), 1 <= n_clips <= 4096,
 *       checked before any launch.  The workspace (46 KB per feature row at the catalog widths, 32 of them the first image) is sized from the call and
 *       checked against the device's free memory before any launch: too large is CRISPY_ERR_OOM with nothing enqueued.
 *       Enqueued on hip_stream (NULL: the handle's own), complete on return.  Before a load: CRISPY_ERR_INVALID_ARG.
 *   crispy_pk_encode       the same call with host pointers; bit-identical results.  There is no CPU path.
 * ------------------------------------------------------------------------------------------ */
typedef struct crispy_pk_config {
  int hidden, layers, heads, ffn, conv_kernel, mel_bins, sub_channels, attention_bias, convolution_bias, scale_input;
} crispy_pk_config;

int crispy_pk_create(int device, void **out);
void crispy_pk_destroy(void *h);
long crispy_pk_frames(long rows);
int crispy_pk_tensor_spec(const void *cfg, int i, const char **name, long *count);
int crispy_pk_load(void *h, const void *cfg, const char *const *names, const float *const *data, const long *count, int n_tensors);
int crispy_pk_loaded(void *h);
int crispy_pk_config_of(void *h, void *cfg);
int crispy_pk_encode_device(void *h, const float *d_feats, const long *frame_offset, int n_clips, float *d_out, float *d_sub, int tap_layer,
                            float *d_tap, float *d_pos, void *hip_stream);
int crispy_pk_encode(void *h, const float *feats, const long *frame_offset, int n_clips, float *out, float *sub, int tap_layer, float *tap,
                     float *pos);

/* ------------------------------------------------------------------------------------------
 * Parakeet encoder, precision mode 1: f16 operands on the dense matrix cores, f32 sums.  New entry points only: no struct
 * grew, the ABI version is unchanged.  Mode 0 (the default) is the section above, bit for bit.
 *
 * Definition.  Every product that the GEMM performs inside crispy_pk_encode -- subsampling.linear, the four feed-forward
 * linears, the fused q | k | v projection, relative_k_proj on the position table, o_proj, pointwise_conv1 and pointwise_conv2 --
 * takes BOTH operands rounded once to IEEE binary16: round to nearest even, subnormals kept (not flushed), overflow to
 * infinity, exactly torch.Tensor.to(torch.float16).  The products are exact and the sums are f32: one accumulator per output
 * element on v_mfma_f32_32x32x16_f16, k ascending in steps of 16 from zero, a chain of K / 16 instructions, so an element's
 * sum depends on K alone -- not on the row's place in a tile, the clip count or its neighbours.  Everything else is mode 0's
 * f32 arithmetic, untouched: the subsampling convolutions, LayerNorm, the attention products and soft-max, the depthwise
 * convolution with its BatchNorm, the bias, the epilogues (scale, SiLU, GLU, residual) and the residual stream.  The features,
 * the TDT handle and its encoder_projector stay f32.  An activation beyond 65504 in magnitude rounds to infinity and makes its
 * own row non-finite; no other row changes.
 *
 *   crispy_pk_set_precision  mode 0 or 1; anything else is CRISPY_ERR_INVALID_ARG naming `mode`.  May be set before or after
 *       crispy_pk_load and survives a reload.  The first time a loaded handle is in mode 1 the f16 copies of the GEMM weights
 *       are packed on the device from the resident f32 matrices (2 bytes per GEMM weight: about 1.2 GB at the catalog widths),
 *       after a check against the device's free memory: CRISPY_ERR_OOM leaves the handle in the mode it had with nothing
 *       enqueued.  The copies live until crispy_pk_destroy or the next load; a load in mode 1 packs its own and is refused as
 *       a whole when they do not fit.  crispy_pk_encode[_device] and crispy_pk_transcribe[_device] honour the encoder handle's mode.
 *   crispy_pk_precision      the mode (NULL handle: 0).
 *   crispy_pk_stage_gemm_device  one GEMM of the encoder as a stage, for tests; needs no load.  d_a [M][K] f32, d_w f32 in the
 *       state-dict layout [cols][K] (cols = N, or 2 N with the GLU, in pointwise_conv1's own row order), d_bias [cols] or NULL,
 *       d_res [M][N] (the residual epilogue only; may be d_c), d_c [M][N].  epilogue: CRISPY_PK_GEMM_SCALE (v * alpha), _SILU,
 *       _RESIDUAL (res + alpha * v), _GLU (value * sigmoid(gate)).  The weight goes through the transposition of the load's
 *       layout, mode 1's pack kernel and the encoder's own GEMM dispatch.  K a multiple of 32, cols of 128, M >= 1; otherwise
 *       CRISPY_ERR_INVALID_ARG.  On the handle's stream, complete on return.
 * ------------------------------------------------------------------------------------------ */
#define CRISPY_PK_GEMM_SCALE 0
#define CRISPY_PK_GEMM_SILU 1
#define CRISPY_PK_GEMM_RESIDUAL 2
#define CRISPY_PK_GEMM_GLU 3
int crispy_pk_set_precision(void *h, int mode);
int crispy_pk_precision(void *h);
int crispy_pk_stage_gemm_device(void *h, int mode, int epilogue, const float *d_a, long M, int K, const float *d_w, const float *d_bias, int N,
                                float alpha, const float *d_res, float *d_c);

/* ------------------------------------------------------------------------------------------
 * Parakeet encoder, attention mode 1: f16 operands in the three products of the relative-position attention, f32 sums.  A second
 * switch on the encoder handle, independent of crispy_pk_set_precision: all four combinations are valid.  New entry points only:
 * no struct grew, the ABI version is unchanged.  Attention mode 0 (the default) is today's attention bit for bit under both GEMM
 * modes.
 *
 * Definition, per (clip, head), over the clip's own n frames.  q, k and v are the f32 outputs of the fused projection, r the f32
 * output of relative_k_proj on the position table, u and v_b the head's bias_u and bias_v.
 *   1. Operands.  Five operands are each rounded once to IEEE binary16: q + u and q + v_b (the sums formed in f32, then rounded),
 *      k, r and v -- round to nearest even, subnormals kept, overflow to infinity, exactly torch.Tensor.to(torch.float16).
 *      Products are exact in f32 and sums are f32.
 *   2. Score.  ac(i, j) = f16(q_i + u) . f16(k_j), bd(i, d) = f16(q_i + v_b) . f16(r_d), and
 *      score(i, j) = (ac(i, j) + bd(i, i - j)) * 128^-1/2: the addition and the scale are f32 and come after the sums (the scale
 *      is not folded into an operand: 2^-3.5 is not exact).
 *   3. Soft-max.  Over the keys in tiles of CRISPY_PK_ATTN_KEY_TILE keys, ascending from the clip's first key, with a running
 *      maximum m and sum l in f32 (m = -inf, l = 0, o = 0 at the start):  m_new = max(m, the tile's largest score);
 *      alpha = expf(m - m_new);  p_j = expf(score_j - m_new);  l = l * alpha + the sum of the unrounded f32 p_j;
 *      o = o * alpha + sum_j f16(p_j) * f16(v_j) (f32 sums);  at the end out = o / l.  Keys behind the clip's end contribute
 *      nothing.  The tile length is part of the definition: f16(p_j) is rounded relative to the running maximum, so another
 *      tiling gives other f16 neighbours.  The order of the additions inside one sum is the implementation's, fixed, and depends
 *      on the clip's own length alone: a clip's bytes are the same alone, at any position of any batch and in any call.
 *   4. Overflow.  An operand beyond 65504 in magnitude makes rows of its own clip non-finite; no other clip's bytes change.
 *
 *   crispy_pk_set_attention_precision  mode 0 or 1; anything else is CRISPY_ERR_INVALID_ARG naming `mode` and leaves the handle
 *       as it was.  May be set before or after crispy_pk_load and survives a reload.  Allocates nothing (the operands are
 *       activations; no weights are packed) and cannot fail on memory.  crispy_pk_encode[_device] and
 *       crispy_pk_transcribe[_device] honour the encoder handle's mode.  crispy_pk_precision is unaffected, and the reverse.
 *   crispy_pk_attention_precision      the mode (NULL handle: 0).
 *   crispy_pk_stage_attention_device   one attention pass as a stage, for tests; needs no load.  d_qkv [sum n][3 * heads * 128]
 *       as the fused projection stores it (q | k | v side by side, each head's 128 columns together); d_r [2 tmax - 1][heads * 128],
 *       row p for the distance d = p - (tmax - 1); d_bias_u, d_bias_v [heads * 128]; frame_offset a host array [n_clips + 1] of
 *       the clips' first frames, frame_offset[0] = 0; d_out [sum n][heads * 128].  The device pointers are 16-byte aligned.  Goes
 *       through the encoder's own attention dispatch with `mode`, whatever the handle's mode is.  Refused with
 *       CRISPY_ERR_INVALID_ARG naming the field, with nothing enqueued: a NULL pointer, n_clips outside 1 ... 4096, heads outside
 *       1 ... 16, tmax outside 1 ... 5000, a clip of 0 frames or longer than tmax, mode outside 0 / 1.  On the handle's stream,
 *       complete on return.
 * ------------------------------------------------------------------------------------------ */
#define CRISPY_PK_ATTN_KEY_TILE 32
int crispy_pk_set_attention_precision(void *h, int mode);
int crispy_pk_attention_precision(void *h);
int crispy_pk_stage_attention_device(void *h, int mode, const float *d_qkv, const float *d_r, const float *d_bias_u, const float *d_bias_v,
                                     const long *frame_offset, int n_clips, int heads, int tmax, float *d_out);

/* ------------------------------------------------------------------------------------------
 * Parakeet TDT decoder: greedy token-and-duration transducer decoding of the encoder's frames -- tokens with frame times, and
 * from them the (start_s, end_s, word) records of the reference's transcribe_with_timestamps
 * (managers/transcription.rs:196-237).  f32 operands and f32 sums throughout; the whole loop runs on the device.  New entry
 * points only, the ABI version is unchanged.  State-dict keys are those of transformers' ParakeetForTDT behind its encoder.
 *
 * crispy_pk_tdt_config: hidden H (the encoder's, a multiple of 32), decoder_hidden D (a multiple of 128 up to 2048),
 * decoder_layers L (1 ... 8), vocab V (2 ... 65536, the blank included), blank (< V), n_durations (1 ... 8) of durations[8]
 * (non-negative, strictly ascending), max_symbols_per_step (1 ... 64).  Tensors: encoder_projector.{weight [D][H], bias},
 * decoder.embedding.weight [V][D], decoder.lstm.{weight_ih_l*, weight_hh_l* [4D][D], bias_ih_l*, bias_hh_l*} (gates i, f, g, o),
 * decoder.decoder_projector.{weight [D][D], bias}, joint.head.{weight [V + n_d][D], bias}.
 *
 * The loop on one clip's frames e[0 .. T'):  p = encoder_projector(e);  t = 0, (h, c) = 0,
 * g = decoder_projector(lstm(embedding[blank])) (which updates the state);  at each step logits = head(relu(p[t] + g)),
 * k = arg-max of the first V logits, d = durations[arg-max of the last n_d], ties to the lowest index; a blank with d == 0
 * takes d = 1; the step (k, t, d) is recorded and t += d; a non-blank k runs the LSTM and the projector on embedding[k] and
 * replaces (h, c, g), a blank leaves them.  The clip ends with t >= T' or after max_symbols_per_step * T' - 1 steps
 * (crispy_pk_tdt_max_steps).  The emitted tokens are the steps with k != blank; a token starts at frame t and ends at
 * min(t + d, T').
 *
 * Device work: all clips of a call step together.  A step is five launches at L = 2: the joint product with each column
 * tile's arg-max, the per-clip advance (arg-max in index order, duration rule, step log, frame pointer, next token, flags, the
 * finished-clips counter), one launch per LSTM layer and decoder_projector on the clips that emitted a token.  Every sum
 * runs in an order fixed by its length alone and no workgroup reads another clip's state: a clip's steps and tapped logits
 * are the same bytes alone, at any position of any batch and in any call.  The host enqueues steps in groups of 32 and reads
 * one counter between groups; a call enqueues at most max_symbols_per_step * Tmax - 1 steps.
 *
 *   crispy_pk_tdt_create / _destroy / _tensor_spec / _load / _loaded / _config_of   as their crispy_pk_* namesakes, `cfg` a
 *       (const) crispy_pk_tdt_config *.  A load takes exactly the tensors above: a ParakeetForTDT state dict without its
 *       encoder.* keys.
 *   crispy_pk_tdt_max_steps  the step budget of one clip of `frames` frames (0 for frames < 1); CRISPY_ERR_INVALID_ARG for a
 *       config outside the supported set or frames > 5000.  No device.
 *   crispy_pk_tdt_decode_device  d_frames [sum T'][H] with host frame_offset [n_clips + 1] (frame_offset[0] = 0) ->
 *       d_steps [sum budget][3] int32 (token, frame, duration), clip c's rows starting at the sum of the budgets before it
 *       and d_n_steps[c] of them written, the rest untouched.  1 <= n_clips <= 4096, 0 <= T' <= 5000; a clip with T' = 0
 *       gives zero steps.  Taps, each nullable: d_proj_tap [sum T'][D] the projected frames, d_logits_tap
 *       [sum budget][V + n_d] each step's logits in the rows of d_steps.  The logits tap is test equipment: at the catalog
 *       widths it is 33 KB per step of budget, 123 MB for one 30 s clip.  The workspace is sized from the call and checked
 *       against the device's free memory before any launch: too large is CRISPY_ERR_OOM with nothing enqueued.  Enqueued on
 *       hip_stream (NULL: the handle's own), complete on return.  Before a load: CRISPY_ERR_INVALID_ARG.
 *   crispy_pk_tdt_decode   the same call with host pointers; bit-identical results; rows behind n_steps[c] are zeros.
 *   crispy_pk_tdt_words    host only, no device, no handle: one clip's steps -> words.  pieces: the vocabulary as `vocab`
 *       NUL-terminated UTF-8 pieces.  A piece that begins with U+2581 starts a word, and so does the first token; the marker
 *       is removed and pieces are concatenated; blanks never appear.  Word i starts at start_s[i] = its first token's frame
 *       and ends at end_s[i] = its last token's min(frame + duration, frames), both times seconds_per_frame (0.08 for the
 *       catalog models: hop 10 ms times the 8-fold subsampling); its text is the NUL-terminated string at text + text_off[i].
 *       Returns the number of words and sets *text_needed (nullable) to the bytes the texts take with their NULs.  When
 *       max_words or text_cap is too small (or a buffer is NULL) nothing is written: call again with what was returned.
 * ------------------------------------------------------------------------------------------ */
typedef struct crispy_pk_tdt_config {
  int hidden, decoder_hidden, decoder_layers, vocab, blank, n_durations, durations[8], max_symbols_per_step;
} crispy_pk_tdt_config;

int crispy_pk_tdt_create(int device, void **out);
void crispy_pk_tdt_destroy(void *h);
int crispy_pk_tdt_tensor_spec(const void *cfg, int i, const char **name, long *count);
int crispy_pk_tdt_load(void *h, const void *cfg, const char *const *names, const float *const *data, const long *count, int n_tensors);
int crispy_pk_tdt_loaded(void *h);
int crispy_pk_tdt_config_of(void *h, void *cfg);
long crispy_pk_tdt_max_steps(const void *cfg, long frames);
int crispy_pk_tdt_decode_device(void *h, const float *d_frames, const long *frame_offset, int n_clips, int *d_steps, int *d_n_steps,
                                float *d_proj_tap, float *d_logits_tap, void *hip_stream);
int crispy_pk_tdt_decode(void *h, const float *frames, const long *frame_offset, int n_clips, int *steps, int *n_steps, float *proj_tap,
                         float *logits_tap);
long crispy_pk_tdt_words(const int *steps, int n_steps, int frames, int blank, const char *const *pieces, int vocab, double seconds_per_frame,
                         float *start_s, float *end_s, long *text_off, int max_words, char *text, long text_cap, long *text_needed);

/* ------------------------------------------------------------------------------------------
 * Parakeet front end: the log-mel features of transformers' ParakeetFeatureExtractor from 16 kHz mono f32 samples, and the
 * whole arm in one call -- samples in, steps (tokens with frame times) out, as the reference calls the model
 * (engine.transcribe(&audio), managers/transcription.rs:174-249).  Exact f32 operands.  New entry points only, the ABI version
 * is unchanged.  The entry points take the encoder's handle (crispy_pk_create); the features need no load.
 *
 * A clip of n samples gives rows = n / 160 (rounded down) rows of M values:
 *   pre-emphasis   y[0] = x[0], y[i] = x[i] - f32(0.97 x[i - 1]), 0 outside the clip's own [0, n).
 *   frames         frame t is centred at sample 160 t: a symmetric 400-point Hann window from sample 160 t - 200, zero-padded to
 *                  512, a real 512-point transform, re^2 + im^2 over bins 0 ... 256.
 *   mel            M filters over the 257 bins, then logf(e + 2^-24).  Built in: Slaney triangles (Slaney scale and norm,
 *                  0 ... 8000 Hz) for any M in 1 ... 128, worked out in double and rounded once.
 *   normalisation  per clip and bin over the clip's own rows: (v - mean) / (std + 1e-5f), std with the divisor rows - 1.
 *
 * Device work: three launches for all clips of a call.  The frame kernel (a workgroup per 32 consecutive frames of one clip)
 * reads samples straight from the clip, keeps twiddles, window and filters in LDS, sums each filter's run of weights in f32 in
 * tap order and stores the rows before normalisation and, per (tile, bin), partial sums in double about the tile's first
 * value; a second kernel adds a clip's partial sums in tile order in double and rounds mean and std once to f32 (a constant
 * column gives std = 0 and rows of exactly 0); a third normalises.  No atomics: a clip's rows are the same bytes alone, at any
 * position of any batch and in any call.
 *
 *   crispy_pk_feature_rows   rows for `samples` samples (0 below 160).  No device.
 *   crispy_pk_mel_filters    the built-in filters for mel_bins (1 ... 128) into fb [mel_bins][257].  No device, no handle.
 *   crispy_pk_set_mel_filters  replaces the built-in filters of handle h with fb [mel_bins][257], for example a checkpoint's own
 *       featurizer.fb; fb = NULL restores the built-in ones (mel_bins is then ignored).  Each filter is stored as the one run
 *       of bins that covers its non-zero weights; a non-finite weight or more than 4096 weights in all runs is
 *       CRISPY_ERR_INVALID_ARG and leaves the handle as it was.
 *   crispy_pk_features_device  d_pcm [sum n] f32 with host sample_offset [n_clips + 1] (sample_offset[0] = 0) -> d_feats
 *       [sum rows][mel_bins], what crispy_pk_encode_device takes.  Taps, each nullable: d_raw_tap [sum rows][mel_bins] the rows
 *       before normalisation, d_stats_tap [n_clips][2][mel_bins] each clip's mean and std.  1 <= n_clips <= 4096; a clip with
 *       fewer than 320 samples (std would divide by 0) or more than 40000 rows is CRISPY_ERR_INVALID_ARG naming the clip, and
 *       so is a mel_bins outside 1 ... 128, other than the loaded encoder's (after a load) or other than that of the filters
 *       set -- all before anything is enqueued.  The workspace (rows before normalisation, 24 bytes per bin and 32 rows of
 *       partial sums) is sized from the call and checked against the device's free memory before any launch: too large is
 *       CRISPY_ERR_OOM.  Enqueued on hip_stream (NULL: the handle's own), complete on return.
 *   crispy_pk_features       the same call with host pointers; bit-identical results.  There is no CPU path.
 *   crispy_pk_transcribe_device  features, crispy_pk_encode_device and crispy_pk_tdt_decode_device in one call: d_pcm and
 *       sample_offset as above -> d_steps and d_n_steps as crispy_pk_tdt_decode_device lays them out, clip c's rows starting
 *       at the sum of crispy_pk_tdt_max_steps(cfg, crispy_pk_frames(rows)) before it.  Rows and frames stay in h_enc's
 *       workspace.  With hip_stream = NULL the features and the encoder run on h_enc's stream and the decoder on h_tdt's,
 *       which waits for an event, not the host; otherwise everything runs on hip_stream.  Refused with
 *       CRISPY_ERR_INVALID_ARG and nothing enqueued: either handle without a load, a `hidden` that differs between the two
 *       configs, handles on different devices, and what crispy_pk_features_device refuses.  Complete on return.
 *   crispy_pk_transcribe     the same call with host pointers; bit-identical results; rows behind n_steps[c] are zeros.
 * ------------------------------------------------------------------------------------------ */
long crispy_pk_feature_rows(long samples);
int crispy_pk_mel_filters(int mel_bins, float *fb);
int crispy_pk_set_mel_filters(void *h, int mel_bins, const float *fb);
int crispy_pk_features_device(void *h, int mel_bins, const float *d_pcm, const long *sample_offset, int n_clips, float *d_feats,
                              float *d_raw_tap, float *d_stats_tap, void *hip_stream);
int crispy_pk_features(void *h, int mel_bins, const float *pcm, const long *sample_offset, int n_clips, float *feats, float *raw_tap,
                       float *stats_tap);
int crispy_pk_transcribe_device(void *h_enc, void *h_tdt, const float *d_pcm, const long *sample_offset, int n_clips, int *d_steps,
                                int *d_n_steps, void *hip_stream);
int crispy_pk_transcribe(void *h_enc, void *h_tdt, const float *pcm, const long *sample_offset, int n_clips, int *steps, int *n_steps);

#ifdef __cplusplus
}
#endif
#endif /* CRISPY_HIP_H */

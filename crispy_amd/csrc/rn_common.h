// rn_common.h -- shared host/device declarations for the batched RNNoise path (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crispy {

constexpr int RN_FRAME = 480;
constexpr int RN_WINDOW = 960;
constexpr int RN_NFREQ = 481;
constexpr int RN_NB = 22;
constexpr int RN_NFEAT = 42;
constexpr int RN_PITCH_BUF = 1728;
constexpr int RN_HIST = 1920;          // 4 frames of high-passed history kept per stream
constexpr int RN_HIST_FRAMES = 4;
constexpr int RN_TAPS = 72;
constexpr int RN_WEIGHT_BYTES = 87503;
constexpr int RN_DBG_FLOATS = 4304;    // mirrors oracle RNO_DBG_*

// Device tables (built on the host in double precision, one copy per handle).
struct RnTables {
  float half_window[RN_FRAME];
  float dct[RN_NB * RN_NB];   // dct[j*22+i] = cos((j+.5) i pi/22), column 0 scaled by sqrt(.5)
  float tansig[208];          // tanh(0.04 i) rounded to 6 decimals, i = 0..200
  float2 w960[RN_WINDOW];     // exp(-2 pi i k / 960)
  float bin_frac[400];        // position of bin inside its Opus band, j / band_size
  int bin_band[400];          // band index of every bin below 20 kHz
  int eband[24];              // band edges in 4-bin chunks (22 used)
  // band_sum (rn_kernels.hip): one piece of a half-band per lane; built and described in rn_band_piece.h
  int band_piece[64];
  // The twiddles of one butterfly of the radix-8, radix-3 and radix-5 passes of the 480-point transform, side by side:
  // copies of w960 entries, so that a lane fetches them with 16-byte loads from ONE row address (rn_twiddle_rows.h)
  alignas(16) float2 tw8[4][8];     // [k][r] = w960[30 k r]   (r = 0: unused)
  alignas(16) float2 tw3[32][2];    // [k][r - 1] = w960[10 k r]
  alignas(16) float2 tw5[96][4];    // [k][r - 1] = w960[2 k r]
};

// Flat blob offsets.
struct RnBlob {
  static constexpr int ID_W = 0, ID_B = ID_W + 42 * 24;
  static constexpr int VG_W = ID_B + 24, VG_R = VG_W + 24 * 72, VG_B = VG_R + 24 * 72;
  static constexpr int VO_W = VG_B + 72, VO_B = VO_W + 24;
  static constexpr int NG_W = VO_B + 1, NG_R = NG_W + 90 * 144, NG_B = NG_R + 48 * 144;
  static constexpr int DG_W = NG_B + 144, DG_R = DG_W + 114 * 288, DG_B = DG_R + 96 * 288;
  static constexpr int DO_W = DG_B + 288, DO_B = DO_W + 96 * 22;
  static constexpr int END = DO_B + 22;
};
static_assert(RnBlob::END == RN_WEIGHT_BYTES, "blob layout");

// Repacked weights: every matrix [K][rows] int8 becomes f16 (int8 values are exact in f16) in units of
// 8 halfs = 16 bytes, laid out [ceil(K/8)][rows][8]: lane == row reads one coalesced 16-byte vector per
// 8 MACs and each MAC is a single v_fma_mix_f32.  Biases are widened to float.
// Matrix offsets are in 16-byte units from the pack base, bias offsets in floats from the pack base.
constexpr int rn_k8(int k) { return (k + 7) / 8; }
struct RnPack {
  static constexpr int ID_W = 0;                               // K=42  rows=24
  static constexpr int VG_W = ID_W + rn_k8(42) * 24;           // K=24  rows=72
  static constexpr int VG_R = VG_W + rn_k8(24) * 72;           // K=24  rows=72
  static constexpr int VO_W = VG_R + rn_k8(24) * 72;           // K=24  rows=1
  static constexpr int NG_W = VO_W + rn_k8(24) * 1;            // K=90  rows=144
  static constexpr int NG_R = NG_W + rn_k8(90) * 144;          // K=48  rows=144
  static constexpr int DG_W = NG_R + rn_k8(48) * 144;          // K=114 rows=288
  static constexpr int DG_R = DG_W + rn_k8(114) * 288;         // K=96  rows=288
  static constexpr int DO_W = DG_R + rn_k8(96) * 288;          // K=96  rows=22
  static constexpr int MAT_END = DO_W + rn_k8(96) * 22;        // 16-byte units
  // float biases (offsets in floats)
  static constexpr int ID_B = MAT_END * 4;
  static constexpr int VG_B = ID_B + 24;
  static constexpr int VO_B = VG_B + 72;
  static constexpr int NG_B = VO_B + 1;
  static constexpr int DG_B = NG_B + 144;
  static constexpr int DO_B = DG_B + 288;
  static constexpr int END = DO_B + 22;                        // total size in dwords
};

// Second copy of the matrices for the int8 MFMA form of the gain network (rn_kernels.hip, RN_GRU_MFMA == 2):
// the int8 values as they are, [ceil(K/16)][rows][16] -- lane == row reads one 16-byte vector per 16 MACs, half
// the bytes of the f16 pack through the CU's vector L1, which is what bounds that stage.  Appended to the same
// buffer; offsets in 16-byte units from the pack base.
constexpr int rn_k16(int k) { return (k + 15) / 16; }
struct RnPack8 {
  static constexpr int ID_W = (RnPack::END + 3) / 4;             // K=42  rows=24
  static constexpr int VG_W = ID_W + rn_k16(42) * 24;            // K=24  rows=72
  static constexpr int VG_R = VG_W + rn_k16(24) * 72;            // K=24  rows=72
  static constexpr int NG_W = VG_R + rn_k16(24) * 72;            // K=90  rows=144
  static constexpr int NG_R = NG_W + rn_k16(90) * 144;           // K=48  rows=144
  static constexpr int DG_W = NG_R + rn_k16(48) * 144;           // K=114 rows=288
  static constexpr int DG_R = DG_W + rn_k16(114) * 288;          // K=96  rows=288
  static constexpr int DO_W = DG_R + rn_k16(96) * 288;           // K=96  rows=22
  static constexpr int MAT_END = DO_W + rn_k16(96) * 22;         // 16-byte units
  static constexpr int END = MAT_END * 4;                        // total size of the buffer in dwords
};

// Kernel arguments of one enqueue (chunk of T frames for all B streams).
struct RnArgs {
  // audio
  const float* in;      // caller layout
  float* out;           // caller layout
  long stride_t, stride_b;  // element strides of (frame, stream) in `in`/`out`
  // int16 sample transport (crispy_rn_process_s16*): `in` / `out` point at int16_t samples (same ELEMENT strides).
  // in_s16: the high-pass reads (float)s -- what the reference's i16 capture path feeds process_frame: s / 32768 (audio.rs:814)
  // x 32768 (audio.rs:264), both exact.  out_s16: the frame kernel stores trunc(clamp(y / 32768, -1, 1) x 32767) -- the
  // adapter's / 32768 + clamp (audio.rs:270-273) and the WAV writer's quantisation (recording.rs:109-110).
  int in_s16, out_s16;
  float* vad;           // [T][B] or null
  float* taps;          // [T][B][72] or null
  float* dbg;           // [B][RN_DBG_FLOATS] or null (last frame of the call)
  int T, B;
  // workspace: high-passed signal, per stream contiguous: [B][xhp_stride], first RN_HIST = history
  float* xhp;
  long xhp_stride;
  // persistent per-stream state (HBM)
  float* hp_mem;        // [B][2]
  float* synth;         // [B][480] overlap-add tails, read at the start of a launch and written at its end
  float* ceps;          // [B][8*22]
  float* lastg;         // [B][22]
  float* rnn;           // [B][168]
  float* last_gain;     // [B]
  int* last_period;     // [B]
  int* memid;           // [B]
  // constants
  const RnTables* tab;
  const uint32_t* wpack;
};

hipError_t rn_launch_highpass(const RnArgs& a, hipStream_t s, bool deep = false);   // deep: 32 samples requested ahead (few streams)
hipError_t rn_launch_frames(const RnArgs& a, hipStream_t s, int waves_per_stream = 1);   // the frame: analysis + gain network + synthesis
hipError_t rn_launch_roll_history(const RnArgs& a, hipStream_t s);
hipError_t rn_launch_tansig(const RnTables* tab, const float* x, float* y, long n, int sigmoid, hipStream_t s);

// ---- crispy_rn_push*: RnnNoiseProcessor::push_sample around the frame kernels (rn_adapter.hip) ----
// One push of n_in capture samples per stream.  The 48 kHz sequence of the push is, per stream, the `carry_len` samples
// left over from the previous push followed by `n_new` new ones: the capture samples themselves (idx == nullptr, rates
// within 1 Hz) or LinearResampler outputs -- new sample r interpolates capture samples idx[r] - 1 and idx[r] of this push
// (idx[r] == 0: the previous push's last sample) at t[r]; both arrays are the same for every stream of the handle.  The
// first `frames` x 480 of them go x32768 to `stage` (and `frames48`), the rest, unscaled, to carry_new.
struct RnAdaptIn {
  const float* in;         // [B][in_stride]
  long in_stride;
  long n_in;
  const int* idx;          // [n_new] or null
  const float* t;          // [n_new]
  int carry_len;           // < 480
  long n_new;
  int frames;
  const float* carry_old;  // [B][480]
  float* carry_new;        // [B][480]
  const float* last_old;   // [B]
  float* last_new;         // [B]: in[b][n_in - 1]
  float* stage;            // [B][frames * 480]: what the frame kernels read as a stream-major (BTF) tensor
  float* frames48;         // [B][frames_stride] or null
  long frames_stride;
  int B;
};
// d_out[b][r] = clamp(y[b][skip + r] / 32768, -1, 1) * volume for r < n_out (a multiple of 480)
struct RnAdaptOut {
  const float* y;          // [B][y_stride], 16-byte aligned rows
  long y_stride;
  long skip;               // 480 while the first frame is dropped, else 0
  float* out;              // [B][out_stride]
  long out_stride;
  long n_out;
  float volume;
  int B;
};
hipError_t rn_launch_adapt_in(const RnAdaptIn& a, hipStream_t s);
hipError_t rn_launch_adapt_out(const RnAdaptOut& a, hipStream_t s);

// ---- crispy_rn_pull* (rn_playback.hip) and crispy_rn_record_* / crispy_rn_level* (rn_record.hip) ----
struct RnRingAppend {
  const float* src;    // [B][src_stride]: the rows the push has just written, from the first sample that is kept
  long src_stride;
  float* ring;         // [B][cap]
  int cap;
  int tail;            // where the first sample goes, < cap
  int n;               // samples per stream, <= cap
  int B;
};

struct RnPull {
  const float* ring;   // [B][cap]
  int cap;
  int head;            // ring index of output_buf[0] at the start of the pull, < cap
  const int* off;      // [n_frames]: samples popped since the start of the pull (< cap - 1); < 0: an underrun, the frame is 0.0
  const float* frac;   // [n_frames]: resample_pos as f32
  void* out;           // [B][out_stride] elements of the format
  long out_stride;
  unsigned n_frames;
  unsigned n_elems;    // n_frames x channels, <= 2^27
  unsigned channels;
  int B;
};

constexpr int REC_FRAME = 1152;                     // the recording worker's frame_size

struct RnRecApp {
  const float* in;     // [B][in_stride]: frames of `channels` interleaved samples, from the first frame that is kept
  long in_stride;
  float* ring;         // [B][cap]
  int cap;
  int tail;            // where the first frame's sample goes, < cap
  int n;               // frames per stream, <= cap
  int channels;        // 1...8
  int B;
};

struct RnRecDrain {
  const float* mic;    // [B][cap]
  const float* app;    // [B][cap]
  int cap;
  int mic_head;        // ring index of the deque's front at the start of the drain, < cap
  int app_head;
  const int* mic_off;  // [n_frames]: samples popped from the mic deque before this frame's 1152 (offset + 1152 <= cap)
  const int* app_off;  // [n_frames]: the same for the app deque; < 0: fewer than 1152 were there, the frame's app samples are 0.0
  void* out;           // [B][out_stride] elements of the format
  long out_stride;
  unsigned n_samples;  // n_frames x 1152
  int B;
};

struct RnLevel {
  const float* in;     // [B][in_stride]
  long in_stride;
  int n;               // samples per stream, 1...2^24
  float* rms;          // [B]
  int B;
};

// format: a crispy_pcm_format (include/crispy_hip.h) -- pull: f32 / i16 / u16; drain: i16 (stereo frames, L == R) / f32 (channel 0)
hipError_t rn_launch_ring_append(const RnRingAppend& a, hipStream_t s);
hipError_t rn_launch_pull(const RnPull& a, int format, hipStream_t s);
hipError_t rn_launch_rec_app(const RnRecApp& a, hipStream_t s);
hipError_t rn_launch_rec_drain(const RnRecDrain& a, int format, hipStream_t s);
hipError_t rn_launch_level(const RnLevel& a, hipStream_t s);

// ---- crispy_rn_capture* / crispy_rn_record_app_push_at* (rn_capture.hip) ----
// The capture callbacks' first statement (audio.rs:754-755, 816-818, 880-883): per frame, the samples converted to f32 and
// `iter().sum::<f32>() / input_channels as f32`.
struct RnCapture {
  const void* in;      // [B][in_stride] elements of the format: frames of `channels` interleaved samples
  long in_stride;
  int n;               // frames per stream, 1...2^24
  int channels;        // 1...8
  float* mono;         // [B][mono_stride]
  long mono_stride;
  int B;
};

// The bypass arm's LinearResampler (audio.rs:108-133, 711-714) over the mono of one capture: output r interpolates mono samples
// idx[r] - 1 and idx[r] (idx[r] == 0: the previous capture's last sample) at t[r]; idx == nullptr: the resampler passes
// through, out = mono.  Both arrays are the same for every stream of the handle.
struct RnCaptureResample {
  const float* mono;       // [B][mono_stride]
  long mono_stride;
  int n_in;                // mono samples per stream, >= 1
  const int* idx;          // [n_out] or null
  const float* t;          // [n_out]
  const float* last_old;   // [B]
  float* last_new;         // [B]: mono[b][n_in - 1]
  float* out;              // [B][out_stride]
  long out_stride;
  long n_out;              // may be 0 (the capture that primes the resampler)
  int B;
};

// resample_audio (src-tauri/src/recording.rs:13-39) of the downmixed frames + append to the app ring: kept output j is output
// skip + j of the buffer, at src_pos = (skip + j) as f64 * ratio.
struct RnRecAppAt {
  const float* in;     // [B][in_stride]: n_in frames of `channels` interleaved samples
  long in_stride;
  int n_in;            // frames per stream, 1...2^24
  int channels;        // 1...8
  double ratio;        // from_rate as f64 / 48000 as f64
  long skip;           // outputs of this buffer that the ring's eviction drops at the front
  float* ring;         // [B][cap]
  int cap;
  int tail;            // where the first kept output goes, < cap
  int n;               // outputs kept per stream, 1...cap; floor((skip + n - 1) * ratio) < n_in
  int B;
};

hipError_t rn_launch_capture(const RnCapture& a, int format, hipStream_t s);       // format: f32 / i16 / u16
hipError_t rn_launch_capture_resample(const RnCaptureResample& a, hipStream_t s);
hipError_t rn_launch_rec_app_at(const RnRecAppAt& a, hipStream_t s);

// ---- the Legacy arm of NsState: SharedAudio (src-tauri/src/audio.rs:136-200) on crispy_rn_push* / crispy_rn_pull* (rn_legacy.hip) ----
// SharedAudio's noise source is the LCG  rng = rng * 1664525 + 1013904223  (wrapping u32), one step per noisy sample.  2^j
// steps are the affine map x -> a[j] * x + c[j]: n steps are one multiply-add per set bit of n, on the host (the handle's copy
// of the state, crispy_ns_noise_state) and in the kernels (a lane's own starting state) alike.  Nothing is carried serially.
constexpr uint32_t NS_LCG_A = 1664525u, NS_LCG_C = 1013904223u, NS_LCG_SEED = 0x1234abcdu;
struct NsLcgPowers {
  uint32_t a[32], c[32];
};
constexpr NsLcgPowers ns_lcg_powers() {
  NsLcgPowers p{};
  uint32_t a = NS_LCG_A, c = NS_LCG_C;
  for (int j = 0; j < 32; ++j) {
    p.a[j] = a;
    p.c[j] = c;
    c = (a + 1u) * c;       // f(f(x)) = a (a x + c) + c
    a = a * a;
  }
  return p;
}
__host__ __device__ inline uint32_t ns_lcg_step(uint32_t s) { return s * NS_LCG_A + NS_LCG_C; }
// Bits LO ... HI - 1 of n: the state n & (2^HI - 2^LO) steps on.  Unrolled, the powers are immediates.
template <int LO, int HI>
__host__ __device__ inline uint32_t ns_lcg_jump_bits(uint32_t s, uint32_t n) {
  constexpr NsLcgPowers P = ns_lcg_powers();
#pragma unroll
  for (int j = LO; j < HI; ++j)
    if ((n >> j) & 1u) s = s * P.a[j] + P.c[j];
  return s;
}
__host__ __device__ inline uint32_t ns_lcg_jump(uint32_t s, uint32_t n) { return ns_lcg_jump_bits<0, 32>(s, n); }
// `(rng as f32 / u32::MAX as f32) * 2.0 - 1.0`: the conversion rounds to nearest even, u32::MAX as f32 is 2^32, so the division
// is an exact scaling (written as the multiply by 2^-32), as is the doubling; the subtraction rounds.  +1.0 from 0xffffff80 on.
__host__ __device__ inline float ns_noise(uint32_t s) {
#pragma clang fp contract(off)
  const float u = (float)s;
  const float q = u * 0x1p-32f;
  const float d = q * 2.0f;
  return d - 1.0f;
}

// One Legacy push of n samples per stream: out[b][k] = in[b][k] * volume, Noisy: + noise(step k + 1 from rng) * 0.05 -- every
// operation rounded on its own --, and the raw in[b][k] of the samples skip ... n - 1 into the playback ring from `tail` on.
struct RnLegacyPush {
  const float* in;     // [B][in_stride]
  long in_stride;
  int n;               // samples per stream, 1...2^24
  float* out;          // [B][out_stride]
  long out_stride;
  float volume;
  uint32_t rng;        // rng_state in front of the push (Noisy)
  float* ring;         // [B][cap] or null: no playback configured
  int cap;
  int tail;            // where sample `skip` goes, < cap
  int skip;            // samples at the front that the ring's eviction drops; n - skip <= cap
  bool ring_vec;       // set by the launcher: every ring row is 16-byte aligned
  int B;
};
// One Legacy pull: RnPull's gather and interpolation, Noisy: + noise(step j + 1 from rng) * 0.05 for live frame j -- the live
// frames of a pull are a prefix of it, so j is the frame's index --, then x volume, the conversion and the fan-out.
struct RnLegacyPull {
  RnPull p;
  float volume;
  uint32_t rng;        // rng_state in front of the pull (Noisy)
};
hipError_t rn_launch_legacy_push(const RnLegacyPush& a, bool noisy, hipStream_t s);
hipError_t rn_launch_legacy_pull(const RnLegacyPull& a, int format, bool noisy, hipStream_t s);

// A launch covers at most 2^23 workgroups (the runtime refuses 2^32 work-items per grid dimension and more): a handle of
// several hundred thousand streams is covered in turns of streams, each turn with its own row pointers.
// launch(b0, nb): the kernel for streams b0 ... b0 + nb - 1, `tiles` (<= RN_MAX_BLOCKS) workgroups each.
constexpr long RN_MAX_BLOCKS = 1L << 23;
template <class Launch>
inline void rn_for_stream_groups(long B, long tiles, Launch launch) {
  const long per = RN_MAX_BLOCKS / tiles;                  // streams per launch
  for (long b0 = 0; b0 < B; b0 += per) launch(b0, (int)(B - b0 < per ? B - b0 : per));
}

}  // namespace crispy

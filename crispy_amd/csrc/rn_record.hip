// rn_record.hip -- crispy_rn_record_* / crispy_rn_level*: the recording leg of the live path for every stream of a handle at
// once.  push_mono_to_buffers appends what push_sample returned to the 48 kHz recording ring (src-tauri/src/audio.rs:701-726)
// and accumulates the level meter (audio.rs:728-729, 779-781); the app-audio handlers downmix their frames into a second ring;
// the recording worker pops 1152-sample frames from both, keeps them within 50 ms of each other and adds them
// (src-tauri/src/commands/recording.rs:196-264); WavWriter::write_samples quantises to interleaved s16
// (src-tauri/src/recording.rs:101-118).
//   (ring append)          the samples a push returned into the mic ring: the append kernel of rn_playback.hip
//   rn_rec_app_kernel      downmix of `channels` interleaved samples per frame + append to the app ring, one pass
//   rn_rec_drain_kernel    per output sample: gather from both rings modulo cap, mix (one f32 add), quantise; a stereo frame
//                          is one 32-bit word q | q << 16 (s16) or the f32 `q / 32768` of channel 0
//   rn_level_kernel        (sum of mono * mono / frames).sqrt(), the sum strictly in sample order: a lane owns a stream
// Ring heads and lengths, the worker's trims and the frame count live on the host: the streams of a handle are pushed in lock
// step, so they are the same for all of them and do not depend on the samples.  crispy_record_worker_plan is the worker loop on
// lengths alone; a drain uploads one (mic offset, app offset) pair per frame.
// The reference rounds every operation (Rust never contracts) and hipcc fuses a * b + c by default: contraction is off for the
// whole file.  The fused multiply-adds that remain in the ISA are those of the correctly rounded f32 division and square root,
// which the hardware has as refinement sequences only (tests/test_record_host.py tells the two apart).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "api_util.h"
#include "rn_common.h"
#include "rn_handle.h"

#pragma clang fp contract(off)

namespace crispy {
namespace {

constexpr int REC_THREADS = 256;
constexpr int REC_TILE = REC_THREADS * 4;           // samples per workgroup of the app pass and of the drain
constexpr long REC_MAX_BLOCKS = 1L << 23;           // per launch: a handle of very many streams goes in turns
constexpr int REC_FRAME = 1152;                     // the worker's frame_size
constexpr long REC_MAX_DESYNC = 2400;               // (SAMPLE_RATE / 20).max(frame_size): 50 ms at 48 kHz
constexpr long REC_DEFAULT_CAP = 48000L * 10;       // recording::SAMPLE_RATE * 10
constexpr long REC_MAX_CAP = 1L << 28;              // ring indices and the elements of a drained row stay inside 32 bits
constexpr long kLevelMaxIn = 1L << 24;              // samples per stream and call: the f32 count is exact
constexpr int LV_STREAMS = 64;                      // streams per workgroup of the level pass: a lane of its first wave each
constexpr int LV_THREADS = 256;                     // four waves load, the first one sums
constexpr int LV_SAMPLES = 128;                     // samples per tile
constexpr int LV_PITCH = LV_SAMPLES + 1;            // LDS row pitch: lanes that read a column fall on different banks
constexpr int LV_ROWS_PER_THREAD = LV_STREAMS * LV_SAMPLES / LV_THREADS;      // 32

__host__ __device__ inline long rec_tiles(long n, long tile) { return n > 0 ? (n + tile - 1) / tile : 1; }

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

// The capture handlers' downmix.  1 channel: the sample itself; 2: (f0 + f1) / 2.0; more: `iter().sum::<f32>()`, which starts
// from 0.0 and adds in order, then `/ channels as f32`.  Every add rounds on its own and the division is correctly rounded.
__device__ __forceinline__ float app_downmix(const float* f, int channels) {
  if (channels == 1) return f[0];
  if (channels == 2) return (f[0] + f[1]) / 2.0f;
  float acc = 0.0f;
  for (int c = 0; c < channels; ++c) acc = acc + f[c];
  return acc / (float)channels;
}

// A lane's four frames are 256 apart, so that every store of a wave covers consecutive ring addresses wherever the tail stands.
__global__ __launch_bounds__(REC_THREADS) void rn_rec_app_kernel(RnRecApp a) {
  const unsigned tiles = (unsigned)rec_tiles(a.n, REC_TILE);
  const long b = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x - (unsigned)b * tiles) * REC_TILE;
  const float* in = a.in + b * a.in_stride;
  float* ring = a.ring + b * a.cap;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = tile0 + e * REC_THREADS + (int)threadIdx.x;
    if (r < a.n) {
      int i = a.tail + r;          // < 2 x cap
      if (i >= a.cap) i -= a.cap;
      ring[i] = app_downmix(in + (long)r * a.channels, a.channels);
    }
  }
}

__device__ __forceinline__ float rec_clamp_pm1(float s) { return s < -1.f ? -1.f : (s > 1.f ? 1.f : s); }     // f32::clamp: a NaN stays a NaN

// `(mixed.clamp(-1.0, 1.0) * 32767.0) as i16` (recording.rs:109-110): Rust's `as` truncates toward zero and makes a NaN 0.
__device__ __forceinline__ int rec_quantise(float mixed) {
  const float x = rec_clamp_pm1(mixed) * 32767.f;
  return mixed != mixed ? 0 : (int)x;         // |x| <= 32767
}

// Sample j of the drain, j = frame x 1152 + k: left_frame[k] + right_frame[k] of that frame, quantised.
__device__ __forceinline__ int drain_sample(const RnRecDrain& a, const float* mic, const float* app, unsigned j) {
  const unsigned f = j / REC_FRAME;
  const int k = (int)(j - f * REC_FRAME);
  int im = a.mic_head + a.mic_off[f] + k;       // < 2 x cap
  if (im >= a.cap) im -= a.cap;
  const int ao = a.app_off[f];
  float right = 0.0f;
  if (ao >= 0) {
    int ia = a.app_head + ao + k;
    if (ia >= a.cap) ia -= a.cap;
    right = app[ia];
  }
  const float mixed = mic[im] + right;
  return rec_quantise(mixed);
}

// What the drain writes per sample: the WAV payload's stereo frame (L == R) or channel 0 as run_transcription reads it back.
template <int FMT> struct RecOut;
template <> struct RecOut<CRISPY_PCM_I16> {
  using T = int16_t;
  static constexpr int EPS = 2;       // elements per sample
  static __device__ __forceinline__ uint32_t word(int q) { const uint32_t u = (uint32_t)q & 0xffffu; return u | (u << 16); }
  static __device__ __forceinline__ T elem(int q) { return (int16_t)q; }
};
template <> struct RecOut<CRISPY_PCM_F32> {
  using T = float;
  static constexpr int EPS = 1;
  static __device__ __forceinline__ uint32_t word(int q) { return __float_as_uint((float)q / 32768.0f); }
  static __device__ __forceinline__ T elem(int q) { return (float)q / 32768.0f; }
};

// A row of `out` is n_samples x EPS elements.  Either format makes one 32-bit word per sample.
// VEC: every row is 16-byte aligned (pointer and stride): a lane takes four consecutive samples -- n_samples is a multiple of
// four -- and stores their words as one 16-byte store.  Otherwise a lane's elements are 256 apart, so that a wave's store still
// covers consecutive addresses, and rows may start on any element.
template <int FMT, bool VEC>
__global__ __launch_bounds__(REC_THREADS) void rn_rec_drain_kernel(RnRecDrain a) {
  using O = RecOut<FMT>;
  using T = typename O::T;
  const unsigned tiles = (unsigned)rec_tiles(a.n_samples, REC_TILE);
  const long b = blockIdx.x / tiles;
  const unsigned tile0 = (blockIdx.x - (unsigned)b * tiles) * REC_TILE;
  const float* mic = a.mic + b * a.cap;
  const float* app = a.app + b * a.cap;
  T* out = reinterpret_cast<T*>(a.out) + b * a.out_stride;
  if (VEC) {
    const unsigned j0 = tile0 + threadIdx.x * 4;
    if (j0 >= a.n_samples) return;
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = O::word(drain_sample(a, mic, app, j0 + e));
    *reinterpret_cast<uint4*>(reinterpret_cast<uint32_t*>(out) + j0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    const unsigned n_elems = a.n_samples * O::EPS;
#pragma unroll
    for (int e = 0; e < 4 * O::EPS; ++e) {
      const unsigned i = tile0 * O::EPS + e * REC_THREADS + threadIdx.x;
      if (i < n_elems) out[i] = O::elem(drain_sample(a, mic, app, i / O::EPS));
    }
  }
}

// The callback's level meter: sum starts at 0.0, `sum += mono * mono` in sample order with the multiply and the add rounded
// separately, frames counts in f32 (exact up to 2^24), `(sum / frames).sqrt()`.  The sum of a stream is a serial chain, so a
// lane owns a stream and a wave covers 64 of them: the first wave of the workgroup.  All four waves load: a tile of 64 streams
// x 128 samples goes through registers -- lanes along the samples, 32 row pieces of 256 contiguous bytes per wave -- into LDS
// and is read back transposed; rows are 129 words apart, so the 64 lanes of a column read fall on 32 different banks twice
// over instead of on one.  The loads of the next tile are issued before the chain over the current one and land during it.
// Rows and columns past the end are loaded from the last valid one (the address is clamped, nothing reads them back).
__global__ __launch_bounds__(LV_THREADS) void rn_level_kernel(RnLevel a) {
  __shared__ float tile[LV_STREAMS * LV_PITCH];
  const int tid = (int)threadIdx.x;
  const int col = tid & (LV_SAMPLES - 1);
  const int half = tid / LV_SAMPLES;              // this thread loads rows half, half + 2, ...
  const long b0 = (long)blockIdx.x * LV_STREAMS;
  const int rows = (int)(a.B - b0 < LV_STREAMS ? a.B - b0 : LV_STREAMS);
  const float* in = a.in + b0 * a.in_stride;
  float pre[LV_ROWS_PER_THREAD];
#pragma unroll
  for (int i = 0; i < LV_ROWS_PER_THREAD; ++i) {
    const int r = half + 2 * i;
    pre[i] = in[(r < rows ? r : rows - 1) * a.in_stride + (col < a.n ? col : a.n - 1)];
  }
  float sum = 0.0f;
  for (int t0 = 0; t0 < a.n; t0 += LV_SAMPLES) {
#pragma unroll
    for (int i = 0; i < LV_ROWS_PER_THREAD; ++i) tile[(half + 2 * i) * LV_PITCH + col] = pre[i];
    __syncthreads();
    const int t1 = t0 + LV_SAMPLES;
    if (t1 < a.n) {
#pragma unroll
      for (int i = 0; i < LV_ROWS_PER_THREAD; ++i) {
        const int r = half + 2 * i;
        pre[i] = in[(r < rows ? r : rows - 1) * a.in_stride + (t1 + col < a.n ? t1 + col : a.n - 1)];
      }
    }
    if (tid < rows) {
      const int cols = a.n - t0 < LV_SAMPLES ? a.n - t0 : LV_SAMPLES;
      for (int k = 0; k < cols; ++k) {
        const float mono = tile[tid * LV_PITCH + k];
        const float sq = mono * mono;
        sum = sum + sq;
      }
    }
    __syncthreads();
  }
  if (tid < rows) {
    const float frames = (float)a.n;
    const float mean = sum / frames;
    a.rms[b0 + tid] = sqrtf(mean);
  }
}

hipError_t launch_app(const RnRecApp& a, hipStream_t s) {
  const long tiles = rec_tiles(a.n, REC_TILE);            // <= 2^18
  const long per = REC_MAX_BLOCKS / tiles;                // streams per launch
  for (long b0 = 0; b0 < a.B; b0 += per) {
    RnRecApp c = a;
    c.B = (int)(a.B - b0 < per ? a.B - b0 : per);
    c.in += b0 * a.in_stride;
    c.ring += b0 * a.cap;
    hipLaunchKernelGGL(rn_rec_app_kernel, dim3((unsigned)(c.B * tiles)), dim3(REC_THREADS), 0, s, c);
  }
  return hipGetLastError();
}

template <int FMT>
hipError_t launch_drain_fmt(const RnRecDrain& a, hipStream_t s) {
  using T = typename RecOut<FMT>::T;
  const long tiles = rec_tiles(a.n_samples, REC_TILE);    // <= 2^18
  const long per = REC_MAX_BLOCKS / tiles;
  const bool vec = (((uintptr_t)a.out | (uintptr_t)(a.out_stride * (long)sizeof(T))) & 15) == 0;
  for (long b0 = 0; b0 < a.B; b0 += per) {
    RnRecDrain c = a;
    c.B = (int)(a.B - b0 < per ? a.B - b0 : per);
    c.mic += b0 * a.cap;
    c.app += b0 * a.cap;
    c.out = reinterpret_cast<T*>(a.out) + b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL((rn_rec_drain_kernel<FMT, true>), grid, dim3(REC_THREADS), 0, s, c);
    else hipLaunchKernelGGL((rn_rec_drain_kernel<FMT, false>), grid, dim3(REC_THREADS), 0, s, c);
  }
  return hipGetLastError();
}

hipError_t launch_level(const RnLevel& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.B + LV_STREAMS - 1) / LV_STREAMS);
  hipLaunchKernelGGL(rn_level_kernel, dim3(blocks), dim3(LV_THREADS), 0, s, a);
  return hipGetLastError();
}

inline size_t rec_elem_bytes(int format) { return format == CRISPY_PCM_F32 ? 4 : 2; }
inline long rec_elems_per_frame(int format) { return format == CRISPY_PCM_F32 ? REC_FRAME : 2L * REC_FRAME; }

// One of the two deques as a ring: where the front is and how many samples it holds.
struct RingPos {
  int head = 0;
  int len = 0;
};

// Appending n samples to a ring of cap (audio.rs:719-724: the oldest sample is dropped for each one that does not fit):
// how many of the n are skipped at the front, where the first one kept goes, and the ring's position afterwards.
struct AppendPlan {
  long skip = 0;
  int n = 0;
  int tail = 0;
  RingPos after;
};
AppendPlan plan_append(const RingPos& r, int cap, long n) {
  AppendPlan p;
  if (n >= cap) {                    // everything that was there is evicted, and the front of this block with it
    p.skip = n - cap;
    p.n = cap;
    p.tail = 0;
    p.after.head = 0;
    p.after.len = cap;
  } else {
    p.n = (int)n;
    p.tail = (int)(((long)r.head + r.len) % cap);
    const long over = (long)r.len + n - cap;
    if (over > 0) {
      p.after.head = (int)(((long)r.head + over) % cap);
      p.after.len = cap;
    } else {
      p.after.head = r.head;
      p.after.len = r.len + (int)n;
    }
  }
  return p;
}

}  // namespace

// The recording state's two buffers (the mic ring that push_mono_to_buffers fills, the app ring of the capture handlers) for all
// streams of a handle, and the buffers of the host entry points.  The object is created on first use; the rings exist, and the
// handle records, from crispy_rn_record_configure on (cap > 0).
struct RnRecord {
  int cap = 0;
  RingPos mic, app;
  DevBuf<float> mic_ring;    // [B][cap]
  DevBuf<float> app_ring;
  DevBuf<int> d_off;         // (mic_off[n], app_off[n]) of the current drain
  int* h_off[2] = {nullptr, nullptr};     // pinned upload slots, used in turns; ev_off: the slot's copy has been read
  long h_off_cap[2] = {0, 0};
  hipEvent_t ev_off[2] = {nullptr, nullptr};
  int slot = 0;
  std::vector<long> mic_off, app_off;     // host scratch of one drain
  DevBuf<unsigned char> d_hout;           // crispy_rn_record_drain: device copy of the host array
  DevBuf<float> d_hin;                    // crispy_rn_record_app_push / crispy_rn_level: device copy of the host array
  DevBuf<float> d_hrms;
};

namespace {

// crispy_rn::rec_free (the caller has made the handle's device current and drained its stream)
void record_free(RnRecord* r) {
  for (int* q : r->h_off)
    if (q) (void)hipHostFree(q);
  for (hipEvent_t e : r->ev_off)
    if (e) (void)hipEventDestroy(e);
  delete r;
}

RnRecord* record_of(crispy_rn* h) {
  if (!h->rec) {
    h->rec = new RnRecord();       // (std::bad_alloc: the entry point's guard makes it CRISPY_ERR_OOM)
    h->rec_free = record_free;
  }
  return h->rec;
}

inline bool recording(const crispy_rn* h) { return h->rec && h->rec->cap > 0; }

int check_app_push(const crispy_rn* h, const float* in, long in_stride, long n_frames, int channels, const char* who) {
  if (!recording(h)) return fail(CRISPY_ERR_INVALID_ARG, "%s: recording not configured (crispy_rn_record_configure)", who);
  if (n_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames < 0", who);
  if (n_frames > kLevelMaxIn) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames %ld above the limit of %ld frames per push", who, n_frames, kLevelMaxIn);
  if (channels < 1 || channels > 8) return fail(CRISPY_ERR_INVALID_ARG, "%s: channels %d outside 1...8", who, channels);
  if (n_frames == 0) return CRISPY_OK;
  if (!in) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL audio pointer", who);
  if (in_stride < n_frames * channels)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than the %ld samples of this push", who, in_stride, n_frames * channels);
  return CRISPY_OK;
}

// Arguments checked (check_app_push), n_frames > 0, the handle's device current.
int app_push_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, hipStream_t s) {
  RnRecord* r = h->rec;
  const AppendPlan p = plan_append(r->app, r->cap, n_frames);
  RnRecApp a{};
  a.in = d_in + p.skip * channels;
  a.in_stride = in_stride;
  a.ring = r->app_ring.p;
  a.cap = r->cap;
  a.tail = p.tail;
  a.n = p.n;
  a.channels = channels;
  a.B = h->B;
  HIP_TRY(launch_app(a, s));
  r->app = p.after;
  return CRISPY_OK;
}

int check_level(const crispy_rn* h, const float* in, long in_stride, long n_in, const float* rms, const char* who) {
  (void)h;
  if (n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in < 0", who);
  if (n_in > kLevelMaxIn) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in %ld above the limit of %ld samples per call", who, n_in, kLevelMaxIn);
  if (n_in == 0) return CRISPY_OK;
  if (!in || !rms) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL pointer", who);
  if (in_stride < n_in) return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than n_in %ld", who, in_stride, n_in);
  return CRISPY_OK;
}

int level_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_rms, hipStream_t s) {
  RnLevel a{};
  a.in = d_in;
  a.in_stride = in_stride;
  a.n = (int)n_in;
  a.rms = d_rms;
  a.B = h->B;
  HIP_TRY(launch_level(a, s));
  return CRISPY_OK;
}

// The arguments every drain checks before it plans.
int check_drain(const crispy_rn* h, long max_frames, int format, const void* out, const long* n_frames, const char* who) {
  if (!recording(h)) return fail(CRISPY_ERR_INVALID_ARG, "%s: recording not configured (crispy_rn_record_configure)", who);
  if (max_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: max_frames < 0", who);
  if (format != CRISPY_PCM_F32 && format != CRISPY_PCM_I16) return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown format %d", who, format);
  if (!out || !n_frames) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL out / n_frames pointer", who);
  return CRISPY_OK;
}

// Frames a drain of at most max_frames would write now; with offsets, their positions (RnRecord::mic_off / app_off).
long plan_drain(RnRecord* r, long max_frames, bool offsets, long* mic_left, long* app_left) {
  long cap_frames = r->mic.len / REC_FRAME;
  if (cap_frames > max_frames) cap_frames = max_frames;
  if (offsets) {
    r->mic_off.resize((size_t)cap_frames);
    r->app_off.resize((size_t)cap_frames);
  }
  return crispy_record_worker_plan(r->mic.len, r->app.len, max_frames, offsets ? r->mic_off.data() : nullptr,
                                   offsets ? r->app_off.data() : nullptr, mic_left, app_left);
}

// Arguments checked (check_drain), the handle's device current.  stride_of(n): the row stride to use for n frames (the host
// form sizes its staging rows from it), or < 0 with the error recorded.
template <class StrideOf>
int drain_device_impl(crispy_rn* h, long max_frames, int format, StrideOf stride_of, long* n_frames, hipStream_t s, const char* who,
                      void** d_out_used, long* stride_used) {
  RnRecord* r = h->rec;
  long mic_left = 0, app_left = 0;
  const long n = plan_drain(r, max_frames, true, &mic_left, &app_left);
  if (n < 0) return (int)n;
  if (n == 0) {
    *n_frames = 0;
    return CRISPY_OK;
  }
  void* d_out = nullptr;
  long out_stride = 0;
  int rc = stride_of(n, &d_out, &out_stride);
  if (rc != CRISPY_OK) return rc;
  // nothing is launched on an offset that leaves what the ring holds
  for (long f = 0; f < n; ++f) {
    if (r->mic_off[f] < 0 || r->mic_off[f] + REC_FRAME > r->mic.len || (r->app_off[f] >= 0 && r->app_off[f] + REC_FRAME > r->app.len))
      return fail(CRISPY_ERR_HIP, "%s: frame %ld of the plan lies outside the rings (mic %ld of %d, app %ld of %d)", who, f, r->mic_off[f],
                  r->mic.len, r->app_off[f], r->app.len);
  }
  // every allocation first: a failure from here on returns with the handle's state as it was
  const size_t words = (size_t)2 * n;
  if (r->d_off.grow(words * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: offset buffer of %zu bytes failed", who, words * sizeof(int));
  }
  const int slot = r->slot;
  if (r->h_off_cap[slot] < (long)words) {
    int* fresh = nullptr;
    if (hipHostMalloc(&fresh, words * sizeof(int), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: pinned allocation of %zu bytes failed", who, words * sizeof(int));
    }
    if (r->ev_off[slot]) HIP_TRY(hipEventSynchronize(r->ev_off[slot]));
    if (r->h_off[slot]) (void)hipHostFree(r->h_off[slot]);
    r->h_off[slot] = fresh;
    r->h_off_cap[slot] = (long)words;
  }
  if (!r->ev_off[slot]) HIP_TRY(hipEventCreateWithFlags(&r->ev_off[slot], hipEventDisableTiming));

  // ---- enqueue ----
  HIP_TRY(hipEventSynchronize(r->ev_off[slot]));      // the upload that used this slot two drains ago (no-op before)
  for (long f = 0; f < n; ++f) {
    r->h_off[slot][f] = (int)r->mic_off[f];
    r->h_off[slot][n + f] = (int)r->app_off[f];
  }
  HIP_TRY(hipMemcpyAsync(r->d_off.p, r->h_off[slot], words * sizeof(int), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(r->ev_off[slot], s));
  r->slot = slot ^ 1;
  RnRecDrain a{};
  a.mic = r->mic_ring.p;
  a.app = r->app_ring.p;
  a.cap = r->cap;
  a.mic_head = r->mic.head;
  a.app_head = r->app.head;
  a.mic_off = r->d_off.p;
  a.app_off = r->d_off.p + n;
  a.out = d_out;
  a.out_stride = out_stride;
  a.n_samples = (unsigned)(n * REC_FRAME);
  a.B = h->B;
  HIP_TRY(format == CRISPY_PCM_I16 ? launch_drain_fmt<CRISPY_PCM_I16>(a, s) : launch_drain_fmt<CRISPY_PCM_F32>(a, s));
  r->mic.head = (int)(((long)r->mic.head + (r->mic.len - mic_left)) % r->cap);
  r->mic.len = (int)mic_left;
  r->app.head = (int)(((long)r->app.head + (r->app.len - app_left)) % r->cap);
  r->app.len = (int)app_left;
  *n_frames = n;
  if (d_out_used) *d_out_used = d_out;
  if (stride_used) *stride_used = out_stride;
  return CRISPY_OK;
}

}  // namespace

// what rn_adapter.hip uses of this file (rn_handle.h)
int rn_record_append_mic(crispy_rn* h, const float* d_rows, long stride, long n, hipStream_t s) {
  if (!recording(h) || n <= 0) return CRISPY_OK;
  RnRecord* r = h->rec;
  const AppendPlan p = plan_append(r->mic, r->cap, n);
  HIP_TRY(rn_launch_ring_append(d_rows + p.skip, stride, r->mic_ring.p, r->cap, p.tail, p.n, h->B, s));
  r->mic = p.after;
  return CRISPY_OK;
}

}  // namespace crispy

using namespace crispy;

extern "C" {

long crispy_record_worker_plan(long mic_len, long app_len, long max_frames, long* mic_off, long* app_off, long* mic_left,
                               long* app_left) try {
  if (mic_len < 0 || app_len < 0 || max_frames < 0)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_record_worker_plan: negative length or frame count");
  long n = 0, mic_pop = 0, app_pop = 0;
  while (mic_len >= REC_FRAME && n < max_frames) {
    // align the heads when one source is more than 50 ms ahead (commands/recording.rs:221-239)
    if (mic_len > app_len + REC_MAX_DESYNC) {
      const long trim = mic_len - app_len - REC_MAX_DESYNC;
      mic_pop += trim;
      mic_len -= trim;
    } else if (app_len > mic_len + REC_MAX_DESYNC) {
      const long trim = app_len - mic_len - REC_MAX_DESYNC;
      app_pop += trim;
      app_len -= trim;
    }
    if (mic_off) mic_off[n] = mic_pop;
    mic_pop += REC_FRAME;
    mic_len -= REC_FRAME;
    if (app_len >= REC_FRAME) {
      if (app_off) app_off[n] = app_pop;
      app_pop += REC_FRAME;
      app_len -= REC_FRAME;
    } else if (app_off) {
      app_off[n] = -1;           // a frame of zeros; the app deque stays as it is
    }
    ++n;
  }
  if (mic_left) *mic_left = mic_len;
  if (app_left) *app_left = app_len;
  return n;
} CRISPY_CATCH_RET("crispy_record_worker_plan")

int crispy_rn_record_configure(crispy_rn* h, long ring_samples) try {
  const char* who = "crispy_rn_record_configure";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const long cap = ring_samples == 0 ? REC_DEFAULT_CAP : ring_samples;
  if (cap < 2 * REC_FRAME || cap > REC_MAX_CAP)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: ring_samples %ld outside %d...%ld (0 = %ld)", who, ring_samples, 2 * REC_FRAME, REC_MAX_CAP,
                REC_DEFAULT_CAP);
  HIP_TRY(hipSetDevice(h->device));
  RnRecord* r = record_of(h);
  if (cap != r->cap) {
    // both new rings before an old one goes: a failure leaves the handle as it was
    DevBuf<float> mic, app;
    const size_t bytes = (size_t)h->B * (size_t)cap * sizeof(float);
    if (mic.alloc(bytes) != hipSuccess || app.alloc(bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: ring allocation of 2 x %zu bytes failed", who, bytes);
    }
    r->mic_ring = std::move(mic);      // (the old ones are freed with the locals; hipFree waits for the work that still reads them)
    r->app_ring = std::move(app);
    r->cap = (int)cap;
  }
  r->mic = RingPos();
  r->app = RingPos();
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_configure")

int crispy_rn_record_buffered(const crispy_rn* h, long* mic, long* app) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_record_buffered: NULL handle");
  const bool on = recording(h);
  if (mic) *mic = on ? h->rec->mic.len : 0;
  if (app) *app = on ? h->rec->app.len : 0;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_buffered")

long crispy_rn_record_frames_ready(const crispy_rn* h) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_record_frames_ready: NULL handle");
  if (!recording(h)) return 0;
  return crispy_record_worker_plan(h->rec->mic.len, h->rec->app.len, 0x7fffffffffffffffL, nullptr, nullptr, nullptr, nullptr);
} CRISPY_CATCH_RET("crispy_rn_record_frames_ready")

int crispy_rn_record_app_push_device(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, void* hip_stream) try {
  const char* who = "crispy_rn_record_app_push_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_app_push(h, d_in, in_stride, n_frames, channels, who);
  if (rc != CRISPY_OK || n_frames == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return app_push_device_impl(h, d_in, in_stride, n_frames, channels, hip_stream ? (hipStream_t)hip_stream : h->stream);
} CRISPY_CATCH_RET("crispy_rn_record_app_push_device")

int crispy_rn_record_app_push(crispy_rn* h, const float* in, long in_stride, long n_frames, int channels) try {
  const char* who = "crispy_rn_record_app_push";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_app_push(h, in, in_stride, n_frames, channels, who);
  if (rc != CRISPY_OK || n_frames == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  RnRecord* r = h->rec;
  const size_t row = (size_t)n_frames * channels;
  if (r->d_hin.grow((size_t)h->B * row * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: staging allocation of %zu bytes failed", who, (size_t)h->B * row * sizeof(float));
  }
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(r->d_hin.p, row * sizeof(float), in, (size_t)in_stride * sizeof(float), row * sizeof(float), (size_t)h->B,
                           hipMemcpyHostToDevice, s));
  rc = app_push_device_impl(h, r->d_hin.p, (long)row, n_frames, channels, s);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_app_push")

int crispy_rn_level_device(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_rms, void* hip_stream) try {
  const char* who = "crispy_rn_level_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_level(h, d_in, in_stride, n_in, d_rms, who);
  if (rc != CRISPY_OK || n_in == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return level_device_impl(h, d_in, in_stride, n_in, d_rms, hip_stream ? (hipStream_t)hip_stream : h->stream);
} CRISPY_CATCH_RET("crispy_rn_level_device")

int crispy_rn_level(crispy_rn* h, const float* in, long in_stride, long n_in, float* rms) try {
  const char* who = "crispy_rn_level";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_level(h, in, in_stride, n_in, rms, who);
  if (rc != CRISPY_OK || n_in == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  RnRecord* r = record_of(h);
  const size_t B = (size_t)h->B;
  if (r->d_hin.grow(B * (size_t)n_in * sizeof(float)) != hipSuccess || r->d_hrms.grow(B * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: staging allocation of %zu bytes failed", who, B * (size_t)(n_in + 1) * sizeof(float));
  }
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(r->d_hin.p, (size_t)n_in * sizeof(float), in, (size_t)in_stride * sizeof(float), (size_t)n_in * sizeof(float), B,
                           hipMemcpyHostToDevice, s));
  rc = level_device_impl(h, r->d_hin.p, n_in, n_in, r->d_hrms.p, s);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rms, r->d_hrms.p, B * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_level")

int crispy_rn_record_drain_device(crispy_rn* h, long max_frames, int format, void* d_out, long out_stride, long* n_frames,
                                  void* hip_stream) try {
  const char* who = "crispy_rn_record_drain_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_drain(h, max_frames, format, d_out, n_frames, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  auto stride_of = [&](long n, void** p, long* stride) {
    if (out_stride < n * rec_elems_per_frame(format))
      return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld elements of this drain", who, out_stride,
                  n * rec_elems_per_frame(format));
    *p = d_out;
    *stride = out_stride;
    return (int)CRISPY_OK;
  };
  return drain_device_impl(h, max_frames, format, stride_of, n_frames, hip_stream ? (hipStream_t)hip_stream : h->stream, who, nullptr, nullptr);
} CRISPY_CATCH_RET("crispy_rn_record_drain_device")

int crispy_rn_record_drain(crispy_rn* h, long max_frames, int format, void* out, long out_stride, long* n_frames) try {
  const char* who = "crispy_rn_record_drain";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_drain(h, max_frames, format, out, n_frames, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  RnRecord* r = h->rec;
  const size_t eb = rec_elem_bytes(format);
  auto stride_of = [&](long n, void** p, long* stride) {
    const long elems = n * rec_elems_per_frame(format);        // a row is a multiple of 16 bytes: staging rows stay aligned
    if (out_stride < elems)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld elements of this drain", who, out_stride, elems);
    if (r->d_hout.grow((size_t)h->B * (size_t)elems * eb) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: staging allocation of %zu bytes failed", who, (size_t)h->B * (size_t)elems * eb);
    }
    *p = r->d_hout.p;
    *stride = elems;
    return (int)CRISPY_OK;
  };
  hipStream_t s = h->stream;
  long n = 0, stride = 0;
  void* d_out = nullptr;
  rc = drain_device_impl(h, max_frames, format, stride_of, &n, s, who, &d_out, &stride);
  if (rc != CRISPY_OK) return rc;
  if (n > 0) {
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * eb, d_out, (size_t)stride * eb, (size_t)stride * eb, (size_t)h->B,
                             hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  *n_frames = n;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_drain")

}  // extern "C"

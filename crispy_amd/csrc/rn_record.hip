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
// lengths alone; a drain uploads one (mic offset, app offset) pair per frame.  Both are host code: rn_io.cpp, which drives the
// kernels of this file through the launchers declared in rn_common.h.
// The reference rounds every operation (Rust never contracts) and hipcc fuses a * b + c by default: contraction is off for the
// whole file.  The fused multiply-adds that remain in the ISA are those of the correctly rounded f32 division and square root,
// which the hardware has as refinement sequences only (tests/test_record_host.py tells the two apart).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/crispy_hip.h"
#include "rn_common.h"
#include "rn_downmix.h"      // app_downmix: the capture handlers' downmix

#pragma clang fp contract(off)

namespace crispy {
namespace {

constexpr int REC_THREADS = 256;
constexpr int REC_TILE = REC_THREADS * 4;           // samples per workgroup of the app pass and of the drain
constexpr int LV_STREAMS = 64;                      // streams per workgroup of the level pass: a lane of its first wave each
constexpr int LV_THREADS = 256;                     // four waves load, the first one sums
constexpr int LV_SAMPLES = 128;                     // samples per tile
constexpr int LV_PITCH = LV_SAMPLES + 1;            // LDS row pitch: lanes that read a column fall on different banks
constexpr int LV_ROWS_PER_THREAD = LV_STREAMS * LV_SAMPLES / LV_THREADS;      // 32

__host__ __device__ inline long rec_tiles(long n, long tile) { return n > 0 ? (n + tile - 1) / tile : 1; }

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

}  // namespace

hipError_t rn_launch_rec_app(const RnRecApp& a, hipStream_t s) {
  const long tiles = rec_tiles(a.n, REC_TILE);            // <= 2^18
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnRecApp c = a;
    c.B = nb;
    c.in += b0 * a.in_stride;
    c.ring += b0 * a.cap;
    hipLaunchKernelGGL(rn_rec_app_kernel, dim3((unsigned)(c.B * tiles)), dim3(REC_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

namespace {
template <int FMT>
hipError_t launch_drain_fmt(const RnRecDrain& a, hipStream_t s) {
  using T = typename RecOut<FMT>::T;
  const long tiles = rec_tiles(a.n_samples, REC_TILE);    // <= 2^18
  const bool vec = (((uintptr_t)a.out | (uintptr_t)(a.out_stride * (long)sizeof(T))) & 15) == 0;
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnRecDrain c = a;
    c.B = nb;
    c.mic += b0 * a.cap;
    c.app += b0 * a.cap;
    c.out = reinterpret_cast<T*>(a.out) + b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL((rn_rec_drain_kernel<FMT, true>), grid, dim3(REC_THREADS), 0, s, c);
    else hipLaunchKernelGGL((rn_rec_drain_kernel<FMT, false>), grid, dim3(REC_THREADS), 0, s, c);
  });
  return hipGetLastError();
}
}  // namespace

hipError_t rn_launch_rec_drain(const RnRecDrain& a, int format, hipStream_t s) {
  return format == CRISPY_PCM_I16 ? launch_drain_fmt<CRISPY_PCM_I16>(a, s) : launch_drain_fmt<CRISPY_PCM_F32>(a, s);
}

hipError_t rn_launch_level(const RnLevel& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.B + LV_STREAMS - 1) / LV_STREAMS);
  hipLaunchKernelGGL(rn_level_kernel, dim3(blocks), dim3(LV_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace crispy

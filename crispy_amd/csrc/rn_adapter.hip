// rn_adapter.hip -- crispy_rn_push*: what RnnNoiseProcessor::push_sample (src-tauri/src/audio.rs:242-295) does per sample
// around process_frame, for one block of capture samples of every stream of a handle at once.  Kernels and their launchers
// (declared in rn_common.h); the entry points that drive them are rn_io.cpp.
//   rn_adapt_in_kernel    LinearResampler (audio.rs:108-133) + frame assembly: carried remainder, then the new 48 kHz samples,
//                         x32768 into the staging rows the high-pass reads; the new remainder into the carry buffer
//   (frame kernels)       the completed frames as one call through crispy_rn_process_device's enqueue path
//   rn_adapt_out_kernel   clamp(y / 32768, -1, 1) x volume (audio.rs:270-273), first frame skipped (audio.rs:275-278)
//   (ring append)         on a handle with playback configured: the returned samples into output_buf (rn_playback.hip);
//                         on a handle that records: into the recording ring as well
// Both kernels are streaming passes: lanes run along the samples of one stream, a workgroup covers 1024 consecutive samples.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rn_common.h"

namespace crispy {
namespace {

constexpr int AD_THREADS = 256;
constexpr int AD_TILE = AD_THREADS * 4;   // samples per workgroup: four consecutive ones per lane, one 16-byte store

__host__ __device__ inline long ad_tiles(long n) { return n > 0 ? (n + AD_TILE - 1) / AD_TILE : 1; }

// last + (sample - last) * t with the multiply and the add rounded separately, as the reference's are (Rust never
// contracts).  hipcc fuses a * b + c by default, __fmul_rn / __fadd_rn included (they are plain operators to it), so
// contraction is switched off for these three operations; tests/test_rn_push_host.py looks at the ISA.
__device__ __forceinline__ float lerp_unfused(float last, float cur, float t) {
#pragma clang fp contract(off)
  const float d = cur - last;
  const float p = d * t;
  return last + p;
}

// The position arithmetic of the resampler (f64 recurrence) is done once per push on the host, for all streams; the
// kernel gets (idx, t) per output and does the interpolation, last + (sample - last) * t, as three separately rounded f32
// operations (lerp_unfused).
template <bool RESAMPLE>
__global__ __launch_bounds__(AD_THREADS) void rn_adapt_in_kernel(RnAdaptIn a) {
  const unsigned tiles = (unsigned)ad_tiles((long)a.carry_len + a.n_new);      // <= 2^23: the launcher's limit
  const long b = blockIdx.x / tiles;
  const long q0 = ((long)(blockIdx.x - (unsigned)b * tiles) * AD_THREADS + threadIdx.x) * 4;
  const long total = (long)a.carry_len + a.n_new;
  const long n_frame = (long)a.frames * RN_FRAME;       // samples of the push that complete frames
  const float* in = a.in + b * a.in_stride;
  if (q0 == 0) a.last_new[b] = in[a.n_in - 1];
  if (q0 >= total) return;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long q = q0 + e;
    float x = 0.f;
    if (q < a.carry_len) {
      x = a.carry_old[b * RN_FRAME + q];
    } else if (q < total) {
      const long r = q - a.carry_len;
      if (RESAMPLE) {
        const int m = a.idx[r];
        const float cur = in[m];
        const float last = m > 0 ? in[m - 1] : a.last_old[b];
        x = lerp_unfused(last, cur, a.t[r]);
      } else {
        x = in[r];
      }
    }
    v[e] = x;
  }
  if (q0 + 4 <= n_frame) {      // n_frame is a multiple of 4: a lane's four samples are all frame samples or none is
    const float4 s4 = make_float4(v[0] * 32768.f, v[1] * 32768.f, v[2] * 32768.f, v[3] * 32768.f);
    *reinterpret_cast<float4*>(a.stage + b * n_frame + q0) = s4;
    if (a.frames48) {
      float* f = a.frames48 + b * a.frames_stride + q0;
      if (((uintptr_t)f & 15) == 0) {
        *reinterpret_cast<float4*>(f) = s4;
      } else {
        f[0] = s4.x; f[1] = s4.y; f[2] = s4.z; f[3] = s4.w;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (q0 + e < total) a.carry_new[b * RN_FRAME + (q0 + e - n_frame)] = v[e];
  }
}

__device__ __forceinline__ float adapt_out_sample(float y, float volume) {
  const float s = y / 32768.f;
  return (s < -1.f ? -1.f : (s > 1.f ? 1.f : s)) * volume;      // f32::clamp: a NaN stays a NaN
}

// VEC: every row of `out` is 16-byte aligned (pointer and stride): one float4 per lane; otherwise a lane stores the four
// samples 256 apart, so that a wave's store still covers consecutive addresses
template <bool VEC>
__global__ __launch_bounds__(AD_THREADS) void rn_adapt_out_kernel(RnAdaptOut a) {
  const unsigned tiles = (unsigned)ad_tiles(a.n_out);
  const long b = blockIdx.x / tiles;
  const long tile0 = (long)(blockIdx.x - (unsigned)b * tiles) * AD_TILE;
  const float* y = a.y + b * a.y_stride + a.skip;
  float* out = a.out + b * a.out_stride;
  if (VEC) {
    const long r = tile0 + threadIdx.x * 4;        // n_out is a multiple of 4
    if (r >= a.n_out) return;
    const float4 y4 = *reinterpret_cast<const float4*>(y + r);
    *reinterpret_cast<float4*>(out + r) = make_float4(adapt_out_sample(y4.x, a.volume), adapt_out_sample(y4.y, a.volume),
                                                      adapt_out_sample(y4.z, a.volume), adapt_out_sample(y4.w, a.volume));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long r = tile0 + e * AD_THREADS + threadIdx.x;
      if (r < a.n_out) out[r] = adapt_out_sample(y[r], a.volume);
    }
  }
}

}  // namespace

hipError_t rn_launch_adapt_in(const RnAdaptIn& a, hipStream_t s) {
  const long tiles = ad_tiles((long)a.carry_len + a.n_new);
  if (tiles > RN_MAX_BLOCKS) return hipErrorInvalidValue;
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnAdaptIn c = a;
    c.B = nb;
    c.in += b0 * a.in_stride;
    c.carry_old += b0 * RN_FRAME;
    c.carry_new += b0 * RN_FRAME;
    c.last_old += b0;
    c.last_new += b0;
    c.stage += b0 * a.frames * RN_FRAME;
    if (c.frames48) c.frames48 += b0 * a.frames_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (a.idx) hipLaunchKernelGGL(rn_adapt_in_kernel<true>, grid, dim3(AD_THREADS), 0, s, c);
    else hipLaunchKernelGGL(rn_adapt_in_kernel<false>, grid, dim3(AD_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

hipError_t rn_launch_adapt_out(const RnAdaptOut& a, hipStream_t s) {
  const long tiles = ad_tiles(a.n_out);
  if (tiles > RN_MAX_BLOCKS) return hipErrorInvalidValue;
  const bool vec = (((uintptr_t)a.out | (uintptr_t)(a.out_stride * sizeof(float))) & 15) == 0;
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnAdaptOut c = a;
    c.B = nb;
    c.y += b0 * a.y_stride;
    c.out += b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL(rn_adapt_out_kernel<true>, grid, dim3(AD_THREADS), 0, s, c);
    else hipLaunchKernelGGL(rn_adapt_out_kernel<false>, grid, dim3(AD_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

}  // namespace crispy

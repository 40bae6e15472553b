// rn_capture.hip -- crispy_rn_capture* / crispy_rn_record_app_push_at*: the statements of the capture callbacks in front of
// push_sample, for every stream of a handle at once.
//   rn_capture_kernel           build_input_stream_f32 / _i16 / _u16 (src-tauri/src/audio.rs:732-921): the device's samples
//                               converted to f32 and `iter().sum::<f32>() / input_channels as f32`, one mono sample per frame
//   (level)                     the callback's level meter over the mono: rn_level_kernel of rn_record.hip
//   rn_capture_resample_kernel  the `shared == None` arm of push_mono_to_buffers (audio.rs:697-714): the callback's own
//                               LinearResampler(input_rate, 48000) over the raw mono, into the caller's rows
//   (ring append)               on a handle that records: those rows into the mic ring, the append kernel of rn_playback.hip
//   rn_rec_app_at_kernel        the app-audio handler of a stream that is not at 48 kHz: downmix, resample_audio
//                               (src-tauri/src/recording.rs:13-39) and append to the app ring, one pass
// All three are streaming passes without LDS: lanes run along the frames (outputs) of one stream, a workgroup covers 1024 of
// them.  Resampler positions of the bypass arm, ring heads and lengths live on the host: rn_capture_io.cpp, which drives
// these kernels through the launchers declared in rn_common.h.
// The reference rounds every operation (Rust never contracts) and hipcc fuses a * b + c by default: contraction is off for the
// whole file, for the f64 position arithmetic of rn_rec_app_at_kernel as well.  The fused multiply-adds that remain in the ISA
// are those of the correctly rounded f32 division, which the hardware has as a refinement sequence only
// (tests/test_capture_host.py compiles the file both ways).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/crispy_hip.h"
#include "rn_common.h"
#include "rn_downmix.h"

#pragma clang fp contract(off)

namespace crispy {
namespace {

constexpr int CAP_THREADS = 256;
constexpr int CAP_TILE = CAP_THREADS * 4;           // frames (outputs) per workgroup

__host__ __device__ inline long cap_tiles(long n) { return n > 0 ? (n + CAP_TILE - 1) / CAP_TILE : 1; }

// What the callbacks map over a frame before they sum it.  Both integer conversions are exact: a 16-bit integer is an f32,
// so is the difference to 32768, and the division is by a power of two.
template <int FMT> struct CapIn;
template <> struct CapIn<CRISPY_PCM_F32> {
  using T = float;
  static __device__ __forceinline__ float conv(float s) { return s; }
  static __device__ __forceinline__ float from_word(uint32_t w, int) { return __uint_as_float(w); }
};
template <> struct CapIn<CRISPY_PCM_I16> {
  using T = int16_t;
  static __device__ __forceinline__ float conv(int16_t s) { return (float)s / 32768.0f; }                 // audio.rs:817
  static __device__ __forceinline__ float from_word(uint32_t w, int half) { return conv((int16_t)(uint16_t)(w >> (16 * half))); }
};
template <> struct CapIn<CRISPY_PCM_U16> {
  using T = uint16_t;
  static __device__ __forceinline__ float conv(uint16_t s) { return ((float)s - 32768.0f) / 32768.0f; }   // audio.rs:882
  static __device__ __forceinline__ float from_word(uint32_t w, int half) { return conv((uint16_t)(w >> (16 * half))); }
};

// CH > 0: every row of `in` is 16-byte aligned (pointer and byte stride) and a frame of CH channels divides 16 bytes: a lane
// takes consecutive frames -- four, or the eight of one load where a frame is two bytes -- with 16-byte loads; a lane whose
// frames reach past the end of the row loads them element by element.  CH == 0: any row, any channel count; a lane's four
// frames are 256 apart, so that every load of a wave covers consecutive frames.
// The mic path has no special case for one or two channels, unlike the app handlers: the sum starts from 0.0
// [UPSTREAM-RECALL: the identity of `Sum for f32` is +0.0, as in tests/record_oracle.py: downmix] and adds in channel order,
// every add rounded, then the correctly rounded division -- a -0.0 in a mono stream becomes +0.0.
template <int FMT, int CH>
__global__ __launch_bounds__(CAP_THREADS) void rn_capture_kernel(RnCapture a) {
  using I = CapIn<FMT>;
  using T = typename I::T;
  const unsigned tiles = (unsigned)cap_tiles(a.n);
  const long b = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x - (unsigned)b * tiles) * CAP_TILE;
  const T* in = reinterpret_cast<const T*>(a.in) + b * a.in_stride;
  float* mono = a.mono + b * a.mono_stride;
  if constexpr (CH > 0) {
    constexpr int FB = CH * (int)sizeof(T);                // bytes per frame: 2, 4, 8 or 16
    constexpr int FPL = FB >= 4 ? 4 : 16 / FB;             // frames per lane
    constexpr int LOADS = FPL * FB / 16;
    constexpr int EPW = 4 / (int)sizeof(T);                // elements per 32-bit word
    if ((int)threadIdx.x >= CAP_TILE / FPL) return;
    const int r0 = tile0 + (int)threadIdx.x * FPL;
    if (r0 >= a.n) return;
    float m[FPL];
    if (r0 + FPL <= a.n) {
      const uint4* p = reinterpret_cast<const uint4*>(in + (long)r0 * CH);
      uint32_t w[LOADS * 4];
#pragma unroll
      for (int l = 0; l < LOADS; ++l) {
        const uint4 v = p[l];
        w[4 * l] = v.x; w[4 * l + 1] = v.y; w[4 * l + 2] = v.z; w[4 * l + 3] = v.w;
      }
#pragma unroll
      for (int e = 0; e < FPL; ++e) {
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int k = e * CH + c;
          acc = acc + I::from_word(w[k / EPW], k % EPW);
        }
        m[e] = acc / (float)CH;
      }
      float* o = mono + r0;
      if (((uintptr_t)o & 15) == 0) {
#pragma unroll
        for (int e = 0; e < FPL; e += 4) *reinterpret_cast<float4*>(o + e) = make_float4(m[e], m[e + 1], m[e + 2], m[e + 3]);
      } else {
#pragma unroll
        for (int e = 0; e < FPL; ++e) o[e] = m[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < FPL; ++e) {
        if (r0 + e < a.n) {
          float acc = 0.0f;
#pragma unroll
          for (int c = 0; c < CH; ++c) acc = acc + I::conv(in[(long)(r0 + e) * CH + c]);
          mono[r0 + e] = acc / (float)CH;
        }
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = tile0 + e * CAP_THREADS + (int)threadIdx.x;
      if (r < a.n) {
        const T* f = in + (long)r * a.channels;
        float acc = 0.0f;
        for (int c = 0; c < a.channels; ++c) acc = acc + I::conv(f[c]);
        mono[r] = acc / (float)a.channels;
      }
    }
  }
}

// LinearResampler::process_sample's interpolation, `last + (sample - last) * t`: three separately rounded f32 operations.  The
// positions (idx, t) are the reference's f64 recurrence, run on the host once per capture for all streams.
template <bool RESAMPLE>
__global__ __launch_bounds__(CAP_THREADS) void rn_capture_resample_kernel(RnCaptureResample a) {
  const unsigned tiles = (unsigned)cap_tiles(a.n_out);
  const long b = blockIdx.x / tiles;
  const long tile0 = (long)(blockIdx.x - (unsigned)b * tiles) * CAP_TILE;
  const float* mono = a.mono + b * a.mono_stride;
  float* out = a.out + b * a.out_stride;
  if (tile0 == 0 && threadIdx.x == 0) a.last_new[b] = mono[a.n_in - 1];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long r = tile0 + e * CAP_THREADS + threadIdx.x;
    if (r < a.n_out) {
      if (RESAMPLE) {
        const int m = a.idx[r];
        const float cur = mono[m];
        const float last = m > 0 ? mono[m - 1] : a.last_old[b];
        const float d = cur - last;
        const float p = d * a.t[r];
        out[r] = last + p;
      } else {
        out[r] = mono[r];
      }
    }
  }
}

// resample_audio is stateless per buffer and a closed form in the reference itself: output i sits at i as f64 * ratio.  The
// f64 multiply, floor, subtract and the conversion to f32 are IEEE operations here as there.  The host has counted the outputs
// with the same expressions, so src_index < n_in for every one of them; the clamp keeps a launch inside its rows regardless.
// A lane's four outputs are 256 apart, so that every store of a wave covers consecutive ring addresses wherever the tail stands.
__global__ __launch_bounds__(CAP_THREADS) void rn_rec_app_at_kernel(RnRecAppAt a) {
  const unsigned tiles = (unsigned)cap_tiles(a.n);
  const long b = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x - (unsigned)b * tiles) * CAP_TILE;
  const float* in = a.in + b * a.in_stride;
  float* ring = a.ring + b * a.cap;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = tile0 + e * CAP_THREADS + (int)threadIdx.x;
    if (j < a.n) {
      const double src_pos = (double)(a.skip + j) * a.ratio;
      const double whole = floor(src_pos);
      const float frac = (float)(src_pos - whole);
      long idx = (long)whole;
      if (idx > a.n_in - 1) idx = a.n_in - 1;
      float s = app_downmix(in + idx * a.channels, a.channels);
      if (idx + 1 < a.n_in) {
        const float s2 = app_downmix(in + (idx + 1) * a.channels, a.channels);
        const float d = s2 - s;
        const float p = d * frac;
        s = s + p;
      }
      int i = a.tail + j;          // < 2 x cap
      if (i >= a.cap) i -= a.cap;
      ring[i] = s;
    }
  }
}

template <int FMT>
hipError_t launch_capture_fmt(const RnCapture& a, hipStream_t s) {
  using T = typename CapIn<FMT>::T;
  const long tiles = cap_tiles(a.n);                      // <= 2^14
  const int fb = a.channels * (int)sizeof(T);
  const bool vec = (((uintptr_t)a.in | (uintptr_t)(a.in_stride * (long)sizeof(T))) & 15) == 0 && 16 % fb == 0;
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnCapture c = a;
    c.B = nb;
    c.in = reinterpret_cast<const T*>(a.in) + b0 * a.in_stride;
    c.mono += b0 * a.mono_stride;
    const dim3 grid((unsigned)(c.B * tiles)), block(CAP_THREADS);
    const int ch = vec ? a.channels : 0;
    if constexpr (sizeof(T) == 2) {       // eight 16-bit channels are 16 bytes; eight floats are never `vec`
      if (ch == 8) {
        hipLaunchKernelGGL((rn_capture_kernel<FMT, 8>), grid, block, 0, s, c);
        return;
      }
    }
    if (ch == 1) hipLaunchKernelGGL((rn_capture_kernel<FMT, 1>), grid, block, 0, s, c);
    else if (ch == 2) hipLaunchKernelGGL((rn_capture_kernel<FMT, 2>), grid, block, 0, s, c);
    else if (ch == 4) hipLaunchKernelGGL((rn_capture_kernel<FMT, 4>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((rn_capture_kernel<FMT, 0>), grid, block, 0, s, c);
  });
  return hipGetLastError();
}

}  // namespace

hipError_t rn_launch_capture(const RnCapture& a, int format, hipStream_t s) {
  switch (format) {
    case CRISPY_PCM_F32: return launch_capture_fmt<CRISPY_PCM_F32>(a, s);
    case CRISPY_PCM_I16: return launch_capture_fmt<CRISPY_PCM_I16>(a, s);
    case CRISPY_PCM_U16: return launch_capture_fmt<CRISPY_PCM_U16>(a, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t rn_launch_capture_resample(const RnCaptureResample& a, hipStream_t s) {
  const long tiles = cap_tiles(a.n_out);                  // <= 2^18
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnCaptureResample c = a;
    c.B = nb;
    c.mono += b0 * a.mono_stride;
    c.last_old += b0;
    c.last_new += b0;
    c.out += b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (a.idx) hipLaunchKernelGGL(rn_capture_resample_kernel<true>, grid, dim3(CAP_THREADS), 0, s, c);
    else hipLaunchKernelGGL(rn_capture_resample_kernel<false>, grid, dim3(CAP_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

hipError_t rn_launch_rec_app_at(const RnRecAppAt& a, hipStream_t s) {
  const long tiles = cap_tiles(a.n);                      // <= 2^18
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnRecAppAt c = a;
    c.B = nb;
    c.in += b0 * a.in_stride;
    c.ring += b0 * a.cap;
    hipLaunchKernelGGL(rn_rec_app_at_kernel, dim3((unsigned)(c.B * tiles)), dim3(CAP_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

}  // namespace crispy

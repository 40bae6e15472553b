// rn_pcm.h -- what the two playback kernels share (rn_playback.hip: the RNNoise arm, rn_legacy.hip: the Legacy arm):
// next_sample's interpolation and the output callback's conversions, device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/crispy_hip.h"

namespace crispy {
namespace {

// s0 + (s1 - s0) * frac with the subtract, the multiply and the add rounded separately, as next_sample's are (Rust never
// contracts).  hipcc fuses a * b + c by default: contraction is switched off here and in the conversions below, and
// tests/test_playback_host.py looks at the ISA.
__device__ __forceinline__ float pull_lerp(float s0, float s1, float frac) {
#pragma clang fp contract(off)
  const float d = s1 - s0;
  const float p = d * frac;
  return s0 + p;
}

__device__ __forceinline__ float clamp_pm1(float s) { return s < -1.f ? -1.f : (s > 1.f ? 1.f : s); }     // f32::clamp: a NaN stays a NaN

// The output callback's conversions (audio.rs:613-650).  Rust's `as` truncates toward zero and makes a NaN 0.
template <int FMT> struct Pcm;
template <> struct Pcm<CRISPY_PCM_F32> {
  using T = float;
  static __device__ __forceinline__ uint32_t bits(float s) { return __float_as_uint(s); }
  static __device__ __forceinline__ T elem(uint32_t w) { return __uint_as_float(w); }
};
template <> struct Pcm<CRISPY_PCM_I16> {
  using T = int16_t;
  static __device__ __forceinline__ uint32_t bits(float s) {
#pragma clang fp contract(off)
    const float x = clamp_pm1(s) * 32767.f;
    const int q = s != s ? 0 : (int)x;       // |x| <= 32767
    return (uint32_t)q & 0xffffu;
  }
  static __device__ __forceinline__ T elem(uint32_t w) { return (int16_t)(uint16_t)w; }
};
template <> struct Pcm<CRISPY_PCM_U16> {
  using T = uint16_t;
  static __device__ __forceinline__ uint32_t bits(float s) {
#pragma clang fp contract(off)
    const float h = clamp_pm1(s) * 0.5f;
    const float u = h + 0.5f;
    const float x = u * 65535.f;
    const int q = s != s ? 0 : (int)x;       // 0 <= x <= 65535
    return (uint32_t)q;
  }
  static __device__ __forceinline__ T elem(uint32_t w) { return (uint16_t)w; }
};

}  // namespace
}  // namespace crispy

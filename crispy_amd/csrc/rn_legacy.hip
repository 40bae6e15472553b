// rn_legacy.hip -- the Legacy arm of NsState, SharedAudio (src-tauri/src/audio.rs:136-200), for every stream of a handle at
// once: what crispy_rn_push* and crispy_rn_pull* run on a handle whose model is CRISPY_NS_DUMMY or CRISPY_NS_NOISY.
//   rn_legacy_push_kernel   push_sample over a block: out = x * volume (Noisy: + noise * 0.05) and, in the same pass, the RAW x
//                           into the playback ring at the tail (modulo cap), minus what the ring's eviction drops at the front
//   rn_legacy_pull_kernel   next_sample per output frame: gather ring[head + offset] and its successor, interpolate, Noisy:
//                           + noise * 0.05, x the volume, convert to f32 / i16 / u16, store to `channels` interleaved outputs
// The recording side of a Legacy push (the callback's LinearResampler over what the push returned, then the mic ring) is
// rn_capture_resample_kernel and the ring append, as in the bypass arm.
// Both kernels are streaming passes without LDS: lanes run along the samples of one stream.  The noise of sample k of a call
// is LCG step k + 1 from the state the call starts with, the same for every stream: a lane jumps to its own first state
// (rn_common.h: one 32-bit multiply-add per set bit -- the bits above the tile are the same for the whole workgroup and go
// through the scalar unit) and steps from there.  Nothing is carried on the device; the host advances its copy of the state.
// The reference rounds every operation (Rust never contracts) and hipcc fuses a * b + c by default: contraction is off for
// the whole file, and tests/test_legacy_host.py looks at the ISA.
// Kernels and their launchers (declared in rn_common.h); the entry points that drive them are rn_legacy_io.cpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/crispy_hip.h"
#include "rn_common.h"
#include "rn_pcm.h"

#pragma clang fp contract(off)

namespace crispy {
namespace {

constexpr int LG_THREADS = 256;
constexpr int LG_TILE = LG_THREADS * 4;            // samples per workgroup of the push

__host__ __device__ inline long lg_tiles(long n, long tile) { return n > 0 ? (n + tile - 1) / tile : 1; }

// `processed = sample * volume; processed += noise * 0.05` and `sample += noise * 0.05`: a multiply and an add, each rounded.
__device__ __forceinline__ float add_noise(float v, uint32_t state) {
  const float nz = ns_noise(state) * 0.05f;
  return v + nz;
}

// A lane takes four consecutive samples.  VEC: every row of `in` and `out` is 16-byte aligned (pointer and stride): one
// 16-byte load and one 16-byte store per lane; the row's last, partial group goes sample by sample.  The ring's tail stands
// anywhere: where a lane's four samples happen to fall on a 16-byte piece of a ring row (ring_vec: rows are aligned, i.e. cap
// is a multiple of 4) they are one store, otherwise four single ones.
template <bool NOISY, bool VEC>
__global__ __launch_bounds__(LG_THREADS) void rn_legacy_push_kernel(RnLegacyPush a) {
  const unsigned tiles = (unsigned)lg_tiles(a.n, LG_TILE);
  const long b = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x - (unsigned)b * tiles) * LG_TILE;
  const int r0 = tile0 + (int)threadIdx.x * 4;
  if (r0 >= a.n) return;
  const float* in = a.in + b * a.in_stride;
  float* out = a.out + b * a.out_stride;
  const bool whole = r0 + 4 <= a.n;
  float x[4];
  if (VEC && whole) {
    const float4 v = *reinterpret_cast<const float4*>(in + r0);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = r0 + e < a.n ? in[r0 + e] : 0.f;
  }
  uint32_t state = 0;
  if (NOISY) {
    state = ns_lcg_jump_bits<10, 32>(a.rng, (uint32_t)tile0);            // the workgroup's: tile0 is a multiple of 1024
    state = ns_lcg_jump_bits<2, 10>(state, threadIdx.x * 4u);           // the lane's: the state in front of sample r0
  }
  float y[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    y[e] = x[e] * a.volume;
    if (NOISY) {
      state = ns_lcg_step(state);
      y[e] = add_noise(y[e], state);
    }
  }
  if (VEC && whole) {
    *reinterpret_cast<float4*>(out + r0) = make_float4(y[0], y[1], y[2], y[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (r0 + e < a.n) out[r0 + e] = y[e];
  }
  if (a.ring) {
    float* ring = a.ring + b * a.cap;
    int i0 = a.tail + (r0 - a.skip);         // < 2 x cap; where the lane's first sample goes, if it is kept
    if (i0 >= a.cap) i0 -= a.cap;
    if (a.ring_vec && whole && r0 >= a.skip && (i0 & 3) == 0) {
      // the four land on one 16-byte piece of the row: cap is a multiple of 4, so the piece does not straddle the wrap
      *reinterpret_cast<float4*>(ring + i0) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = r0 + e;
        if (r < a.n && r >= a.skip) {
          int i = a.tail + (r - a.skip);       // < 2 x cap
          if (i >= a.cap) i -= a.cap;
          ring[i] = x[e];
        }
      }
    }
  }
}

// Frame f of a pull.  A dry frame (off < 0) returns next_sample's 0.0 and advances nothing; the live ones are frames
// 0 ... n_live - 1, so live frame f takes LCG step f + 1.
template <bool NOISY>
__device__ __forceinline__ float legacy_pull_sample(const RnLegacyPull& a, const float* ring, unsigned f) {
  const RnPull& p = a.p;
  const int off = p.off[f];
  if (off < 0) return 0.f;
  int i0 = p.head + off;           // < 2 x cap
  if (i0 >= p.cap) i0 -= p.cap;
  const int i1 = i0 + 1 == p.cap ? 0 : i0 + 1;
  float s = pull_lerp(ring[i0], ring[i1], p.frac[f]);
  if (NOISY) s = add_noise(s, ns_lcg_jump_bits<0, 25>(a.rng, f + 1u));       // f < 2^24
  return s * a.volume;
}

// The layout of rn_pull_kernel (rn_playback.hip): a row of `out` is n_frames x channels elements, element e belonging to
// frame e / channels.  VEC: every row is 16-byte aligned (pointer and stride): a lane takes the 16 / sizeof(T) consecutive
// elements of one 16-byte store and works out each frame they touch once; the row's last, partial piece goes element by
// element.  Otherwise a lane's elements are 256 apart, so that a wave's store still covers consecutive addresses.
template <int FMT, bool NOISY, bool VEC>
__global__ __launch_bounds__(LG_THREADS) void rn_legacy_pull_kernel(RnLegacyPull a) {
  using P = Pcm<FMT>;
  using T = typename P::T;
  constexpr int EPV = 16 / (int)sizeof(T);
  constexpr unsigned TILE = LG_THREADS * EPV;
  const RnPull& p = a.p;
  const unsigned tiles = (unsigned)lg_tiles(p.n_elems, TILE);
  const long b = blockIdx.x / tiles;
  const unsigned tile0 = (blockIdx.x - (unsigned)b * tiles) * TILE;
  const float* ring = p.ring + b * p.cap;
  T* out = reinterpret_cast<T*>(p.out) + b * p.out_stride;
  if (VEC) {
    const unsigned e0 = tile0 + threadIdx.x * EPV;
    if (e0 >= p.n_elems) return;
    unsigned f = e0 / p.channels;
    unsigned c = e0 - f * p.channels;
    uint32_t cur = P::bits(legacy_pull_sample<NOISY>(a, ring, f));
    uint32_t w[EPV];
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
      w[k] = cur;
      if (++c == p.channels) {
        c = 0;
        ++f;
        if (k + 1 < EPV && f < p.n_frames) cur = P::bits(legacy_pull_sample<NOISY>(a, ring, f));
      }
    }
    if (e0 + EPV <= p.n_elems) {
      uint4 v;
      if constexpr (EPV == 4) v = make_uint4(w[0], w[1], w[2], w[3]);
      else v = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
      *reinterpret_cast<uint4*>(out + e0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < EPV; ++k)
        if (e0 + k < p.n_elems) out[e0 + k] = P::elem(w[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
      const unsigned e = tile0 + k * LG_THREADS + threadIdx.x;
      if (e < p.n_elems) out[e] = P::elem(P::bits(legacy_pull_sample<NOISY>(a, ring, e / p.channels)));
    }
  }
}

template <bool NOISY>
hipError_t launch_push(const RnLegacyPush& a, hipStream_t s) {
  const long tiles = lg_tiles(a.n, LG_TILE);              // <= 2^14
  const bool vec = (((uintptr_t)a.in | (uintptr_t)a.out | (uintptr_t)(a.in_stride * 4) | (uintptr_t)(a.out_stride * 4)) & 15) == 0;
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnLegacyPush c = a;
    c.B = nb;
    c.in += b0 * a.in_stride;
    c.out += b0 * a.out_stride;
    if (c.ring) c.ring += b0 * a.cap;
    c.ring_vec = c.ring && a.cap % 4 == 0 && ((uintptr_t)c.ring & 15) == 0;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL((rn_legacy_push_kernel<NOISY, true>), grid, dim3(LG_THREADS), 0, s, c);
    else hipLaunchKernelGGL((rn_legacy_push_kernel<NOISY, false>), grid, dim3(LG_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

template <int FMT, bool NOISY>
hipError_t launch_pull(const RnLegacyPull& a, hipStream_t s) {
  using T = typename Pcm<FMT>::T;
  const RnPull& p = a.p;
  const long tiles = lg_tiles(p.n_elems, LG_THREADS * (16 / (long)sizeof(T)));       // <= 2^17
  const bool vec = (((uintptr_t)p.out | (uintptr_t)(p.out_stride * (long)sizeof(T))) & 15) == 0;
  rn_for_stream_groups(p.B, tiles, [&](long b0, int nb) {
    RnLegacyPull c = a;
    c.p.B = nb;
    c.p.ring += b0 * p.cap;
    c.p.out = reinterpret_cast<T*>(p.out) + b0 * p.out_stride;
    const dim3 grid((unsigned)(c.p.B * tiles));
    if (vec) hipLaunchKernelGGL((rn_legacy_pull_kernel<FMT, NOISY, true>), grid, dim3(LG_THREADS), 0, s, c);
    else hipLaunchKernelGGL((rn_legacy_pull_kernel<FMT, NOISY, false>), grid, dim3(LG_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

template <bool NOISY>
hipError_t launch_pull_fmt(const RnLegacyPull& a, int format, hipStream_t s) {
  switch (format) {
    case CRISPY_PCM_F32: return launch_pull<CRISPY_PCM_F32, NOISY>(a, s);
    case CRISPY_PCM_I16: return launch_pull<CRISPY_PCM_I16, NOISY>(a, s);
    case CRISPY_PCM_U16: return launch_pull<CRISPY_PCM_U16, NOISY>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t rn_launch_legacy_push(const RnLegacyPush& a, bool noisy, hipStream_t s) {
  return noisy ? launch_push<true>(a, s) : launch_push<false>(a, s);
}

hipError_t rn_launch_legacy_pull(const RnLegacyPull& a, int format, bool noisy, hipStream_t s) {
  return noisy ? launch_pull_fmt<true>(a, format, s) : launch_pull_fmt<false>(a, format, s);
}

}  // namespace crispy

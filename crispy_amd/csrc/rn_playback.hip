// rn_playback.hip -- crispy_rn_playback_* / crispy_rn_pull*: the playback half of RnnNoiseProcessor for every stream of a
// handle at once.  push_sample appends what it returns to `output_buf`, a deque of at most one second (src-tauri/src/audio.rs:
// 280-285); the output callback reads next_sample() once per output frame (audio.rs:297-314, 610-657), a linear-interpolating
// read at input_rate / output_rate, converts the sample to the device's format and writes it to every channel of the frame.
//   rn_ring_append_kernel   the samples a push returned, copied into the ring [n_streams][cap] at the tail (modulo cap)
//   rn_pull_kernel          per output frame: gather ring[head + offset] and its successor, interpolate (three separately
//                           rounded f32 operations), convert to f32 / i16 / u16, store to `channels` interleaved outputs
// Head, length and resample_pos live on the host: the streams of a handle are pushed and pulled in lock step, so they are the
// same for all of them and do not depend on the samples.  The host runs the reference's f64 recurrence once per pull, frame by
// frame, and uploads one (offset, fraction) pair per output frame.
// Both kernels are streaming passes: lanes run along the samples of one stream, a workgroup covers consecutive ones.
// Kernels and their launchers (declared in rn_common.h); the entry points that drive them are rn_io.cpp.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/crispy_hip.h"
#include "rn_common.h"
#include "rn_pcm.h"

namespace crispy {
namespace {

constexpr int PB_THREADS = 256;
constexpr int PB_COPY_TILE = PB_THREADS * 4;       // samples per workgroup of the append

__host__ __device__ inline long pb_tiles(long n, long tile) { return n > 0 ? (n + tile - 1) / tile : 1; }

// A pure copy: the ring holds exactly the bits the push returned.  A lane's four samples are 256 apart, so that every store
// of a wave covers consecutive addresses wherever the tail stands.
__global__ __launch_bounds__(PB_THREADS) void rn_ring_append_kernel(RnRingAppend a) {
  const unsigned tiles = (unsigned)pb_tiles(a.n, PB_COPY_TILE);
  const long b = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x - (unsigned)b * tiles) * PB_COPY_TILE;
  const float* src = a.src + b * a.src_stride;
  float* ring = a.ring + b * a.cap;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = tile0 + e * PB_THREADS + (int)threadIdx.x;
    if (r < a.n) {
      int i = a.tail + r;          // < 2 x cap
      if (i >= a.cap) i -= a.cap;
      ring[i] = src[r];
    }
  }
}

__device__ __forceinline__ float pull_sample(const RnPull& a, const float* ring, unsigned f) {
  const int off = a.off[f];
  if (off < 0) return 0.f;
  int i0 = a.head + off;           // < 2 x cap
  if (i0 >= a.cap) i0 -= a.cap;
  const int i1 = i0 + 1 == a.cap ? 0 : i0 + 1;
  return pull_lerp(ring[i0], ring[i1], a.frac[f]);
}

// A row of `out` is n_frames x channels elements, element e belonging to frame e / channels.
// VEC: every row is 16-byte aligned (pointer and stride): a lane takes the 16 / sizeof(T) consecutive elements of one
// 16-byte store and works out each frame they touch once; the row's last, partial piece goes element by element.
// Otherwise a lane's elements are 256 apart, so that a wave's store still covers consecutive addresses.
template <int FMT, bool VEC>
__global__ __launch_bounds__(PB_THREADS) void rn_pull_kernel(RnPull a) {
  using P = Pcm<FMT>;
  using T = typename P::T;
  constexpr int EPV = 16 / (int)sizeof(T);
  constexpr unsigned TILE = PB_THREADS * EPV;
  const unsigned tiles = (unsigned)pb_tiles(a.n_elems, TILE);
  const long b = blockIdx.x / tiles;
  const unsigned tile0 = (blockIdx.x - (unsigned)b * tiles) * TILE;
  const float* ring = a.ring + b * a.cap;
  T* out = reinterpret_cast<T*>(a.out) + b * a.out_stride;
  if (VEC) {
    const unsigned e0 = tile0 + threadIdx.x * EPV;
    if (e0 >= a.n_elems) return;
    unsigned f = e0 / a.channels;
    unsigned c = e0 - f * a.channels;
    uint32_t cur = P::bits(pull_sample(a, ring, f));
    uint32_t w[EPV];
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
      w[k] = cur;
      if (++c == a.channels) {
        c = 0;
        ++f;
        if (k + 1 < EPV && f < a.n_frames) cur = P::bits(pull_sample(a, ring, f));
      }
    }
    if (e0 + EPV <= a.n_elems) {
      uint4 v;
      if constexpr (EPV == 4) v = make_uint4(w[0], w[1], w[2], w[3]);
      else v = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
      *reinterpret_cast<uint4*>(out + e0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < EPV; ++k)
        if (e0 + k < a.n_elems) out[e0 + k] = P::elem(w[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
      const unsigned e = tile0 + k * PB_THREADS + threadIdx.x;
      if (e < a.n_elems) out[e] = P::elem(P::bits(pull_sample(a, ring, e / a.channels)));
    }
  }
}

}  // namespace

// tiles <= 47 for a cap of one second, <= 2^18 for a recording ring
hipError_t rn_launch_ring_append(const RnRingAppend& a, hipStream_t s) {
  const long tiles = pb_tiles(a.n, PB_COPY_TILE);
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnRingAppend c = a;
    c.B = nb;
    c.src += b0 * a.src_stride;
    c.ring += b0 * a.cap;
    hipLaunchKernelGGL(rn_ring_append_kernel, dim3((unsigned)(c.B * tiles)), dim3(PB_THREADS), 0, s, c);
  });
  return hipGetLastError();
}

namespace {
template <int FMT>
hipError_t launch_pull_fmt(const RnPull& a, hipStream_t s) {
  using T = typename Pcm<FMT>::T;
  const long tiles = pb_tiles(a.n_elems, PB_THREADS * (16 / (long)sizeof(T)));       // <= 2^17
  const bool vec = (((uintptr_t)a.out | (uintptr_t)(a.out_stride * (long)sizeof(T))) & 15) == 0;
  rn_for_stream_groups(a.B, tiles, [&](long b0, int nb) {
    RnPull c = a;
    c.B = nb;
    c.ring += b0 * a.cap;
    c.out = reinterpret_cast<T*>(a.out) + b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL((rn_pull_kernel<FMT, true>), grid, dim3(PB_THREADS), 0, s, c);
    else hipLaunchKernelGGL((rn_pull_kernel<FMT, false>), grid, dim3(PB_THREADS), 0, s, c);
  });
  return hipGetLastError();
}
}  // namespace

hipError_t rn_launch_pull(const RnPull& a, int format, hipStream_t s) {
  switch (format) {
    case CRISPY_PCM_F32: return launch_pull_fmt<CRISPY_PCM_F32>(a, s);
    case CRISPY_PCM_I16: return launch_pull_fmt<CRISPY_PCM_I16>(a, s);
    default: return launch_pull_fmt<CRISPY_PCM_U16>(a, s);
  }
}

}  // namespace crispy

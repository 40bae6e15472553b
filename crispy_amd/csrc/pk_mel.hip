// pk_mel.hip -- Parakeet's log-mel front end for MI355X (gfx950): what transformers' ParakeetFeatureExtractor computes from 16 kHz
// mono f32 samples, for all clips of a ragged call in three launches.  Exact f32 operands.
//
//   mel_frames_kernel     grid (tiles of all clips): a workgroup of 4 waves takes kMelTileFrames consecutive frames of one clip,
//                         a wave kMelWaveFrames of them, PM_NF at a time.  Per frame t: the 400 samples from 160 t - 200 and
//                         their predecessors read straight from the clip (zero outside the clip's own [0, n)), pre-emphasis
//                         x[s] - f32(0.97 x[s - 1]), symmetric Hann window, zero padding to 512 (the window sits at 0 ... 399: a
//                         circular shift of the reference's 56 ... 455 leaves the power alone), the real FFT as a 256-point
//                         complex Stockham transform in LDS (radices 4.4.4.4) plus the real-input pass, power in place over
//                         bins 0 ... 256, each filter's run of weights summed in f32 in tap order, logf(e + 2^-24).  Twiddles,
//                         window and the filter runs sit in LDS once per workgroup.  Then, per bin, the tile's partial sums
//                         for the statistics, in double and in frame order, about the tile's own first value.
//   mel_stats_kernel      one thread per (clip, bin): the tiles' partial sums moved to the clip's first value and added in
//                         tile order, in double; mean and standard deviation (divisor rows - 1) rounded once to f32.  No
//                         atomics: the order is fixed by the clip's length alone.  A constant column gives std = 0 exactly.
//   mel_normalise_kernel  (v - mean) / (std + 1e-5f) in f32 over the clip's rows.
#include <cmath>

#include "fft_lds.h"
#include "pk_internal.h"

namespace crispy {
namespace pk {
namespace {

using namespace fftx;

constexpr int PM_NF = 4;         // frames a wave transforms at once
constexpr int PM_BS = 264;       // complex numbers between two frames' buffers (257 used: bin 256 keeps its power there)
constexpr size_t PM_LDS_BUF = 4 * PM_NF * PM_BS * sizeof(float2);
constexpr size_t PM_LDS = PM_LDS_BUF + sizeof(MelTables);
constexpr int PM_HEAD = (int)(offsetof(MelTables, taps) / 4);      // 32-bit words in front of the taps
static_assert(kMelWaveFrames % PM_NF == 0 && kMelTileFrames == 4 * kMelWaveFrames, "a tile is 4 waves of whole batches");
static_assert(offsetof(MelTables, taps) % 4 == 0 && sizeof(MelTables) % 4 == 0, "copied into LDS as 32-bit words");
static_assert(PM_LDS <= 64 * 1024, "above the default dynamic-LDS limit");
static_assert(kMelWin <= 7 * 64 && kMelFft == 512, "seven samples per lane; the eighth 64 are zeros");

// y[s] of the clip: x[s] - f32(0.97 x[s - 1]), y[0] = x[0], 0 outside [0, n).  The product is rounded before the subtraction.
__device__ __forceinline__ float preemph(const float* __restrict__ x, int s, int n) {
#pragma clang fp contract(off)
  if (s < 0 || s >= n) return 0.0f;
  const float cur = x[s];
  if (s == 0) return cur;
  const float p = 0.97f * x[s - 1];
  return cur - p;
}

__global__ __launch_bounds__(256) void mel_frames_kernel(const MelTables* __restrict__ tab, int M, const float* __restrict__ pcm,
                                                         const MelClip* __restrict__ clips, const MelTile* __restrict__ tiles,
                                                         float* __restrict__ raw, double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // per wave: PM_NF transform buffers (the power of bin k replaces the real part of element k); per workgroup: the tables
  float2* buf = reinterpret_cast<float2*>(smem) + wave * (PM_NF * PM_BS);
  float* fl = reinterpret_cast<float*>(buf);
  const MelTables* lt = reinterpret_cast<const MelTables*>(smem + PM_LDS_BUF);
  {
    const int* __restrict__ src = reinterpret_cast<const int*>(tab);
    int* dst = reinterpret_cast<int*>(smem + PM_LDS_BUF);
    const int words = PM_HEAD + min(max(tab->n_taps, 0), kMelMaxTaps);
    for (int i = threadIdx.x; i < words; i += 256) dst[i] = src[i];
    __syncthreads();
  }
  const MelTile tile = tiles[blockIdx.x];
  const MelClip cl = clips[tile.clip];
  const float* __restrict__ x = pcm + cl.first;

  for (int fb = 0; fb < kMelWaveFrames; fb += PM_NF) {
    const int f0 = tile.frame0 + wave * kMelWaveFrames + fb;
    if (f0 >= cl.rows) break;      // the same for the whole wave; only wave-level synchronisation inside the loop
    // samples, pre-emphasis, window; frames past the clip's last redo it (their rows are not stored)
#pragma unroll
    for (int f = 0; f < PM_NF; ++f) {
      const int s0 = min(f0 + f, cl.rows - 1) * kMelHop - kMelWin / 2;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int i = lane + 64 * j;
        fl[f * 2 * PM_BS + i] = i < kMelWin ? preemph(x, s0 + i, cl.n) * lt->window[i] : 0.0f;
      }
      fl[f * 2 * PM_BS + 448 + lane] = 0.0f;
    }
    wave_lds_sync();
    // z[m] = (y[2m], y[2m+1]) is the float array itself
    pass_batched<256, 4, 1, 512, PM_NF, PM_BS>(buf, lt->w512, lane);
    pass_batched<256, 4, 4, 512, PM_NF, PM_BS>(buf, lt->w512, lane);
    pass_batched<256, 4, 16, 512, PM_NF, PM_BS>(buf, lt->w512, lane);
    pass_batched<256, 4, 64, 512, PM_NF, PM_BS>(buf, lt->w512, lane);
    // real-input pass of the pair (k, 256 - k) and power spectrum
    {
      constexpr int TOT = PM_NF * 129, NT = (TOT + 63) / 64;
#pragma unroll
      for (int it = 0; it < NT; ++it) {
        const int idx = lane + 64 * it;
        if (idx < TOT) {
          const int f = idx / 129, k = idx - f * 129;
          const float2* bf = buf + f * PM_BS;
          const float2 zk = bf[k];
          const float2 zn = (k == 0) ? zk : bf[256 - k];
          float2 zc = cconj(zn);
          float2 fe = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
          float2 d = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
          float2 tt = cmul(lt->w512[k], make_float2(d.y, -d.x));
          const float2 xk = cadd(fe, tt);
          zc = cconj(zk);
          fe = make_float2(0.5f * (zn.x + zc.x), 0.5f * (zn.y + zc.y));
          d = make_float2(0.5f * (zn.x - zc.x), 0.5f * (zn.y - zc.y));
          tt = cmul(lt->w512[256 - k], make_float2(d.y, -d.x));
          const float2 xn = cadd(fe, tt);
          // in place: elements k and 256 - k belong to this work item alone, and both were read above
          fl[2 * (f * PM_BS + k)] = xk.x * xk.x + xk.y * xk.y;
          fl[2 * (f * PM_BS + 256 - k)] = xn.x * xn.x + xn.y * xn.y;
        }
      }
    }
    wave_lds_sync();
    // filter runs, f32 in tap order, log with the guard: one (frame, bin) per lane and step
    {
      const int tot = PM_NF * M;
      for (int idx = lane; idx < tot; idx += 64) {
        const int f = idx / M, m = idx - f * M;
        const unsigned meta = lt->meta[m];
        const int k0 = (int)(meta & 0x1ffu), len = (int)((meta >> 9) & 0x1ffu);
        const float* w = lt->taps + (meta >> 18);
        const float* p = fl + 2 * (f * PM_BS + k0);
        float e = 0.0f;
        for (int q = 0; q < len; ++q) e += p[2 * q] * w[q];
        if (f0 + f < cl.rows) raw[(cl.row0 + f0 + f) * M + m] = logf(e + 5.9604644775390625e-08f);
      }
    }
    wave_lds_sync();
  }
  // the tile's rows are in global memory, written by this workgroup: per bin, their sums in frame order
  __syncthreads();
  if ((int)threadIdx.x < M) {
    const int m = threadIdx.x;
    const int nf = min(kMelTileFrames, cl.rows - tile.frame0);
    const float* r = raw + (cl.row0 + tile.frame0) * M + m;
    const double p = (double)r[0];
    double s1 = 0.0, s2 = 0.0;
    for (int t = 1; t < nf; ++t) {
      const double d = (double)r[(long)t * M] - p;
      s1 += d;
      s2 += d * d;
    }
    double* o = part + (long)blockIdx.x * 3 * M + m;
    o[0] = p;
    o[M] = s1;
    o[2 * M] = s2;
  }
}

__global__ __launch_bounds__(256) void mel_stats_kernel(const MelClip* __restrict__ clips, int n_clips, int M, const double* __restrict__ part,
                                                        float* __restrict__ stats) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int c = idx / M, m = idx - c * M;
  if (c >= n_clips) return;
  const MelClip cl = clips[c];
  const double* q = part + (long)cl.tile0 * 3 * M + m;
  const double v0 = q[0];
  double s1 = 0.0, s2 = 0.0;
  for (int t = 0; t < cl.n_tiles; ++t) {
    const double* o = q + (long)t * 3 * M;
    const double nf = (double)min(kMelTileFrames, cl.rows - t * kMelTileFrames);
    const double d = o[0] - v0, a = o[M], b = o[2 * M];
    // sum (v - v0) = a + nf d;  sum (v - v0)^2 = b + 2 d a + nf d^2
    s1 += a + nf * d;
    s2 += b + 2.0 * d * a + nf * d * d;
  }
  const double n = (double)cl.rows;
  const double var = fmax(s2 - s1 * s1 / n, 0.0) / (n - 1.0);
  stats[((long)c * 2) * M + m] = (float)(v0 + s1 / n);
  stats[((long)c * 2 + 1) * M + m] = (float)sqrt(var);
}

__global__ __launch_bounds__(256) void mel_normalise_kernel(const MelClip* __restrict__ clips, const MelTile* __restrict__ tiles, int M,
                                                            const float* __restrict__ raw, const float* __restrict__ stats,
                                                            float* __restrict__ feats) {
  const MelTile tile = tiles[blockIdx.x];
  const MelClip cl = clips[tile.clip];
  const int nf = min(kMelTileFrames, cl.rows - tile.frame0);
  const long base = (cl.row0 + tile.frame0) * M;
  const float* st = stats + (long)tile.clip * 2 * M;
  for (int i = threadIdx.x; i < nf * M; i += 256) {
    const int m = i % M;
    feats[base + i] = (raw[base + i] - st[m]) / (st[M + m] + 1e-5f);
  }
}

}  // namespace

hipError_t launch_mel_frames(const MelTables* d_tab, int M, const float* d_pcm, const MelClip* d_clips, const MelTile* d_tiles, int n_tiles,
                             float* d_raw, double* d_part, hipStream_t st) {
  if (n_tiles < 1) return hipSuccess;
  hipLaunchKernelGGL(mel_frames_kernel, dim3(n_tiles), dim3(256), PM_LDS, st, d_tab, M, d_pcm, d_clips, d_tiles, d_raw, d_part);
  return hipGetLastError();
}

hipError_t launch_mel_stats(const MelClip* d_clips, int n_clips, int M, const double* d_part, float* d_stats, hipStream_t st) {
  const int total = n_clips * M;
  if (total < 1) return hipSuccess;
  hipLaunchKernelGGL(mel_stats_kernel, dim3((total + 255) / 256), dim3(256), 0, st, d_clips, n_clips, M, d_part, d_stats);
  return hipGetLastError();
}

hipError_t launch_mel_normalise(const MelClip* d_clips, const MelTile* d_tiles, int n_tiles, int M, const float* d_raw, const float* d_stats,
                                float* d_feats, hipStream_t st) {
  if (n_tiles < 1) return hipSuccess;
  hipLaunchKernelGGL(mel_normalise_kernel, dim3(n_tiles), dim3(256), 0, st, d_clips, d_tiles, M, d_raw, d_stats, d_feats);
  return hipGetLastError();
}

}  // namespace pk
}  // namespace crispy

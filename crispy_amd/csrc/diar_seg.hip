// diar_seg.hip -- the segmentation network of the diarization path for MI355X (gfx950): pyannote segmentation-3.0
// (SincNet, a 4-layer bidirectional LSTM, three linear layers), the first session.run of run_diarization
// (src-tauri/src/managers/diarization.rs:103-145).  f32 operands and f32 sums everywhere; rows are time-major
// ([position][channel]) from the first pooled stage on, so that every store and every tile load is contiguous.
//
//   seg_windows_kernel    PCM of a recording -> zero-padded float windows (i16, or f32 through f32_to_i16, / 32768).
//   seg_stats_kernel      one workgroup per window: mean and 1 / sqrt(biased variance + 1e-5) of every channel over time.
//                         Two passes, both about the channel's first value, 1024 / C strided slices per channel summed in
//                         a fixed tree: a constant row has deviation 0 exactly and normalises to beta.
//   seg_conv_pool_kernel  one stage of the SincNet: a workgroup takes 32 pooled positions (96 convolution positions) of one
//                         window for all output channels.  The input span goes to LDS normalised (and through leaky_relu
//                         from stage 1 on); thread (group, co) keeps 24 sums, reads its weight once per tap (contiguous
//                         over co) and the inputs as LDS broadcasts; abs or bias and the max over 3 in the store, so no
//                         pre-pool value reaches memory.  Taps are summed in (ci, k) order.
//   seg_norm_kernel       the last instance norm and leaky_relu -> [frames][60].
//   seg_proj_kernel       x [rows][in] . w_ih^T + (bias_ih + bias_hh) for both directions: 64 x 64 tiles, 4 x 4 per thread,
//                         k in ascending order per output.
//   seg_lstm_kernel       one workgroup of 512 threads per (window, direction): thread g keeps row g of weight_hh (128 f32)
//                         in registers for all steps, h is read from LDS as broadcasts, the four gates of a cell meet in
//                         LDS, c stays in the registers of 128 threads; two barriers per step.  expf and tanhf, not the
//                         fast forms.
//   seg_head_kernel       8 frame rows per workgroup: two linear layers with leaky_relu, the classifier, log_softmax; every dot
//                         product as four interleaved partial sums (one chain over 256 terms put the scores at 1.3 - 2.1 x
//                         the float32 torch oracle's distance to float64 while the LSTM output below it sat at 0.9).
// No sum depends on the number of windows in the launch: every workgroup works on one window (the projection and the head
// on rows, each row by itself).
#include <cmath>

#include "diar_internal.h"

namespace crispy {
namespace diar {
namespace {

constexpr float kSegEps = 1e-5f, kSegSlope = 0.01f;

__device__ __forceinline__ float leaky(float v) { return v > 0.0f ? v : kSegSlope * v; }

template <bool F32>
__global__ __launch_bounds__(256) void seg_windows_kernel(const void* __restrict__ pcm, long n, long first, long total, float* __restrict__ x) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long s = first + i;
  int q = 0;
  if (s < n) {
    if (F32) {
      const float v = static_cast<const float*>(pcm)[s];
      const float c = fminf(fmaxf(v, -1.0f), 1.0f);
      q = v != v ? 0 : (int)(c * 32767.0f);
    } else {
      q = static_cast<const short*>(pcm)[s];
    }
  }
  x[i] = (float)q / 32768.0f;
}

// Sum over the slices of part[slice * C + c] in a fixed tree; the result is in part[c].
__device__ __forceinline__ void slice_tree(float* part, int S, int C, int s, int c) {
  int top = 1;
  while (top < S) top <<= 1;
  for (int h = top >> 1; h >= 1; h >>= 1) {
    if (s < h && s + h < S) part[s * C + c] += part[(s + h) * C + c];
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void seg_stats_kernel(const float* __restrict__ x, int P, int C, float2* __restrict__ stats) {
  __shared__ float part[1024];
  const int S = 1024 / C;
  const int t = threadIdx.x, s = t / C, c = t - s * C;      // s == S: the threads left over, idle
  const float* xw = x + (size_t)blockIdx.x * P * C;
  const float shift = s < S ? xw[c] : 0.0f;
  float a = 0.0f;
  if (s < S)
    for (int p = s; p < P; p += S) a += xw[(size_t)p * C + c] - shift;
  part[t] = a;
  __syncthreads();
  slice_tree(part, S, C, s, c);
  const float mean = shift + part[c] / (float)P;
  __syncthreads();
  a = 0.0f;
  if (s < S)
    for (int p = s; p < P; p += S) {
      const float d = xw[(size_t)p * C + c] - mean;
      a += d * d;
    }
  part[t] = a;
  __syncthreads();
  slice_tree(part, S, C, s, c);
  if (t < C) stats[(size_t)blockIdx.x * C + t] = make_float2(mean, 1.0f / sqrtf(part[t] / (float)P + kSegEps));
}

constexpr int kConvGroups = 4, kConvPoolPerThread = 8, kConvPerThread = 3 * kConvPoolPerThread;
constexpr int kConvTilePool = kConvGroups * kConvPoolPerThread, kConvTile = 3 * kConvTilePool;

// in [n_win][n_in][CI], wT [CI * K][CO], out [n_win][n_pool][CO]; COP: threads of a group (CO rounded up to what divides the waves well)
template <int CI, int CO, int COP, int K, int STRIDE, bool FIRST>
__global__ __launch_bounds__(COP * kConvGroups) void seg_conv_pool_kernel(const float* __restrict__ in, int n_in, const float2* __restrict__ stats,
                                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                          const float* __restrict__ wT, const float* __restrict__ bias,
                                                                          float* __restrict__ out, int n_pool) {
  constexpr int SPAN = (kConvTile - 1) * STRIDE + K;
  __shared__ float xs[SPAN * CI];
  const int w = blockIdx.y;
  const int pos0 = blockIdx.x * kConvTile * STRIDE;      // first input position of the tile
  const float* xw = in + (size_t)w * n_in * CI;
  const float2* sw = stats + (size_t)w * CI;
  for (int idx = threadIdx.x; idx < SPAN * CI; idx += COP * kConvGroups) {
    const int pos = idx / CI, ci = idx - pos * CI;
    float v = 0.0f;
    if (pos0 + pos < n_in) {      // positions behind the end feed only pooled positions that are not stored
      const float2 ms = sw[ci];
      v = (xw[(size_t)(pos0 + pos) * CI + ci] - ms.x) * (ms.y * gamma[ci]) + beta[ci];
      if (!FIRST) v = leaky(v);
    }
    xs[idx] = v;
  }
  __syncthreads();
  const int g = threadIdx.x / COP, co = threadIdx.x - g * COP;
  const bool live = co < CO;
  float acc[kConvPerThread];
#pragma unroll
  for (int j = 0; j < kConvPerThread; ++j) acc[j] = 0.0f;
  const float* xg = xs + g * kConvPerThread * STRIDE * CI;
  const float* wc = wT + (live ? co : 0);
  auto tap = [&](int ci, int k) {
    const float wv = wc[(size_t)(ci * K + k) * CO];
#pragma unroll
    for (int j = 0; j < kConvPerThread; ++j) acc[j] = fmaf(xg[(j * STRIDE + k) * CI + ci], wv, acc[j]);
  };
  constexpr int KM = K / 5 * 5;      // 251 = 50 * 5 + 1
  for (int ci = 0; ci < CI; ++ci) {
#pragma unroll 1
    for (int k0 = 0; k0 < KM; k0 += 5) {
#pragma unroll
      for (int kk = 0; kk < 5; ++kk) tap(ci, k0 + kk);
    }
    for (int k = KM; k < K; ++k) tap(ci, k);
  }
  if (!live) return;
  const float b = FIRST ? 0.0f : bias[co];
  float* ow = out + (size_t)w * n_pool * CO;
#pragma unroll
  for (int pp = 0; pp < kConvPoolPerThread; ++pp) {
    const int p = blockIdx.x * kConvTilePool + g * kConvPoolPerThread + pp;
    float a0 = acc[3 * pp], a1 = acc[3 * pp + 1], a2 = acc[3 * pp + 2];
    if (FIRST) { a0 = fabsf(a0); a1 = fabsf(a1); a2 = fabsf(a2); }
    const float m = fmaxf(fmaxf(a0, a1), a2) + b;      // max(a + b) == max(a) + b: rounding is monotonic
    if (p < n_pool) ow[(size_t)p * CO + co] = m;
  }
}

__global__ __launch_bounds__(256) void seg_norm_kernel(const float* __restrict__ in, int per_win, int C, const float2* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= per_win) return;
  const int w = blockIdx.y, c = i % C;
  const float2 ms = stats[(size_t)w * C + c];
  const size_t at = (size_t)w * per_win + i;
  out[at] = leaky((in[at] - ms.x) * (ms.y * gamma[c]) + beta[c]);
}

constexpr int kProjTile = 64, kProjK = 16, kProjN = 2 * kSegGates;

// xproj [rows][1024] = x [rows][in] . w [1024][in]^T + b; in is a multiple of 4
__global__ __launch_bounds__(256) void seg_proj_kernel(const float* __restrict__ x, long rows, int in, const float* __restrict__ w,
                                                       const float* __restrict__ b, float* __restrict__ xproj) {
  __shared__ __attribute__((aligned(16))) float as[kProjK][kProjTile + 4];
  __shared__ __attribute__((aligned(16))) float ws[kProjK][kProjTile + 4];
  const long m0 = (long)blockIdx.y * kProjTile;
  const int n0 = blockIdx.x * kProjTile;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int lr = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;      // the row and the first k this thread loads
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  for (int k0 = 0; k0 < in; k0 += kProjK) {
    float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f), wv = av;      // zeros behind the last row and the last k add nothing
    if (k0 + lk < in) {
      if (m0 + lr < rows) av = *reinterpret_cast<const float4*>(x + (size_t)(m0 + lr) * in + k0 + lk);
      wv = *reinterpret_cast<const float4*>(w + (size_t)(n0 + lr) * in + k0 + lk);
    }
    __syncthreads();
    as[lk][lr] = av.x; as[lk + 1][lr] = av.y; as[lk + 2][lr] = av.z; as[lk + 3][lr] = av.w;
    ws[lk][lr] = wv.x; ws[lk + 1][lr] = wv.y; ws[lk + 2][lr] = wv.z; ws[lk + 3][lr] = wv.w;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kProjK; ++kk) {
      const float4 a = *reinterpret_cast<const float4*>(&as[kk][ty * 4]);
      const float4 bb = *reinterpret_cast<const float4*>(&ws[kk][tx * 4]);
      const float ar[4] = {a.x, a.y, a.z, a.w}, br[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ar[i], br[j], acc[i][j]);
    }
  }
  const float4 bv = *reinterpret_cast<const float4*>(b + n0 + tx * 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long m = m0 + ty * 4 + i;
    if (m < rows)
      *reinterpret_cast<float4*>(xproj + (size_t)m * kProjN + n0 + tx * 4) =
          make_float4(acc[i][0] + bv.x, acc[i][1] + bv.y, acc[i][2] + bv.z, acc[i][3] + bv.w);
  }
}

// xproj [n_win][frames][2][512], whh [2][512][128], y [n_win][frames][2][128]; grid 2 * n_win
__global__ __launch_bounds__(kSegGates) void seg_lstm_kernel(const float* __restrict__ xproj, const float* __restrict__ whh, int frames,
                                                             float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float h_s[kSegHidden];
  __shared__ float gate_s[kSegGates];
  const int g = threadIdx.x, w = blockIdx.x >> 1, dir = blockIdx.x & 1;
  float wr[kSegHidden];
  {
    const float4* src = reinterpret_cast<const float4*>(whh + ((size_t)dir * kSegGates + g) * kSegHidden);
#pragma unroll
    for (int k = 0; k < kSegHidden / 4; ++k) {
      const float4 v = src[k];
      wr[4 * k] = v.x; wr[4 * k + 1] = v.y; wr[4 * k + 2] = v.z; wr[4 * k + 3] = v.w;
    }
  }
  if (g < kSegHidden) h_s[g] = 0.0f;
  float c = 0.0f;
  __syncthreads();
  const float* xp = xproj + (size_t)w * frames * kProjN + dir * kSegGates + g;
  float* yo = y + (size_t)w * frames * (2 * kSegHidden) + dir * kSegHidden + g;
  const int dt = dir ? -1 : 1;
  int t = dir ? frames - 1 : 0;
  const bool is_cell = (g >> 7) == 2;      // rows 256 ... 383: the cell candidate (tanh); the same for a whole wave
  float x_next = xp[(size_t)t * kProjN];
  for (int s = 0; s < frames; ++s, t += dt) {
    const float xv = x_next;
    if (s + 1 < frames) x_next = xp[(size_t)(t + dt) * kProjN];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
    for (int k = 0; k < kSegHidden; k += 4) {
      const float4 hv = *reinterpret_cast<const float4*>(&h_s[k]);
      a0 = fmaf(wr[k], hv.x, a0);
      a1 = fmaf(wr[k + 1], hv.y, a1);
      a2 = fmaf(wr[k + 2], hv.z, a2);
      a3 = fmaf(wr[k + 3], hv.w, a3);
    }
    const float v = xv + ((a0 + a1) + (a2 + a3));
    gate_s[g] = is_cell ? tanhf(v) : 1.0f / (1.0f + expf(-v));
    __syncthreads();
    if (g < kSegHidden) {
      c = gate_s[kSegHidden + g] * c + gate_s[g] * gate_s[2 * kSegHidden + g];
      const float h = gate_s[3 * kSegHidden + g] * tanhf(c);
      h_s[g] = h;
      yo[(size_t)t * (2 * kSegHidden)] = h;
    }
    __syncthreads();
  }
}

constexpr int kHeadRows = 8;

__global__ __launch_bounds__(kSegHidden) void seg_head_kernel(const float* __restrict__ y, long rows, const float* __restrict__ l0,
                                                              const float* __restrict__ l0_b, const float* __restrict__ l1,
                                                              const float* __restrict__ l1_b, const float* __restrict__ cls,
                                                              const float* __restrict__ cls_b, float* __restrict__ scores) {
  __shared__ __attribute__((aligned(16))) float xs[kHeadRows][2 * kSegHidden];
  __shared__ __attribute__((aligned(16))) float h1[kHeadRows][2 * kSegHidden];      // the first half of a row is used
  __shared__ __attribute__((aligned(16))) float h2[kHeadRows][kSegHidden];
  __shared__ float lg[kHeadRows][8];
  const int j = threadIdx.x;
  const long m0 = (long)blockIdx.x * kHeadRows;
  for (int idx = j; idx < kHeadRows * 2 * kSegHidden; idx += kSegHidden) {
    const int r = idx / (2 * kSegHidden), k = idx - r * (2 * kSegHidden);
    xs[r][k] = m0 + r < rows ? y[(size_t)(m0 + r) * (2 * kSegHidden) + k] : 0.0f;
  }
  __syncthreads();
  // every dot product as four interleaved partial sums (k mod 4), joined as (s0 + s1) + (s2 + s3)
  float acc[kHeadRows][4];
  auto layer = [&](const float(*in)[2 * kSegHidden], int n_in, const float* __restrict__ wT) {
#pragma unroll
    for (int r = 0; r < kHeadRows; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[r][i] = 0.0f;
    for (int k = 0; k < n_in; k += 4) {
      float wv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) wv[i] = wT[(k + i) * kSegHidden + j];
#pragma unroll
      for (int r = 0; r < kHeadRows; ++r) {
        const float4 v = *reinterpret_cast<const float4*>(&in[r][k]);
        acc[r][0] = fmaf(v.x, wv[0], acc[r][0]);
        acc[r][1] = fmaf(v.y, wv[1], acc[r][1]);
        acc[r][2] = fmaf(v.z, wv[2], acc[r][2]);
        acc[r][3] = fmaf(v.w, wv[3], acc[r][3]);
      }
    }
  };
  layer(xs, 2 * kSegHidden, l0);
#pragma unroll
  for (int r = 0; r < kHeadRows; ++r) h1[r][j] = leaky(((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3])) + l0_b[j]);
  __syncthreads();
  layer(h1, kSegHidden, l1);
#pragma unroll
  for (int r = 0; r < kHeadRows; ++r) h2[r][j] = leaky(((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3])) + l1_b[j]);
  __syncthreads();
  if (j < kHeadRows * kSegClasses) {
    const int r = j / kSegClasses, cl = j - r * kSegClasses;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < kSegHidden; k += 4)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = fmaf(h2[r][k + i], cls[cl * kSegHidden + k + i], a[i]);
    lg[r][cl] = ((a[0] + a[1]) + (a[2] + a[3])) + cls_b[cl];
  }
  __syncthreads();
  if (j < kHeadRows && m0 + j < rows) {
    float mx = lg[j][0];
    for (int cl = 1; cl < kSegClasses; ++cl) mx = fmaxf(mx, lg[j][cl]);
    float sum = 0.0f;
    for (int cl = 0; cl < kSegClasses; ++cl) sum += expf(lg[j][cl] - mx);
    const float lse = mx + logf(sum);
    for (int cl = 0; cl < kSegClasses; ++cl) scores[(size_t)(m0 + j) * kSegClasses + cl] = lg[j][cl] - lse;
  }
}

}  // namespace

hipError_t launch_seg_windows(const void* d_pcm, int pcm_format, long n, long w0, int n_win, float* d_x, hipStream_t st) {
  const long total = (long)n_win * kSegWindow;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (pcm_format == CRISPY_PCM_F32)
    hipLaunchKernelGGL(seg_windows_kernel<true>, grid, dim3(256), 0, st, d_pcm, n, w0 * kSegWindow, total, d_x);
  else
    hipLaunchKernelGGL(seg_windows_kernel<false>, grid, dim3(256), 0, st, d_pcm, n, w0 * kSegWindow, total, d_x);
  return hipGetLastError();
}

hipError_t launch_seg_stats(const float* d_x, int n_win, int P, int C, float2* d_stats, hipStream_t st) {
  if (C < 1 || C > 1024 || P < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_stats_kernel, dim3(n_win), dim3(1024), 0, st, d_x, P, C, d_stats);
  return hipGetLastError();
}

hipError_t launch_seg_conv(int stage, const SegModel& m, const float* d_in, int n_win, int n_in, const float2* d_stats, float* d_out,
                           int n_pool, hipStream_t st) {
  if (n_pool < 1) return hipErrorInvalidValue;
  const dim3 grid((n_pool + kConvTilePool - 1) / kConvTilePool, n_win);
  if (stage == 0)
    hipLaunchKernelGGL((seg_conv_pool_kernel<1, kSegC0, 80, kSegTaps0, kSegStride0, true>), grid, dim3(80 * kConvGroups), 0, st, d_in, n_in,
                       d_stats, m.wav_g, m.wav_b, m.f0, static_cast<const float*>(nullptr), d_out, n_pool);
  else if (stage == 1)
    hipLaunchKernelGGL((seg_conv_pool_kernel<kSegC0, kSegC1, 64, kSegTaps, 1, false>), grid, dim3(64 * kConvGroups), 0, st, d_in, n_in,
                       d_stats, m.n_g[0], m.n_b[0], m.w1, m.b1, d_out, n_pool);
  else
    hipLaunchKernelGGL((seg_conv_pool_kernel<kSegC1, kSegC1, 64, kSegTaps, 1, false>), grid, dim3(64 * kConvGroups), 0, st, d_in, n_in,
                       d_stats, m.n_g[1], m.n_b[1], m.w2, m.b2, d_out, n_pool);
  return hipGetLastError();
}

hipError_t launch_seg_norm(const SegModel& m, const float* d_in, int n_win, int frames, const float2* d_stats, float* d_out, hipStream_t st) {
  const int per_win = frames * kSegC1;
  hipLaunchKernelGGL(seg_norm_kernel, dim3((per_win + 255) / 256, n_win), dim3(256), 0, st, d_in, per_win, kSegC1, d_stats, m.n_g[2], m.n_b[2],
                     d_out);
  return hipGetLastError();
}

hipError_t launch_seg_proj(const float* d_x, long rows, int in, const float* d_w, const float* d_b, float* d_xproj, hipStream_t st) {
  if (rows < 1 || in % 4 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_proj_kernel, dim3(kProjN / kProjTile, (unsigned)((rows + kProjTile - 1) / kProjTile)), dim3(256), 0, st, d_x, rows, in,
                     d_w, d_b, d_xproj);
  return hipGetLastError();
}

hipError_t launch_seg_lstm(const float* d_xproj, const float* d_whh, int n_win, int frames, float* d_y, hipStream_t st) {
  if (frames < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(seg_lstm_kernel, dim3(2 * n_win), dim3(kSegGates), 0, st, d_xproj, d_whh, frames, d_y);
  return hipGetLastError();
}

hipError_t launch_seg_head(const SegModel& m, const float* d_y, long rows, float* d_scores, hipStream_t st) {
  hipLaunchKernelGGL(seg_head_kernel, dim3((unsigned)((rows + kHeadRows - 1) / kHeadRows)), dim3(kSegHidden), 0, st, d_y, rows, m.l0, m.l0_b,
                     m.l1, m.l1_b, m.cls, m.cls_b, d_scores);
  return hipGetLastError();
}

}  // namespace diar
}  // namespace crispy

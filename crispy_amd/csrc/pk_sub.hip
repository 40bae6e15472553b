// pk_sub.hip -- the row kernels of the Parakeet FastConformer encoder for MI355X (gfx950): the subsampling convolutions, the
// LayerNorm, the position table and the convolution module's depthwise stage.  f32 operands and f32 sums; clips are ragged
// and lie end to end, PkTables says where each starts at every stage, and a workgroup reads its own clip's rows only.
//
//   pk_sub_conv0_kernel   Conv2d(1, C, 3, stride 2, pad 1) + ReLU: one output time row of one clip per workgroup, thread = channel,
//                         the three feature rows in LDS with their zero borders.  Images are [t][f][c], the channel contiguous.
//   pk_sub_dwpw_kernel    depthwise Conv2d(C, C, 3, stride 2, pad 1), Conv2d(C, C, 1) and ReLU in one: thread c forms the depthwise
//                         value of channel c at kSubNF frequencies of one output row (its 3 x 17 inputs are reads coalesced over
//                         c), puts them in LDS, then thread co sums the pointwise product over ci in four partial sums.  The
//                         depthwise image never reaches memory.  The last stage stores [t][c * F + f], the Linear's operand.
//   pk_layernorm_kernel   one row per workgroup, two passes (mean, then squared distances), both sums through one fixed tree.
//   pk_pos_kernel         the position table with f64 sin / cos of the single f32 product f32(d) * inv_freq[k].
//   pk_dwconv_kernel      depthwise K-tap Conv1d + folded BatchNorm + SiLU, thread = channel, 16 frames of one clip per workgroup.
#include <cmath>

#include "pk_internal.h"

namespace crispy {
namespace pk {
namespace {

__global__ __launch_bounds__(kMaxSubCh) void pk_sub_conv0_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                                 float* __restrict__ out, const int* __restrict__ off0,
                                                                 const int* __restrict__ off1, int M, int C) {
  extern __shared__ float xs[];      // [3][M + 2]
  const int clip = blockIdx.y, t = blockIdx.x;
  const int r0 = off0[clip], n0 = off0[clip + 1] - r0, q0 = off1[clip], n1 = off1[clip + 1] - q0;
  if (t >= n1) return;
  const int MP = M + 2;
  for (int idx = threadIdx.x; idx < 3 * MP; idx += blockDim.x) {
    const int kt = idx / MP, f = idx - kt * MP - 1, tt = 2 * t + kt - 1;
    xs[idx] = (tt >= 0 && tt < n0 && f >= 0 && f < M) ? x[(size_t)(r0 + tt) * M + f] : 0.0f;
  }
  __syncthreads();
  const int c = threadIdx.x;
  float wv[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) wv[k] = w[k * C + c];
  const float bias = b[c];
  const int F = M / 2;
  float* o = out + (size_t)(q0 + t) * F * C + c;
  for (int f = 0; f < F; ++f) {
    float a = bias;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt)
#pragma unroll
      for (int kf = 0; kf < 3; ++kf) a = fmaf(wv[kt * 3 + kf], xs[kt * MP + 2 * f + kf], a);
    o[(size_t)f * C] = fmaxf(a, 0.0f);
  }
}

__global__ __launch_bounds__(kMaxSubCh) void pk_sub_dwpw_kernel(const float* __restrict__ in, const float* __restrict__ dw_w,
                                                                const float* __restrict__ dw_b, const float* __restrict__ pw_w,
                                                                const float* __restrict__ pw_b, float* __restrict__ out,
                                                                const int* __restrict__ in_off, const int* __restrict__ out_off, int Fin,
                                                                int C, int flat) {
  __shared__ __attribute__((aligned(16))) float dwv[kMaxSubCh][kSubNF];
  const int clip = blockIdx.z, t = blockIdx.y, f0 = blockIdx.x * kSubNF;
  const int r0 = in_off[clip], nin = in_off[clip + 1] - r0, q0 = out_off[clip], nout = out_off[clip + 1] - q0;
  if (t >= nout) return;
  const int Fout = Fin / 2, c = threadIdx.x;
  float d[kSubNF];
  const float db = dw_b[c];
#pragma unroll
  for (int j = 0; j < kSubNF; ++j) d[j] = db;
  for (int kt = 0; kt < 3; ++kt) {
    const int tt = 2 * t + kt - 1;
    if (tt < 0 || tt >= nin) continue;      // the clip's own edge: zeros
    const float* row = in + (size_t)(r0 + tt) * Fin * C + c;
    float v[2 * kSubNF + 1];
#pragma unroll
    for (int i = 0; i < 2 * kSubNF + 1; ++i) {
      const int ff = 2 * f0 - 1 + i;
      v[i] = (ff >= 0 && ff < Fin) ? row[(size_t)ff * C] : 0.0f;
    }
    const float w0 = dw_w[(kt * 3) * C + c], w1 = dw_w[(kt * 3 + 1) * C + c], w2 = dw_w[(kt * 3 + 2) * C + c];
#pragma unroll
    for (int j = 0; j < kSubNF; ++j) d[j] = fmaf(w2, v[2 * j + 2], fmaf(w1, v[2 * j + 1], fmaf(w0, v[2 * j], d[j])));
  }
#pragma unroll
  for (int j = 0; j < kSubNF; ++j) dwv[c][j] = d[j];
  __syncthreads();
  float a[4][kSubNF];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int j = 0; j < kSubNF; ++j) a[p][j] = 0.0f;
  const float* wt = pw_w + c;      // [ci][co], this thread is co
  for (int ci = 0; ci < C; ci += 4) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float wv = wt[(size_t)(ci + p) * C];
      const float4 lo = *reinterpret_cast<const float4*>(&dwv[ci + p][0]), hi = *reinterpret_cast<const float4*>(&dwv[ci + p][4]);
      a[p][0] = fmaf(wv, lo.x, a[p][0]); a[p][1] = fmaf(wv, lo.y, a[p][1]); a[p][2] = fmaf(wv, lo.z, a[p][2]); a[p][3] = fmaf(wv, lo.w, a[p][3]);
      a[p][4] = fmaf(wv, hi.x, a[p][4]); a[p][5] = fmaf(wv, hi.y, a[p][5]); a[p][6] = fmaf(wv, hi.z, a[p][6]); a[p][7] = fmaf(wv, hi.w, a[p][7]);
    }
  }
  const float pb = pw_b[c];
#pragma unroll
  for (int j = 0; j < kSubNF; ++j) {
    const int f = f0 + j;
    if (f >= Fout) break;
    const float v = fmaxf(((a[0][j] + a[1][j]) + (a[2][j] + a[3][j])) + pb, 0.0f);
    const size_t row = (size_t)(q0 + t) * Fout * C;
    out[flat ? row + (size_t)c * Fout + f : row + (size_t)f * C + c] = v;
  }
}

// the sum of one value per thread of a 256-thread workgroup, the same in every thread: xor tree in the wave, then the four waves in order
__device__ inline float block_sum(float v, float* red) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();      // red may still be read from the call before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void pk_layernorm_kernel(const float* in, const float* __restrict__ g, const float* __restrict__ b, float* out,
                                                           int H) {      // in == out is allowed
  __shared__ float red[4];
  const float* x = in + (size_t)blockIdx.x * H;
  float* y = out + (size_t)blockIdx.x * H;
  float s = 0.0f;
  for (int i = threadIdx.x; i < H; i += 256) s += x[i];
  const float mean = block_sum(s, red) / (float)H;
  float q = 0.0f;
  for (int i = threadIdx.x; i < H; i += 256) {
    const float d = x[i] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(block_sum(q, red) / (float)H + (float)kEps);
  for (int i = threadIdx.x; i < H; i += 256) y[i] = fmaf((x[i] - mean) * rstd, g[i], b[i]);
}

__global__ __launch_bounds__(256) void pk_pos_kernel(const float* __restrict__ inv_freq, int tmax, int H, float* __restrict__ pos) {
  const int p = blockIdx.x;
  const float d = (float)(p - (tmax - 1));
  for (int k = threadIdx.x; k < H / 2; k += 256) {
    const float arg = __fmul_rn(d, inv_freq[k]);
    pos[(size_t)p * H + 2 * k] = (float)sin((double)arg);
    pos[(size_t)p * H + 2 * k + 1] = (float)cos((double)arg);
  }
}

constexpr int kDwTile = 16;

__global__ __launch_bounds__(128) void pk_dwconv_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ out, const int* __restrict__ off,
                                                        int H, int K) {
  const int clip = blockIdx.y, t0 = blockIdx.x * kDwTile, c = blockIdx.z * 128 + threadIdx.x;
  const int r0 = off[clip], n = off[clip + 1] - r0;
  if (t0 >= n) return;
  const int pad = (K - 1) / 2;
  const float sc = scale[c], sh = shift[c];
  const int t1 = min(n, t0 + kDwTile);
  for (int t = t0; t < t1; ++t) {
    float a = 0.0f;
    for (int k = 0; k < K; ++k) {
      const int tt = t + k - pad;
      if (tt >= 0 && tt < n) a = fmaf(w[k * H + c], in[(size_t)(r0 + tt) * H + c], a);
    }
    const float v = fmaf(a, sc, sh);
    out[(size_t)(r0 + t) * H + c] = v / (1.0f + expf(-v));
  }
}

}  // namespace

hipError_t launch_sub_conv0(const PkModel& m, const PkTables& t, const float* d_feats, int M, int C, float* d_out, hipStream_t st) {
  if (t.n_clips < 1 || t.max_len[1] < 1 || C < 1 || C > kMaxSubCh) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_sub_conv0_kernel, dim3(t.max_len[1], t.n_clips), dim3(C), 3 * (M + 2) * sizeof(float), st, d_feats, m.conv0_w, m.conv0_b,
                     d_out, t.off[0], t.off[1], M, C);
  return hipGetLastError();
}

hipError_t launch_sub_dwpw(int s, const PkModel& m, const PkTables& t, const float* d_in, int F, int C, float* d_out, bool flat, hipStream_t st) {
  if (s < 1 || s > 2 || t.n_clips < 1 || t.max_len[s + 1] < 1 || C < 4 || C % 4 != 0 || C > kMaxSubCh || F < 2 || F % 2 != 0) return hipErrorInvalidValue;
  const int Fout = F / 2;
  hipLaunchKernelGGL(pk_sub_dwpw_kernel, dim3((Fout + kSubNF - 1) / kSubNF, t.max_len[s + 1], t.n_clips), dim3(C), 0, st, d_in, m.dw_w[s - 1],
                     m.dw_b[s - 1], m.pw_w[s - 1], m.pw_b[s - 1], d_out, t.off[s], t.off[s + 1], F, C, flat ? 1 : 0);
  return hipGetLastError();
}

hipError_t launch_layernorm(const float* d_in, const float* g, const float* b, float* d_out, long rows, int H, hipStream_t st) {
  if (rows < 1 || rows > 0x7fffffffL || H < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_layernorm_kernel, dim3((unsigned)rows), dim3(256), 0, st, d_in, g, b, d_out, H);
  return hipGetLastError();
}

hipError_t launch_pos_table(const float* inv_freq, int tmax, int H, float* d_pos, hipStream_t st) {
  if (tmax < 1 || H < 2 || H % 2 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_pos_kernel, dim3(2 * tmax - 1), dim3(256), 0, st, inv_freq, tmax, H, d_pos);
  return hipGetLastError();
}

hipError_t launch_dwconv(const PkLayer& l, const PkTables& t, const float* d_in, int H, int K, float* d_out, hipStream_t st) {
  if (t.n_clips < 1 || t.max_len[3] < 1 || H % 128 != 0 || K < 1 || K > kMaxTaps || K % 2 == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pk_dwconv_kernel, dim3((t.max_len[3] + kDwTile - 1) / kDwTile, t.n_clips, H / 128), dim3(128), 0, st, d_in, l.dw_w, l.dw_scale,
                     l.dw_shift, d_out, t.off[3], H, K);
  return hipGetLastError();
}

}  // namespace pk
}  // namespace crispy

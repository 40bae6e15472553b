// pk_attn.hip -- the relative-position attention (Transformer-XL form) of the Parakeet encoder for MI355X (gfx950), exact f32 on
// v_mfma_f32_32x32x2_f32.  score(i, j) = ((q_i + u) . k_j + (q_i + v) . r_{i - j}) / sqrt(128), soft-max over the clip's own
// keys, times V.  One workgroup (four waves) per (clip, head, tile of 32 queries); keys come in tiles of 32 with a running
// maximum and sum, so there is no [T'][T'] buffer.
//
// For the query tile at i0 and the key tile at j0 the position term needs only r_d with d = i0 - j0 - 31 ... i0 - j0 + 31: that
// band of 63 rows of R goes to LDS, (Q + v) . R_band^T is one 32 x 64 product, and entry (i, j) is read at column i - j + 31.
// Per key tile: wave 0 forms (Q + u) . K^T, waves 1 and 2 the two halves of the band product (wave 3 has no product to form),
// each with its Q operand in 64 registers for the whole workgroup; then eight threads per query row take the tile's maximum
// and sum through one fixed tree and write P; then every wave adds P . V for its 32 of the 128 output columns onto its
// rescaled accumulator.  The V tile waits in registers while the scores are formed and then takes the K tile's place in LDS:
// 68 KB per workgroup, two workgroups per CU.  Everything is indexed from the clip's own first
// frame, rows and keys behind its last are zeros that are masked (keys) or never stored (queries): a clip's frames do not
// depend on the batch or on its neighbours.
#include <cmath>

#include "pk_internal.h"

namespace crispy {
namespace pk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = kHeadDim, kPad = 33, kBand = 64, kBandPad = 65;
static_assert(kAttnQ == 32 && kAttnK == 32 && kD == 128, "the wave roles below are written for 32 x 32 tiles of 128-wide heads");
// floats: k^T [128][33] (first q^T, and v [32][128] once the scores are formed), band [128][65], s_ac [32][33], s_bd [32][65],
// p^T [32][33], u, v [128], factor [32]
constexpr int kOffK = 0, kOffR = kOffK + kD * kPad, kOffSac = kOffR + kD * kBandPad, kOffSbd = kOffSac + kAttnQ * kPad,
              kOffP = kOffSbd + kAttnQ * kBandPad, kOffU = kOffP + kAttnK * kPad, kOffBv = kOffU + kD, kOffFac = kOffBv + kD,
              kAttnFloats = kOffFac + kAttnQ;
static_assert(kAttnK * kD <= kD * kPad, "the V tile takes the K tile's place");

// A [32][128] (this lane's operands of the 64 steps in qa) times B^T, B in LDS as [dim][column] with row stride LD and b at
// this lane's first element: two chains of 64 terms, added in order.  Unrolled in full: qa and the LDS offsets are constants.
template <int LD>
__device__ inline f32x16 tile_product(const float (&qa)[kD / 2], const float* b) {
  f32x16 acc, tot;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = tot[i] = 0.0f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int kk = half * 64; kk < half * 64 + 64; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[kk / 2], b[kk * LD], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      tot[i] += acc[i];
      acc[i] = 0.0f;
    }
  }
  return tot;
}

__global__ __launch_bounds__(256, 2) void pk_attn_kernel(const float* __restrict__ qkv, const float* __restrict__ r, const float* __restrict__ bias_u,
                                                      const float* __restrict__ bias_v, float* __restrict__ out, const int* __restrict__ off,
                                                      int H, int tmax) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* kt = sm + kOffK;      // [dim][key]; before the first tile [dim][query]
  float* vs = sm + kOffK;      // [key][dim], in the K tile's place from the soft-max on
  float* rb = sm + kOffR;      // [dim][band column]
  float* sac = sm + kOffSac;   // [query][key]
  float* sbd = sm + kOffSbd;   // [query][band column]
  float* pt = sm + kOffP;      // [key][query]
  float* us = sm + kOffU;
  float* bvs = sm + kOffBv;
  float* fac = sm + kOffFac;
  const int clip = blockIdx.z, head = blockIdx.y, i0 = blockIdx.x * kAttnQ;
  const int r0 = off[clip], n = off[clip + 1] - r0;
  if (i0 >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lk = lane >> 5;
  const size_t ld = (size_t)3 * H;
  const float* qbase = qkv + (size_t)r0 * ld + (size_t)head * kD;
  for (int idx = tid; idx < kAttnQ * kD; idx += 256) {
    const int i = idx >> 7, d = idx & (kD - 1);
    kt[d * kPad + i] = (i0 + i < n) ? qbase[(size_t)(i0 + i) * ld + d] : 0.0f;
  }
  if (tid < kD) {
    us[tid] = bias_u[head * kD + tid];
    bvs[tid] = bias_v[head * kD + tid];
  }
  __syncthreads();
  float qa[kD / 2];      // this lane's A operands of the 64 steps: Q + u in wave 0, Q + v in waves 1 and 2
  {
    const float* add = wave == 0 ? us : bvs;
#pragma unroll
    for (int s = 0; s < kD / 2; ++s) qa[s] = kt[(2 * s + lk) * kPad + li] + add[2 * s + lk];
  }
  const float scale = 0.08838834764831845f;      // 128^-1/2
  const int srow = tid >> 3, ssub = tid & 7;      // the soft-max's row and its four keys
  float m_run = -INFINITY, l_run = 0.0f;
  f32x16 o;
#pragma unroll
  for (int i = 0; i < 16; ++i) o[i] = 0.0f;
  for (int j0 = 0; j0 < n; j0 += kAttnK) {
    __syncthreads();      // the tile before has been read
    float vr[kAttnK * kD / 256];
#pragma unroll
    for (int it = 0; it < kAttnK * kD / 256; ++it) {
      const int idx = tid + 256 * it, j = idx >> 7, d = idx & (kD - 1);
      const bool in = j0 + j < n;
      const float* row = qbase + (size_t)(j0 + j) * ld + d;
      kt[d * kPad + j] = in ? row[H] : 0.0f;
      vr[it] = in ? row[2 * H] : 0.0f;
    }
    for (int idx = tid; idx < kBand * kD; idx += 256) {
      const int b = idx >> 7, d = idx & (kD - 1);
      const int p = i0 - j0 - (kAttnK - 1) + b + (tmax - 1);
      rb[d * kBandPad + b] = (b < kAttnQ + kAttnK - 1 && p >= 0 && p < 2 * tmax - 1) ? r[(size_t)p * H + head * kD + d] : 0.0f;
    }
    __syncthreads();
    if (wave < 3) {
      const f32x16 tot = wave == 0 ? tile_product<kPad>(qa, kt + lk * kPad + li) : tile_product<kBandPad>(qa, rb + lk * kBandPad + (wave - 1) * 32 + li);
      // C/D of the 32 x 32 form: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * lk;
        if (wave == 0) sac[row * kPad + li] = tot[i];
        else sbd[row * kBandPad + (wave - 1) * 32 + li] = tot[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kAttnK * kD / 256; ++it) vs[tid + 256 * it] = vr[it];      // [key][dim] is the order of the load
    {
      float s[4], mx = -INFINITY;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j = ssub * 4 + q;
        s[q] = (j0 + j < n) ? (sac[srow * kPad + j] + sbd[srow * kBandPad + srow - j + (kAttnK - 1)]) * scale : -INFINITY;
        mx = fmaxf(mx, s[q]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
      const float m_new = fmaxf(m_run, mx);      // finite: key j0 is the clip's own
      const float alpha = expf(m_run - m_new);
      float sum = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float p = expf(s[q] - m_new);
        pt[(ssub * 4 + q) * kPad + srow] = p;
        sum += p;
      }
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 4, 64);
      l_run = fmaf(l_run, alpha, sum);
      m_run = m_new;
      if (ssub == 0) fac[srow] = alpha;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] *= fac[(i & 3) + 8 * (i >> 2) + 4 * lk];
#pragma unroll
    for (int kk = 0; kk < kAttnK; kk += 2) o = __builtin_amdgcn_mfma_f32_32x32x2f32(pt[(kk + lk) * kPad + li], vs[(kk + lk) * kD + wave * 32 + li], o, 0, 0, 0);
  }
  __syncthreads();
  if (ssub == 0) fac[srow] = l_run;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = (i & 3) + 8 * (i >> 2) + 4 * lk;
    if (i0 + row < n) out[(size_t)(r0 + i0 + row) * H + head * kD + wave * 32 + li] = o[i] / fac[row];
  }
}

}  // namespace

hipError_t launch_attention(const PkLayer& l, const PkTables& t, const float* d_qkv, const float* d_r, int tmax, int heads, float* d_out, hipStream_t st) {
  if (t.n_clips < 1 || t.max_len[3] < 1 || tmax < t.max_len[3] || heads < 1) return hipErrorInvalidValue;
  const size_t smem = kAttnFloats * sizeof(float);
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pk_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pk_attn_kernel, dim3((t.max_len[3] + kAttnQ - 1) / kAttnQ, heads, t.n_clips), dim3(256), smem, st, d_qkv, d_r, l.bias_u, l.bias_v,
                     d_out, t.off[3], heads * kD, tmax);
  return hipGetLastError();
}

}  // namespace pk
}  // namespace crispy

// pk_gemm.hip -- every Linear and 1x1 convolution of the Parakeet encoder for MI355X (gfx950) on v_mfma_f32_32x32x2_f32: exact f32
// operands and sums.  64 x 128 tiles, four waves of 32 x 64, as the embedding network's GEMM (diar_emb.hip); K = H, ffn or
// C * M / 8.  k runs in ascending order in blocks of 32; two blocks form one chain of 64 terms that starts from zero, and the
// chains are added in order, so an element's sum depends on K alone, never on where its row sits in a tile or in the launch.
// The LayerNorm runs as a row pass in front (pk_sub.hip); the store carries the bias and one of: a scale, SiLU, the residual with
// its factor, or the GLU of a value / gate column pair that pointwise_conv1's column order puts into one lane.
#include <cmath>

#include "pk_internal.h"

namespace crispy {
namespace pk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kGemmM = 64, kGemmN = 128, kGemmK = 32, kGemmFold = 2;

template <int EPI>
__global__ __launch_bounds__(256) void pk_gemm_kernel(const float* __restrict__ A, int K, const float* __restrict__ Bt, int N,
                                                      const float* __restrict__ bias, float alpha, const float* res, float* C, int ldc, long M) {
  __shared__ float as[kGemmK][kGemmM + 1];      // [k][row]: the lanes of an operand load read consecutive rows
  __shared__ __attribute__((aligned(16))) float bs[kGemmK][kGemmN];
  const long m0 = (long)blockIdx.x * kGemmM;
  const int n0 = blockIdx.y * kGemmN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 64;
  const int li = lane & 31, lk = lane >> 5;
  const int ar = tid >> 3, ak = (tid & 7) * 4;      // the row (and row + 32) and the first k of this thread's A loads
  f32x16 acc0, acc1, tot0, tot1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = tot0[i] = tot1[i] = 0.0f;
  const int n_tiles = K / kGemmK;
  for (int kt = 0; kt < n_tiles; ++kt) {
    const int k0 = kt * kGemmK;
    __syncthreads();      // the previous tile's operand reads are over
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const long m = m0 + ar + 32 * p;
      float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // rows behind the last: never stored
      if (m < M) x = *reinterpret_cast<const float4*>(A + (size_t)m * K + k0 + ak);
      as[ak][ar + 32 * p] = x.x; as[ak + 1][ar + 32 * p] = x.y; as[ak + 2][ar + 32 * p] = x.z; as[ak + 3][ar + 32 * p] = x.w;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = tid + 256 * p;
      *reinterpret_cast<float4*>(&bs[idx >> 5][(idx & 31) * 4]) =
          *reinterpret_cast<const float4*>(Bt + (size_t)(k0 + (idx >> 5)) * N + n0 + (idx & 31) * 4);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kGemmK; kk += 2) {
      const float a = as[kk + lk][wm + li];
      const float b0 = bs[kk + lk][wn + li], b1 = bs[kk + lk][wn + 32 + li];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
    }
    if ((kt + 1) % kGemmFold == 0 || kt + 1 == n_tiles) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        tot0[i] += acc0[i];
        tot1[i] += acc1[i];
        acc0[i] = acc1[i] = 0.0f;
      }
    }
  }
  // C/D of the 32 x 32 form: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int c0 = n0 + wn + li, c1 = c0 + 32;
  const float bias0 = bias ? bias[c0] : 0.0f, bias1 = bias ? bias[c1] : 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * lk;
    if (m >= M) continue;
    const float v0 = tot0[i] + bias0, v1 = tot1[i] + bias1;
    float* row = C + (size_t)m * ldc;
    if (EPI == kGemmGlu) {
      row[(n0 + wn) / 2 + li] = v0 / (1.0f + expf(-v1));
    } else if (EPI == kGemmSilu) {
      row[c0] = v0 / (1.0f + expf(-v0));
      row[c1] = v1 / (1.0f + expf(-v1));
    } else if (EPI == kGemmResidual) {
      const float* r = res + (size_t)m * ldc;
      const float r0 = r[c0], r1 = r[c1];
      row[c0] = fmaf(alpha, v0, r0);
      row[c1] = fmaf(alpha, v1, r1);
    } else {
      row[c0] = v0 * alpha;
      row[c1] = v1 * alpha;
    }
  }
}

}  // namespace

hipError_t launch_gemm(GemmEpilogue e, const float* d_a, int K, const float* d_bt, const float* bias, int N, float alpha, const float* d_res,
                       float* d_c, long M, hipStream_t st) {
  const int cols = e == kGemmGlu ? 2 * N : N;
  if (M < 1 || K < kGemmK || K % kGemmK != 0 || cols % kGemmN != 0 || (e == kGemmResidual && !d_res)) return hipErrorInvalidValue;
  const long tiles = (M + kGemmM - 1) / kGemmM;
  if (tiles > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles, cols / kGemmN);
  switch (e) {
    case kGemmScale: hipLaunchKernelGGL(pk_gemm_kernel<kGemmScale>, grid, dim3(256), 0, st, d_a, K, d_bt, cols, bias, alpha, d_res, d_c, N, M); break;
    case kGemmSilu: hipLaunchKernelGGL(pk_gemm_kernel<kGemmSilu>, grid, dim3(256), 0, st, d_a, K, d_bt, cols, bias, alpha, d_res, d_c, N, M); break;
    case kGemmResidual: hipLaunchKernelGGL(pk_gemm_kernel<kGemmResidual>, grid, dim3(256), 0, st, d_a, K, d_bt, cols, bias, alpha, d_res, d_c, N, M); break;
    case kGemmGlu: hipLaunchKernelGGL(pk_gemm_kernel<kGemmGlu>, grid, dim3(256), 0, st, d_a, K, d_bt, cols, bias, alpha, d_res, d_c, N, M); break;
  }
  return hipGetLastError();
}

// The encoder's form: the handle's precision mode picks the f32 kernel above or the f16-operand one of pk_gemm_f16.hip.
hipError_t launch_gemm(int mode, GemmEpilogue e, const float* d_a, int K, const float* d_bt, const void* d_bp, const float* bias, int N, float alpha,
                       const float* d_res, float* d_c, long M, hipStream_t st) {
  if (mode == 1) return launch_gemm_f16(e, d_a, K, d_bp, bias, N, alpha, d_res, d_c, M, st);
  if (mode != 0) return hipErrorInvalidValue;
  return launch_gemm(e, d_a, K, d_bt, bias, N, alpha, d_res, d_c, M, st);
}

}  // namespace pk
}  // namespace crispy

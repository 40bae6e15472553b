// pk_gemm_f16.hip -- precision mode 1 of the Parakeet encoder's GEMMs for MI355X (gfx950): both operands rounded once to IEEE
// binary16 (round to nearest even, subnormals kept, overflow to infinity), f32 sums on v_mfma_f32_32x32x16_f16.  128 x 128 tiles,
// four waves of 64 x 64 (2 x 2 accumulators of 32 x 32), k tiles of 32.  The weights come pre-packed in operand order
// (pk_pack_f16_kernel), so a lane's B fragment of one 16-deep step is one 16-byte load straight from global memory; A is read as
// f32, rounded on the way into LDS (64-byte rows, the 16-byte chunk XORed with (row >> 2) & 3 so that the row reads of an
// operand are conflict-free) and read back as one ds_read_b128 per fragment.  The loads of tile t + 1 are in flight while tile t
// is multiplied; the two LDS images alternate, one barrier per tile.  An element has ONE accumulator over all of K: k ascending
// in steps of 16, a chain of K / 16 matrix instructions that starts from zero, so its sum depends on K alone, never on where its
// row sits in a tile or in the launch.  The store is pk_gemm_kernel's: bias, then a scale, SiLU, the residual or the GLU, in f32.
#include <cmath>
#include <cstdint>

#include "pk_internal.h"

namespace crispy {
namespace pk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int kHalfM = 128, kHalfN = 128, kHalfK = 32, kHalfStep = 16;

// halves from the start of an A image to the 16-byte chunk `chunk` (0 ... 3) of row `row`
__device__ __forceinline__ int a_chunk(int row, int chunk) { return row * kHalfK + ((chunk ^ ((row >> 2) & 3)) << 3); }

template <int EPI>
__global__ __launch_bounds__(256) void pk_gemm_f16_kernel(const float* __restrict__ A, int K, const uint4* __restrict__ Bp, int N,
                                                          const float* __restrict__ bias, float alpha, const float* res, float* C, int ldc, long M) {
  __shared__ __attribute__((aligned(16))) _Float16 as[2][kHalfM * kHalfK];
  const long m0 = (long)blockIdx.x * kHalfM;
  const int n0 = blockIdx.y * kHalfN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  const int li = lane & 31, lh = lane >> 5;
  const int ar = tid >> 3, ak = (tid & 7) * 4;      // the row (and row + 32 p) and the first k of this thread's A loads
  const int steps = K / kHalfStep, n_tiles = K / kHalfK;
  // the packed image: [column block of 32][step of 16][lane][8 halves]
  const uint4* b0 = Bp + (size_t)((n0 + wn) / 32) * steps * 64 + lane;
  const uint4* b1 = b0 + (size_t)steps * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[0][0][i] = acc[0][1][i] = acc[1][0][i] = acc[1][1][i] = 0.0f;
  float4 an[4];
  uint4 bn[2][2];      // [column block][step]
  auto load = [&](int kt) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const long m = m0 + ar + 32 * p;
      an[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // rows behind the last: never stored
      if (m < M) an[p] = *reinterpret_cast<const float4*>(A + (size_t)m * K + kt * kHalfK + ak);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bn[0][s] = b0[(size_t)(2 * kt + s) * 64];
      bn[1][s] = b1[(size_t)(2 * kt + s) * 64];
    }
  };
  load(0);
  for (int kt = 0; kt < n_tiles; ++kt) {
    _Float16* img = as[kt & 1];      // last read in tile kt - 2, and every wave has passed tile kt - 1's barrier since
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      f16x4 v;
      v[0] = (_Float16)an[p].x; v[1] = (_Float16)an[p].y; v[2] = (_Float16)an[p].z; v[3] = (_Float16)an[p].w;
      *reinterpret_cast<f16x4*>(img + a_chunk(ar + 32 * p, ak >> 3) + (ak & 4)) = v;
    }
    uint4 bc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bc[0][s] = bn[0][s];
      bc[1][s] = bn[1][s];
    }
    __syncthreads();
    if (kt + 1 < n_tiles) load(kt + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // A of the 32 x 32 x 16 form: lane l holds row l & 31, k = 8 (l >> 5) + j in element j; B likewise with its column
      const f16x8 a0 = *reinterpret_cast<const f16x8*>(img + a_chunk(wm + li, 2 * s + lh));
      const f16x8 a1 = *reinterpret_cast<const f16x8*>(img + a_chunk(wm + 32 + li, 2 * s + lh));
      const f16x8 f0 = __builtin_bit_cast(f16x8, bc[0][s]), f1 = __builtin_bit_cast(f16x8, bc[1][s]);
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, f0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, f1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, f0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, f1, acc[1][1], 0, 0, 0);
    }
  }
  // C/D of the 32 x 32 form: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int c0 = n0 + wn + li, c1 = c0 + 32;
  const float bias0 = bias ? bias[c0] : 0.0f, bias1 = bias ? bias[c1] : 0.0f;
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long m = m0 + wm + 32 * rb + (i & 3) + 8 * (i >> 2) + 4 * lh;
      if (m >= M) continue;
      const float v0 = acc[rb][0][i] + bias0, v1 = acc[rb][1][i] + bias1;
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
}

// f32 [K][N] -> the packed f16 image [N / 32][K / 16][64 lanes][8]: lane l of (column block, step) holds column 32 block + (l & 31),
// k = 16 step + 8 (l >> 5) + j in element j.  The columns keep the order of the f32 matrix (q | k | v, the GLU groups).
__global__ __launch_bounds__(256) void pk_pack_f16_kernel(const float* __restrict__ Bt, int K, int N, uint4* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int steps = K / kHalfStep;
  if (idx >= (size_t)(N / 32) * steps * 64) return;
  const int lane = (int)(idx & 63);
  const size_t frag = idx >> 6;
  const int step = (int)(frag % steps), block = (int)(frag / steps);
  const float* src = Bt + (size_t)(step * kHalfStep + 8 * (lane >> 5)) * N + block * 32 + (lane & 31);
  f16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (_Float16)src[(size_t)j * N];
  out[idx] = __builtin_bit_cast(uint4, v);
}

// The state dict's [cols][K] -> the [K][cols] of the handle's device copy, as crispy_pk_load's host code lays it out; with `glu`
// output channel o goes to column glu_column(o, cols / 2).  Only crispy_pk_stage_gemm_device runs it.
__global__ __launch_bounds__(256) void pk_transpose_kernel(const float* __restrict__ w, int K, int cols, int glu, float* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)K * cols) return;
  const size_t o = idx / (size_t)K, k = idx % (size_t)K;
  const size_t col = glu ? glu_column(o, (size_t)cols / 2) : o;
  out[k * cols + col] = w[idx];
}

}  // namespace

hipError_t launch_gemm_f16(GemmEpilogue e, const float* d_a, int K, const void* d_bp, const float* bias, int N, float alpha, const float* d_res,
                           float* d_c, long M, hipStream_t st) {
  const int cols = e == kGemmGlu ? 2 * N : N;
  if (!d_bp || M < 1 || K < kHalfK || K % kHalfK != 0 || cols % kHalfN != 0 || (e == kGemmResidual && !d_res)) return hipErrorInvalidValue;
  const long tiles = (M + kHalfM - 1) / kHalfM;
  if (tiles > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)tiles, cols / kHalfN);
  const uint4* bp = static_cast<const uint4*>(d_bp);
  switch (e) {
    case kGemmScale: hipLaunchKernelGGL(pk_gemm_f16_kernel<kGemmScale>, grid, dim3(256), 0, st, d_a, K, bp, cols, bias, alpha, d_res, d_c, N, M); break;
    case kGemmSilu: hipLaunchKernelGGL(pk_gemm_f16_kernel<kGemmSilu>, grid, dim3(256), 0, st, d_a, K, bp, cols, bias, alpha, d_res, d_c, N, M); break;
    case kGemmResidual: hipLaunchKernelGGL(pk_gemm_f16_kernel<kGemmResidual>, grid, dim3(256), 0, st, d_a, K, bp, cols, bias, alpha, d_res, d_c, N, M); break;
    case kGemmGlu: hipLaunchKernelGGL(pk_gemm_f16_kernel<kGemmGlu>, grid, dim3(256), 0, st, d_a, K, bp, cols, bias, alpha, d_res, d_c, N, M); break;
  }
  return hipGetLastError();
}

hipError_t launch_pack_f16(const float* d_bt, int K, int cols, void* d_out, hipStream_t st) {
  if (K < kHalfK || K % kHalfK != 0 || cols < kHalfN || cols % kHalfN != 0) return hipErrorInvalidValue;
  const size_t n = (size_t)K * cols / 8;
  hipLaunchKernelGGL(pk_pack_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_bt, K, cols, static_cast<uint4*>(d_out));
  return hipGetLastError();
}

hipError_t launch_weight_transpose(const float* d_w, int K, int cols, bool glu, float* d_bt, hipStream_t st) {
  const size_t n = (size_t)K * cols;
  hipLaunchKernelGGL(pk_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_w, K, cols, glu ? 1 : 0, d_bt);
  return hipGetLastError();
}

}  // namespace pk
}  // namespace crispy

// diar_emb.hip -- the speaker-embedding network of the diarization path for MI355X (gfx950): WeSpeaker CAMPPlus ("CAM++"), the
// session.run of EmbeddingExtractor::compute (src-tauri/src/managers/diarization.rs:53-75).  f32 operands and f32 sums
// everywhere.  Chunks are ragged and lie end to end; a turn's offset tables (EmbTables) say where each starts.  The head works
// on rows [t][f][c] (the channel contiguous), everything from the tdnn on on time-major rows [position][channel]; a dense
// block is one buffer [t2][C_final] whose layers append their 32 channels in place.
//
//   emb_conv2d_kernel   one 3x3 (or 1x1 shortcut) convolution of the head: a workgroup takes one time row of one chunk for all
//                       frequencies and channels.  The three input rows go to LDS with their zero borders; thread (group, co)
//                       keeps NF frequencies, reads four weights (contiguous over co) per four input channels and the inputs
//                       as LDS broadcasts of float4.  BatchNorm, the residual and the ReLU in the store.
//   emb_tdnn_kernel     Conv1d(320, 128, 5, stride 2): 8 output positions of one chunk per workgroup, 19 input rows in LDS.
//   emb_gemm_kernel     every 1x1 convolution (linear1 of the 52 dense layers, the three transits) on v_mfma_f32_32x32x2_f32:
//                       64 x 128 tiles, four waves of 32 x 64.  The BatchNorm + ReLU in front goes into the A load, the one
//                       behind into the store.  k runs in ascending order in blocks of 64; each block's chain starts from zero
//                       and the blocks are added in order, so an element's sum depends on K alone, never on where its row
//                       sits in a tile or in the launch.
//   emb_gates_kernel    one workgroup per chunk: the sums of h over each context segment (four strided slices per channel,
//                       joined in a fixed tree), the chunk's sum as the segments' in order, then per segment the two small
//                       linear layers and the sigmoid.  No atomics; a chunk reads its own rows only.
//   emb_local_kernel    linear_local (k 3, dilation d) on 16 positions of one chunk per workgroup, times the gate of the
//                       position's segment, stored at the layer's channel offset of the block's buffer.
//   emb_pool_kernel     mean and sqrt(unbiased variance + 1e-7) over a chunk's positions, two passes, four partial sums each.
//   emb_dense_kernel    Conv1d(1024, dim, 1) and the affine-free BatchNorm.
// Sums of more than 64 terms are split over two or four partial sums that are joined pairwise.
#include <cmath>

#include "diar_internal.h"

namespace crispy {
namespace diar {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- head -----------------------------------------------------------------------------------------------------------
// in [rows][FIN][CIN], w [(kf * KS + kt) * CIN + ci][32], out [rows][FIN / FS][32] (transposed: [rows][32][FIN / FS])
template <int CIN, int FIN, int KS, int FS>
__global__ __launch_bounds__(256) void emb_conv2d_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, const float* __restrict__ res, float* __restrict__ out,
                                                         const int* __restrict__ row_off, int relu, int transposed) {
  constexpr int PAD = KS / 2, FP = FIN + 2 * PAD, FOUT = FIN / FS, NF = FOUT == 80 ? 10 : 5, G = FOUT / NF;
  __shared__ __attribute__((aligned(16))) float xs[KS * FP * CIN];
  const int c = blockIdx.y, t = blockIdx.x;
  const int r0 = row_off[c], n = row_off[c + 1] - r0;
  if (t >= n) return;
  const int tid = threadIdx.y * 32 + threadIdx.x;
  for (int idx = tid; idx < KS * FP * CIN; idx += 32 * G) {
    const int kt = idx / (FP * CIN), rest = idx - kt * (FP * CIN), fi = rest / CIN, ci = rest - fi * CIN;
    const int tt = t + kt - PAD, f = fi - PAD;
    xs[idx] = (tt >= 0 && tt < n && f >= 0 && f < FIN) ? in[((size_t)(r0 + tt) * FIN + f) * CIN + ci] : 0.0f;
  }
  __syncthreads();
  const int co = threadIdx.x, g = threadIdx.y;
  float a0[NF], a1[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) a0[j] = a1[j] = 0.0f;
#pragma unroll
  for (int kf = 0; kf < KS; ++kf)
#pragma unroll
    for (int kt = 0; kt < KS; ++kt) {
      const float* wt = w + (size_t)(kf * KS + kt) * CIN * kEmbHeadCh + co;
      const float* xr = xs + (kt * FP + g * NF * FS + kf) * CIN;
      if constexpr (CIN == 1) {
        const float wv = wt[0];
#pragma unroll
        for (int j = 0; j < NF; ++j) a0[j] = fmaf(xr[j * FS], wv, a0[j]);
      } else {
#pragma unroll 2
        for (int ci = 0; ci < CIN; ci += 4) {
          const float w0 = wt[ci * kEmbHeadCh], w1 = wt[(ci + 1) * kEmbHeadCh], w2 = wt[(ci + 2) * kEmbHeadCh], w3 = wt[(ci + 3) * kEmbHeadCh];
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            const float4 v = *reinterpret_cast<const float4*>(xr + j * FS * CIN + ci);
            a0[j] = fmaf(v.x, w0, a0[j]);
            a1[j] = fmaf(v.y, w1, a1[j]);
            a0[j] = fmaf(v.z, w2, a0[j]);
            a1[j] = fmaf(v.w, w3, a1[j]);
          }
        }
      }
    }
  const float sc = scale[co], sh = shift[co];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    const int f = g * NF + j;
    const size_t at = ((size_t)(r0 + t) * FOUT + f) * kEmbHeadCh + co;
    float v = fmaf(a0[j] + a1[j], sc, sh);
    if (res) v += res[at];
    if (relu) v = fmaxf(v, 0.0f);
    out[transposed ? ((size_t)(r0 + t) * kEmbHeadCh + co) * FOUT + f : at] = v;
  }
}

// ---- tdnn -----------------------------------------------------------------------------------------------------------
constexpr int kTdnnTile = 8, kTdnnSpan = (kTdnnTile - 1) * kEmbTdnnStride + kEmbTdnnTaps;

__global__ __launch_bounds__(kEmbInit) void emb_tdnn_kernel(const float* __restrict__ head, const float* __restrict__ w, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ blk, int ldc,
                                                            const int* __restrict__ row_off, const int* __restrict__ t2_off) {
  __shared__ __attribute__((aligned(16))) float xs[kTdnnSpan * kEmbHeadOut];
  const int c = blockIdx.y, p0 = blockIdx.x * kTdnnTile;
  const int r0 = row_off[c], n = row_off[c + 1] - r0, q0 = t2_off[c], n2 = t2_off[c + 1] - q0;
  if (p0 >= n2) return;
  const int first = p0 * kEmbTdnnStride - kEmbTdnnTaps / 2;
  for (int idx = threadIdx.x; idx < kTdnnSpan * kEmbHeadOut; idx += kEmbInit) {
    const int i = idx / kEmbHeadOut, tt = first + i;
    xs[idx] = (tt >= 0 && tt < n) ? head[(size_t)(r0 + tt) * kEmbHeadOut + (idx - i * kEmbHeadOut)] : 0.0f;
  }
  __syncthreads();
  const int co = threadIdx.x;
  float a0[kTdnnTile], a1[kTdnnTile];
#pragma unroll
  for (int j = 0; j < kTdnnTile; ++j) a0[j] = a1[j] = 0.0f;
  for (int k = 0; k < kEmbTdnnTaps; ++k) {
    const float* wt = w + (size_t)k * kEmbHeadOut * kEmbInit + co;
    const float* xr = xs + k * kEmbHeadOut;
#pragma unroll 2
    for (int ci = 0; ci < kEmbHeadOut; ci += 4) {
      const float w0 = wt[ci * kEmbInit], w1 = wt[(ci + 1) * kEmbInit], w2 = wt[(ci + 2) * kEmbInit], w3 = wt[(ci + 3) * kEmbInit];
#pragma unroll
      for (int j = 0; j < kTdnnTile; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(xr + j * kEmbTdnnStride * kEmbHeadOut + ci);
        a0[j] = fmaf(v.x, w0, a0[j]);
        a1[j] = fmaf(v.y, w1, a1[j]);
        a0[j] = fmaf(v.z, w2, a0[j]);
        a1[j] = fmaf(v.w, w3, a1[j]);
      }
    }
  }
  const float sc = scale[co], sh = shift[co];
#pragma unroll
  for (int j = 0; j < kTdnnTile; ++j)
    if (p0 + j < n2) blk[(size_t)(q0 + p0 + j) * ldc + co] = fmaxf(fmaf(a0[j] + a1[j], sc, sh), 0.0f);
}

// ---- 1x1 convolutions on the matrix cores ---------------------------------------------------------------------------
constexpr int kGemmM = 64, kGemmN = 128, kGemmK = 32, kGemmFold = 2;      // a chain of kGemmFold * kGemmK = 64 terms, then the blocks in order

template <bool EPI>
__global__ __launch_bounds__(256) void emb_gemm_kernel(const float* __restrict__ A, int lda, int K, const float* __restrict__ in_s,
                                                       const float* __restrict__ in_h, const float* __restrict__ Bt, int N,
                                                       const float* __restrict__ out_s, const float* __restrict__ out_h, float* __restrict__ C,
                                                       int ldc, long M) {
  __shared__ float as[kGemmK][kGemmM + 1];      // [k][row]: the lanes of an operand load read consecutive rows
  __shared__ __attribute__((aligned(16))) float bs[kGemmK][kGemmN];
  const long m0 = (long)blockIdx.y * kGemmM;
  const int n0 = blockIdx.x * kGemmN;
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
    const float4 s4 = *reinterpret_cast<const float4*>(in_s + k0 + ak), h4 = *reinterpret_cast<const float4*>(in_h + k0 + ak);
    __syncthreads();      // the previous tile's operand reads are over
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const long m = m0 + ar + 32 * p;
      float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // rows behind the last: never stored
      if (m < M) {
        x = *reinterpret_cast<const float4*>(A + (size_t)m * lda + k0 + ak);
        x = make_float4(fmaxf(fmaf(x.x, s4.x, h4.x), 0.0f), fmaxf(fmaf(x.y, s4.y, h4.y), 0.0f), fmaxf(fmaf(x.z, s4.z, h4.z), 0.0f),
                        fmaxf(fmaf(x.w, s4.w, h4.w), 0.0f));
      }
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
  auto store = [&](const f32x16& tot, int col) {
    float sc = 1.0f, sh = 0.0f;
    if (EPI) { sc = out_s[col]; sh = out_h[col]; }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const long m = m0 + wm + (i & 3) + 8 * (i >> 2) + 4 * lk;
      float v = tot[i];
      if (EPI) v = fmaxf(fmaf(v, sc, sh), 0.0f);
      if (m < M) C[(size_t)m * ldc + col] = v;
    }
  };
  store(tot0, n0 + wn + li);
  store(tot1, n0 + wn + 32 + li);
}

// ---- context gates --------------------------------------------------------------------------------------------------
constexpr int kGateSlices = 4;

__global__ __launch_bounds__(kGateSlices * kEmbBn) void emb_gates_kernel(const float* __restrict__ h, const float* __restrict__ g1,
                                                                         const float* __restrict__ b1, const float* __restrict__ g2,
                                                                         const float* __restrict__ b2, float* __restrict__ segsum,
                                                                         float* __restrict__ gates, const int* __restrict__ t2_off,
                                                                         const int* __restrict__ seg_off) {
  __shared__ float part[kGateSlices][kEmbBn];
  __shared__ float ctx[kEmbBn];
  __shared__ float hid[kEmbGate];
  const int c = blockIdx.x, tid = threadIdx.x, s = tid / kEmbBn, ch = tid - s * kEmbBn;
  const int q0 = t2_off[c], n2 = t2_off[c + 1] - q0, sg0 = seg_off[c], n_seg = seg_off[c + 1] - sg0;
  float total = 0.0f;      // of the chunk, in the threads of slice 0
  for (int sg = 0; sg < n_seg; ++sg) {
    const int end = min(n2, (sg + 1) * kEmbSegLen);
    float a = 0.0f;
    for (int p = sg * kEmbSegLen + s; p < end; p += kGateSlices) a += h[(size_t)(q0 + p) * kEmbBn + ch];
    part[s][ch] = a;
    __syncthreads();
    if (s == 0) {
      const float v = (part[0][ch] + part[1][ch]) + (part[2][ch] + part[3][ch]);
      segsum[(size_t)(sg0 + sg) * kEmbBn + ch] = v;      // read back below by the thread that wrote it
      total += v;
    }
    __syncthreads();
  }
  for (int sg = 0; sg < n_seg; ++sg) {
    const int count = min(n2, (sg + 1) * kEmbSegLen) - sg * kEmbSegLen;
    if (s == 0) ctx[ch] = total / (float)n2 + segsum[(size_t)(sg0 + sg) * kEmbBn + ch] / (float)count;
    __syncthreads();
    if (tid < kEmbGate) {
      float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
      for (int k = 0; k < kEmbBn; k += 4)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = fmaf(ctx[k + i], g1[(k + i) * kEmbGate + tid], a[i]);
      hid[tid] = fmaxf(((a[0] + a[1]) + (a[2] + a[3])) + b1[tid], 0.0f);
    }
    __syncthreads();
    if (tid < kEmbGrowth) {
      float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
      for (int k = 0; k < kEmbGate; k += 4)
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = fmaf(hid[k + i], g2[(k + i) * kEmbGrowth + tid], a[i]);
      const float z = ((a[0] + a[1]) + (a[2] + a[3])) + b2[tid];
      gates[(size_t)(sg0 + sg) * kEmbGrowth + tid] = 1.0f / (1.0f + expf(-z));
    }
    __syncthreads();
  }
}

// ---- local convolution ----------------------------------------------------------------------------------------------
constexpr int kLocalTile = 16, kLocalPer = 2, kLocalMaxDil = 2;

__global__ __launch_bounds__(256) void emb_local_kernel(const float* __restrict__ h, const float* __restrict__ wl, const float* __restrict__ gates,
                                                        float* __restrict__ blk, int ldc, int c_at, int dil, const int* __restrict__ t2_off,
                                                        const int* __restrict__ seg_off) {
  __shared__ __attribute__((aligned(16))) float hs[(kLocalTile + 2 * kLocalMaxDil) * kEmbBn];
  const int c = blockIdx.y, p0 = blockIdx.x * kLocalTile;
  const int q0 = t2_off[c], n2 = t2_off[c + 1] - q0;
  if (p0 >= n2) return;
  const int span = kLocalTile + 2 * dil;
  for (int idx = threadIdx.x; idx < span * kEmbBn; idx += 256) {
    const int i = idx / kEmbBn, p = p0 - dil + i;
    hs[idx] = (p >= 0 && p < n2) ? h[(size_t)(q0 + p) * kEmbBn + (idx - i * kEmbBn)] : 0.0f;      // the zeros pad h: after its ReLU
  }
  __syncthreads();
  const int co = threadIdx.x & 31, g = threadIdx.x >> 5;
  float a0[kLocalPer], a1[kLocalPer];
#pragma unroll
  for (int j = 0; j < kLocalPer; ++j) a0[j] = a1[j] = 0.0f;
  for (int k = 0; k < 3; ++k) {
    const float* wt = wl + (size_t)k * kEmbBn * kEmbGrowth + co;
    const float* xr = hs + (g * kLocalPer + k * dil) * kEmbBn;
#pragma unroll 4
    for (int ci = 0; ci < kEmbBn; ci += 4) {
      const float w0 = wt[ci * kEmbGrowth], w1 = wt[(ci + 1) * kEmbGrowth], w2 = wt[(ci + 2) * kEmbGrowth], w3 = wt[(ci + 3) * kEmbGrowth];
#pragma unroll
      for (int j = 0; j < kLocalPer; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(xr + j * kEmbBn + ci);
        a0[j] = fmaf(v.x, w0, a0[j]);
        a1[j] = fmaf(v.y, w1, a1[j]);
        a0[j] = fmaf(v.z, w2, a0[j]);
        a1[j] = fmaf(v.w, w3, a1[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kLocalPer; ++j) {
    const int p = p0 + g * kLocalPer + j;
    if (p < n2) blk[(size_t)(q0 + p) * ldc + c_at + co] = (a0[j] + a1[j]) * gates[(size_t)(seg_off[c] + p / kEmbSegLen) * kEmbGrowth + co];
  }
}

// ---- pooling and the last dense layer -------------------------------------------------------------------------------
__global__ __launch_bounds__(kEmbXvec) void emb_pool_kernel(const float* __restrict__ xvec, float* __restrict__ stats, const int* __restrict__ t2_off) {
  const int c = blockIdx.x, ch = threadIdx.x;
  const int q0 = t2_off[c], n2 = t2_off[c + 1] - q0;
  const float* x = xvec + (size_t)q0 * kEmbXvec + ch;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int p = 0; p < n2; ++p) a[p & 3] += x[(size_t)p * kEmbXvec];
  const float mean = ((a[0] + a[1]) + (a[2] + a[3])) / (float)n2;
  a[0] = a[1] = a[2] = a[3] = 0.0f;
  for (int p = 0; p < n2; ++p) {
    const float d = x[(size_t)p * kEmbXvec] - mean;
    a[p & 3] = fmaf(d, d, a[p & 3]);
  }
  const float var = ((a[0] + a[1]) + (a[2] + a[3])) / (float)(n2 - 1);      // n2 >= 2: the entry points refuse fewer than 3 rows
  stats[(size_t)c * kEmbStats + ch] = mean;
  stats[(size_t)c * kEmbStats + kEmbXvec + ch] = sqrtf(var + kEmbPoolEps);
}

__global__ __launch_bounds__(256) void emb_dense_kernel(const float* __restrict__ stats, const float* __restrict__ w, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, int dim, float* __restrict__ emb) {
  __shared__ float st[kEmbStats];
  const int c = blockIdx.x;
  for (int k = threadIdx.x; k < kEmbStats; k += 256) st[k] = stats[(size_t)c * kEmbStats + k];
  __syncthreads();
  for (int d = threadIdx.x; d < dim; d += 256) {
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < kEmbStats; k += 4)
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = fmaf(st[k + i], w[(size_t)(k + i) * dim + d], a[i]);
    emb[(size_t)c * dim + d] = fmaf((a[0] + a[1]) + (a[2] + a[3]), scale[d], shift[d]);
  }
}

template <int CIN, int FIN, int KS, int FS>
hipError_t conv2d(const EmbConv& cv, const EmbTables& t, const float* in, const float* res, float* out, bool relu, bool transposed, hipStream_t st) {
  constexpr int FOUT = FIN / FS, NF = FOUT == 80 ? 10 : 5;
  hipLaunchKernelGGL((emb_conv2d_kernel<CIN, FIN, KS, FS>), dim3(t.max_rows, t.n_chunks), dim3(32, FOUT / NF), 0, st, in, cv.w, cv.scale, cv.shift,
                     res, out, t.row_off, relu ? 1 : 0, transposed ? 1 : 0);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_emb_head_conv(int idx, const EmbModel& m, const EmbTables& t, const float* d_in, const float* d_res, float* d_out, hipStream_t st) {
  if (t.n_chunks < 1 || t.max_rows < 1) return hipErrorInvalidValue;
  const EmbConv& cv = m.head[idx];
  switch (idx) {
    case 0: return conv2d<1, 80, 3, 1>(cv, t, d_in, nullptr, d_out, true, false, st);
    case 1: return conv2d<32, 80, 3, 2>(cv, t, d_in, nullptr, d_out, true, false, st);       // layer1.0.conv1
    case 3: return conv2d<32, 80, 1, 2>(cv, t, d_in, nullptr, d_out, false, false, st);      // layer1.0.shortcut
    case 2: case 5: return conv2d<32, 40, 3, 1>(cv, t, d_in, d_res, d_out, true, false, st); // layer1.{0,1}.conv2
    case 4: return conv2d<32, 40, 3, 1>(cv, t, d_in, nullptr, d_out, true, false, st);       // layer1.1.conv1
    case 6: return conv2d<32, 40, 3, 2>(cv, t, d_in, nullptr, d_out, true, false, st);       // layer2.0.conv1
    case 8: return conv2d<32, 40, 1, 2>(cv, t, d_in, nullptr, d_out, false, false, st);      // layer2.0.shortcut
    case 7: case 10: return conv2d<32, 20, 3, 1>(cv, t, d_in, d_res, d_out, true, false, st);
    case 9: return conv2d<32, 20, 3, 1>(cv, t, d_in, nullptr, d_out, true, false, st);
    case 11: return conv2d<32, 20, 3, 2>(cv, t, d_in, nullptr, d_out, true, true, st);       // head.conv2 -> [rows][320]
  }
  return hipErrorInvalidValue;
}

hipError_t launch_emb_tdnn(const EmbModel& m, const EmbTables& t, const float* d_head, float* d_blk, hipStream_t st) {
  if (t.n_chunks < 1 || t.max_t2 < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(emb_tdnn_kernel, dim3((t.max_t2 + kTdnnTile - 1) / kTdnnTile, t.n_chunks), dim3(kEmbInit), 0, st, d_head, m.tdnn.w, m.tdnn.scale,
                     m.tdnn.shift, d_blk, kEmbBlockWidth[0], t.row_off, t.t2_off);
  return hipGetLastError();
}

hipError_t launch_emb_gemm(const float* d_a, int lda, int K, const float* in_s, const float* in_h, const float* d_bt, int N, const float* out_s,
                           const float* out_h, float* d_c, int ldc, long M, hipStream_t st) {
  if (M < 1 || K < kGemmK || K % kGemmK != 0 || N % kGemmN != 0 || lda % 4 != 0 || lda < K || ldc < N) return hipErrorInvalidValue;
  const dim3 grid(N / kGemmN, (unsigned)((M + kGemmM - 1) / kGemmM));
  if (out_s)
    hipLaunchKernelGGL(emb_gemm_kernel<true>, grid, dim3(256), 0, st, d_a, lda, K, in_s, in_h, d_bt, N, out_s, out_h, d_c, ldc, M);
  else
    hipLaunchKernelGGL(emb_gemm_kernel<false>, grid, dim3(256), 0, st, d_a, lda, K, in_s, in_h, d_bt, N, out_s, out_h, d_c, ldc, M);
  return hipGetLastError();
}

hipError_t launch_emb_gates(const EmbDense& l, const EmbTables& t, const float* d_h, float* d_segsum, float* d_gates, hipStream_t st) {
  hipLaunchKernelGGL(emb_gates_kernel, dim3(t.n_chunks), dim3(kGateSlices * kEmbBn), 0, st, d_h, l.g1, l.b1, l.g2, l.b2, d_segsum, d_gates, t.t2_off,
                     t.seg_off);
  return hipGetLastError();
}

hipError_t launch_emb_local(const EmbDense& l, const EmbTables& t, const float* d_h, const float* d_gates, float* d_blk, int ldc, hipStream_t st) {
  if (l.dilation < 1 || l.dilation > kLocalMaxDil || l.c_in + kEmbGrowth > ldc) return hipErrorInvalidValue;
  hipLaunchKernelGGL(emb_local_kernel, dim3((t.max_t2 + kLocalTile - 1) / kLocalTile, t.n_chunks), dim3(256), 0, st, d_h, l.wl, d_gates, d_blk, ldc,
                     l.c_in, l.dilation, t.t2_off, t.seg_off);
  return hipGetLastError();
}

hipError_t launch_emb_pool(const EmbTables& t, const float* d_xvec, float* d_stats, hipStream_t st) {
  hipLaunchKernelGGL(emb_pool_kernel, dim3(t.n_chunks), dim3(kEmbXvec), 0, st, d_xvec, d_stats, t.t2_off);
  return hipGetLastError();
}

hipError_t launch_emb_dense(const EmbModel& m, const EmbTables& t, const float* d_stats, float* d_emb, hipStream_t st) {
  if (m.dim < 1 || m.dim > kEmbMaxDim) return hipErrorInvalidValue;
  hipLaunchKernelGGL(emb_dense_kernel, dim3(t.n_chunks), dim3(256), 0, st, d_stats, m.dense.w, m.dense.scale, m.dense.shift, m.dim, d_emb);
  return hipGetLastError();
}

}  // namespace diar
}  // namespace crispy

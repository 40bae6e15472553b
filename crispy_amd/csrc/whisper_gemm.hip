// whisper_gemm.hip -- the f32-activation products of the Whisper path and its LayerNorm (gfx950).
//
//   gemm_f32_nt_kernel      C[M,N] = A[M,K] . W[N,K]^T (+bias) (GELU) (+residual | +row-periodic table) on 128 x 128 tiles,
//                           f32 operands on v_mfma_f32_32x32x2_f32.  A may be a strided view (lda < K): both convolutions
//                           run as products over overlapping rows.  The f32 encoder (precision mode 0), the cross K|V
//                           projection (head-major store) and every product too tall or too odd for the skinny kernels.
//   gemm_skinny_f32_kernel  a decode step's projection over DENSE weights (f32, or an f16 copy: WH), <= 512 rows, one
//                           workgroup per 32 rows x 32 columns, K split over its waves; LayerNorm fold, GELU, residual and
//                           the split q | k|v output are compile-time forms.  The staged decode path (prompt steps, the
//                           f32 decoder, what the fused / matrix-vector paths do not take).
//   gemm_skinny_q_kernel    the same product over RESIDENT QUANTISED weights (ggml blocks de-quantised in registers):
//                           the staged decode path of crispy_asr_load_resident models.
//   layernorm_kernel        LayerNorm over the last dimension, one wave per row: the f32 encoder and the explicit
//                           LayerNorms of the decoder.
//
// The two skinny kernels share their decomposition and their epilogue -- defined ONCE below (the SK_* macros); what
// each kernel spells out itself is how its W operand reaches the matrix instruction.  A clip decodes to the same bits alone
// and in any batch, and a resident model to the same bits as its de-quantised copy, because these pieces are the same text.
// Host side (end of file): one description of a skinny product (skinny_form) and one dispatch from it to a kernel form.
#include <algorithm>
#include <atomic>
#include "asr_common.h"
#include "asr_quant.h"
#include "wave_ops.h"

namespace crispy {
namespace {

constexpr int GB_M = 128, GB_N = 128, GB_K = 16, GB_LD = 20;  // LDS row stride 20 floats: conflict-free b128 reads

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void gemm_f32_nt_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float As[2][GB_M * GB_LD];
  __shared__ __attribute__((aligned(16))) float Ws[2][GB_N * GB_LD];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int bz = blockIdx.z;
  const float* __restrict__ A = g.A + (long)bz * g.strideA;
  const float* __restrict__ W = g.W;
  float* __restrict__ C = g.C + (long)bz * g.strideC + (g.c_off_dev ? (long)(*g.c_off_dev) * g.c_off_scale : 0L);
  const int m0 = blockIdx.y * GB_M, n0 = blockIdx.x * GB_N;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  // staging: thread loads float4 #q of row (tid>>2) + 64*h, k-offset 4*(tid&3)
  const int lr = tid >> 2, lk = (tid & 3) * 4;
  float4 ra[2], rw[2];
  auto load_tiles = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int m = m0 + lr + 64 * h, n = n0 + lr + 64 * h;
      ra[h] = (m < g.M) ? *reinterpret_cast<const float4*>(A + (long)m * g.lda + k0 + lk) : make_float4(0, 0, 0, 0);
      rw[h] = (n < g.N) ? *reinterpret_cast<const float4*>(W + (long)n * g.ldw + k0 + lk) : make_float4(0, 0, 0, 0);
    }
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<float4*>(&As[buf][(lr + 64 * h) * GB_LD + lk]) = ra[h];
      *reinterpret_cast<float4*>(&Ws[buf][(lr + 64 * h) * GB_LD + lk]) = rw[h];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = g.K / GB_K;
  load_tiles(0);
  store_tiles(0);
  __syncthreads();
  const int li = lane & 31, lh = lane >> 5;
  for (int kb = 0; kb < nk; ++kb) {
    const int buf = kb & 1;
    if (kb + 1 < nk) load_tiles((kb + 1) * GB_K);
    // operands: MFMA step s contracts the k-pair (s, s+8) of this 16-wide block; lane half lh owns k = 8*lh + s
    float a[2][8], w[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4* pa = reinterpret_cast<const float4*>(&As[buf][(wm + 32 * i + li) * GB_LD + 8 * lh]);
      const float4* pw = reinterpret_cast<const float4*>(&Ws[buf][(wn + 32 * i + li) * GB_LD + 8 * lh]);
      const float4 a0 = pa[0], a1 = pa[1], w0 = pw[0], w1 = pw[1];
      a[i][0] = a0.x; a[i][1] = a0.y; a[i][2] = a0.z; a[i][3] = a0.w;
      a[i][4] = a1.x; a[i][5] = a1.y; a[i][6] = a1.z; a[i][7] = a1.w;
      w[i][0] = w0.x; w[i][1] = w0.y; w[i][2] = w0.z; w[i][3] = w0.w;
      w[i][4] = w1.x; w[i][5] = w1.y; w[i][6] = w1.z; w[i][7] = w1.w;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s], w[j][s], acc[i][j], 0, 0, 0);
    if (kb + 1 < nk) store_tiles(buf ^ 1);
    __syncthreads();
  }

  // epilogue.  The residual / row-table operands of a lane's 16 rows are requested together from clamped (always
  // valid) addresses before any of them is used: one exposed round trip per 32 x 32 block instead of one per element
  // (with a load, a wait and a store per row the short-K projections of the encoder spent their tail waiting on L2).
  const bool hm = g.hm_rows > 0;              // head-major store (cross K|V): see GemmArgs
  int hm_b0 = 0, hm_t0 = 0;
  if (hm) { hm_b0 = m0 / g.hm_rows; hm_t0 = m0 - hm_b0 * g.hm_rows; }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + 32 * j + li;
      const int nc = min(n, g.N - 1);
      const float bias = g.bias ? g.bias[nc] : 0.f;
      long hm_col = 0;
      if (hm) {
        const int kv = nc >= g.hm_width ? 1 : 0, rem = nc - kv * g.hm_width;
        hm_col = ((long)kv * g.hm_width + (long)(rem >> 6) * 64) * g.hm_rows + (rem & 63);
      }
#pragma unroll
      for (int r0 = 0; r0 < 16; r0 += 8) {     // eight rows at a time: enough loads in flight, 3 waves per SIMD kept
        float extra[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) extra[r] = 0.f;
        if (g.residual) {
          const float* rp = g.residual + (long)bz * g.strideR + nc;
#pragma unroll
          for (int r = 0; r < 8; ++r)
            extra[r] = rp[(long)min(m0 + wm + 32 * i + acc_row(r0 + r, lane), g.M - 1) * g.ldr];
        }
        if (g.rowtab) {
#pragma unroll
          for (int r = 0; r < 8; ++r)
            extra[r] += g.rowtab[(long)(min(m0 + wm + 32 * i + acc_row(r0 + r, lane), g.M - 1) % g.rowtab_period) * g.N + nc];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int dm = wm + 32 * i + acc_row(r0 + r, lane);
          const int m = m0 + dm;
          float v = acc[i][j][r0 + r] + bias;
          if (g.gelu) v = g.gelu == 2 ? gelu_ggml(v) : gelu_erf(v);
          v += extra[r];
          if (m >= g.M || n >= g.N) continue;
          if (hm) {
            int t = hm_t0 + dm, b = hm_b0;      // a 128-row tile crosses at most one clip boundary where hm_rows >= 128 ...
            if (g.hm_rows < GB_M) { b = m / g.hm_rows; t = m - b * g.hm_rows; }      // ... and several below (a reduced audio context)
            else if (t >= g.hm_rows) { t -= g.hm_rows; ++b; }
            C[(long)b * g.N * g.hm_rows + (long)t * 64 + hm_col] = v;
          } else {
            C[(long)m * g.ldc + n] = v;
          }
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------
// Skinny GEMM for the decoder (M = clips of one decode step): latency-, not FLOP-bound.
// One workgroup per 32 clips x 32 output columns; the 4 waves split K four ways and feed the MFMA straight from
// global memory (both operands are K-contiguous rows, so a lane's operands are 16 contiguous floats per
// 32-wide K chunk: step s contracts k = s and k = s + 16); partial tiles are summed through LDS.
// No LDS staging, no barriers in the K loop.  The kernel is a chain of memory latencies, not of MFMAs (48 per wave
// at K = 384): three K chunks of operands are requested before the first MFMA, so Whisper-tiny's K = 384
// projections expose one round trip instead of three, and 32-row blocks put twice the workgroups on the chip
// (24 for N = 384).  W is re-read per row block from L2.
// ---------------------------------------------------------------------------------------------
constexpr int SK_PF = 3;                       // K chunks (32 wide) in flight per wave
constexpr int SK_WAVE_LDS = 2048;              // floats of LDS per wave (two 4 KB operand chunks; later the 32 x 33 partial tile)
// LN / GELU / RES are compile-time so that the epilogue operands (ln_s, ln_c or bias, residual) can be requested
// up front, next to the first K chunks, from clamped (always valid) addresses: with run-time flags every one of them
// sat behind its own branch in the epilogue and cost a serialized L2 round trip after the barrier.
// NW = waves of a workgroup = ways K is split.  4 for the K = d projections; 16 for the MLP's second GEMM (K = 4 d):
// with 4 waves that one ran four rounds of the memory latency on 24 workgroups (19.5 us at Whisper-tiny, three times
// the other projections), with 16 it runs one like the rest.
// WH: W is an f16 matrix (g.W reinterpreted, g.ldw in halves) and the products run on v_mfma_f32_32x32x16_f16 with
// the A operand rounded to f16 on the way in -- ggml's arithmetic for a plain mul_mat (precision mode 1: the attention
// output projections and the MLP's second GEMM, where no LayerNorm is folded in).  In f32 a 32 x 32 x 1536 tile is
// 768 MFMAs of 64 cycles on ONE CU: 5 us of matrix-pipe time for the K = 4 d projection at Whisper-tiny, whatever the
// number of clips; in f16 it is 96 MFMAs of 32 cycles.  Same loads for A, same epilogue; W arrives as two 16-byte
// pieces per lane and chunk (4 lanes per 64-byte row piece, slot = piece ^ ((row >> 2) & 3): see gemm_hd_kernel).
//
// ---- what gemm_skinny_f32_kernel and gemm_skinny_q_kernel share, each piece written once ----
// Macros in the idiom of SK_REQUEST / SK_CHUNK, not functions: the rule for this file is that a kernel's listing does not
// change when its text is shared, and the function forms tried (the epilogue, the MFMA steps) changed it; so did moving a
// statement of the set-up relative to the kernels' own (NOTEBOOK 18) -- hence three pieces of set-up, each where the
// kernels had it.  They use the kernels' template arguments (LN, GELU, RES, NW) and the argument g by name.
//
// SK_SETUP: the decomposition.  Per wave 8 KB of LDS: the transposition area of its operand chunks (32 rows x 8
// sixteen-byte pieces each); the wave's partial tile replaces it after the K loop.
// Global loads of A are row-coalesced: 8 lanes take the 8 sixteen-byte pieces of one row's 32-wide K chunk (one 128-byte
// line), an instruction covers 8 rows, four cover the chunk.  (Loading in MFMA operand order -- lane = row, 16
// contiguous floats -- made every instruction touch 64 lines for 16 bytes each and the texture addresser, not the
// memory latency, set the pace: 19.5 us for K = 1536 on 24 workgroups.)  The chunk goes through the wave's LDS area
// to reach operand order; piece c of row r sits in slot c ^ (r & 7), so both the linear writes and the
// row-per-lane 16-byte reads are conflict-free.  Operand registers, MFMA order and results are those of the
// direct-load form.  Sources are wave-uniform bases (scalar registers) + 32-bit byte offsets per lane: eight address
// registers instead of sixteen, which is what lets the 16-wave form keep three chunks in flight inside its 128 registers.
#define SK_SETUP                                                                                                   \
  extern __shared__ __attribute__((aligned(16))) float sk_smem[];                                                  \
  float (*red)[SK_WAVE_LDS] = reinterpret_cast<float (*)[SK_WAVE_LDS]>(sk_smem);                                   \
  float (*rstat)[32][2] = reinterpret_cast<float (*)[32][2]>(sk_smem + NW * SK_WAVE_LDS);                          \
  constexpr int ET = NW >= 16 ? 1024 : NW >= 8 ? 512 : 256; /* threads that finish outputs (12 waves: the first 512) */ \
  constexpr int RP = ET / 32, NQ = 32 / RP;                 /* epilogue: RP rows per pass, NQ passes */              \
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;                   \
  const int li = lane & 31, lh = lane >> 5;                                                                        \
  const int n0 = blockIdx.x * 32;                                                                                  \
  const int mb = blockIdx.y * 32;                           /* row block of 32 clips */                            \
  const float* __restrict__ A = g.A;                                                                               \
  const bool second = g.C2 && n0 >= g.n_split;              /* split output: a workgroup's 32 columns go to one destination */ \
  const int kper = g.K / NW;                                /* K range of this wave (multiple of 32) */             \
  const int kbeg = wave * kper;                                                                                    \
  const int lr = lane >> 3, lc = (lane & 7) ^ lr;
// the byte offset of this lane's piece of A row j (of four) in a chunk; rows >= M: clamped row, never stored
#define SK_A_SOURCE(j) (unsigned)(((long)min(mb + lr + 8 * (j), g.M - 1) * g.lda + 4 * lc) * 4)
// SK_ACCUMULATOR: where the lane's operand pieces come back from in the wave's area, and what they are summed into
#define SK_ACCUMULATOR                                                                                             \
  int rslot[4];                                             /* slots of this lane's operand pieces 4 lh + q of row li */ \
  _Pragma("unroll") for (int q = 0; q < 4; ++q) rslot[q] = li * 8 + ((4 * lh + q) ^ (li & 7));                     \
  f32x16 acc;                                                                                                      \
  _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[r] = 0.f;                                                     \
  float s0 = 0.f, q0 = 0.f;                                 /* row sum / sum of squares of this lane's share (LN folding) */
// SK_EPILOGUE_OPERANDS: the epilogue operands of this thread's outputs -- column ec of rows (tid >> 5) + 8 q -- and the
// lambda that requests them, from clamped (always valid) addresses.  When it is called is each kernel's own business.
#define SK_EPILOGUE_OPERANDS                                                                                       \
  const int ec = min(tid & 31, g.N - 1 - n0), enn = n0 + ec;                                                       \
  float e_s = 0.f, e_c = 0.f, e_res[NQ];                                                                           \
  auto request_epilogue = [&]() {                                                                                  \
    if (LN) { e_s = g.ln_s[enn]; e_c = g.ln_c[enn]; }                                                              \
    else if (g.bias) e_c = g.bias[enn];                                                                            \
    if (RES) {                                                                                                     \
      _Pragma("unroll") for (int q = 0; q < NQ; ++q)                                                               \
        e_res[q] = g.residual[(long)min(mb + min((tid >> 5) + RP * q, 31), g.M - 1) * g.ldr + enn];                \
    }                                                                                                              \
  };
// SK_DESTINATION: where this workgroup's 32 columns go (C, or C2 behind n_split; the KV-cache slot offset of the device)
#define SK_DESTINATION                                                                                             \
  const long coff = g.c_off_dev ? (long)(*g.c_off_dev) * g.c_off_scale : 0L;                                       \
  float* __restrict__ C = second ? g.C2 + coff - g.n_split : g.C + (g.C2 ? 0L : coff);                             \
  const long ldc = second ? g.ldc2 : g.ldc;
// SK_REDUCE_AND_STORE: the waves' partial tiles (and LayerNorm sums) through LDS, summed in the fixed order wave 0, 1, ...;
// LayerNorm fold, bias, GELU, residual; the store.  Only the stores are predicated.
#define SK_REDUCE_AND_STORE                                                                                        \
  _Pragma("unroll") for (int r = 0; r < 16; ++r) red[wave][acc_row(r, lane) * 33 + li] = acc[r]; /* own area: after the wave's last reads */ \
  if (LN) {                                                                                                        \
    /* the two half-waves hold the two 16-wide halves of every 32-wide K chunk of row li */                        \
    s0 += __shfl_xor(s0, 32, 64); q0 += __shfl_xor(q0, 32, 64);                                                    \
    if (lh == 0) { rstat[wave][li][0] = s0; rstat[wave][li][1] = q0; }                                             \
  }                                                                                                                \
  __syncthreads();                                                                                                 \
  _Pragma("unroll") for (int q = 0; q < NQ; ++q) {                                                                 \
    const int ml = min((tid >> 5) + RP * q, 31);   /* row inside this 32-row block (threads >= ET: clamped, not stored) */ \
    const int m = mb + ml;                                                                                         \
    float v = red[0][ml * 33 + ec];                                                                                \
    _Pragma("unroll") for (int w2 = 1; w2 < NW; ++w2) v += red[w2][ml * 33 + ec];                                  \
    if (LN) {                                                                                                      \
      float sum = rstat[0][ml][0], sq = rstat[0][ml][1];                                                           \
      _Pragma("unroll") for (int w2 = 1; w2 < NW; ++w2) { sum += rstat[w2][ml][0]; sq += rstat[w2][ml][1]; }       \
      const float mean = sum / (float)g.K;                                                                         \
      const float var = fmaxf(sq / (float)g.K - mean * mean, 0.f);                                                 \
      const float rstd = 1.f / sqrtf(var + 1e-5f);                                                                 \
      v = rstd * (v - mean * e_s) + e_c;                                                                           \
    } else {                                                                                                       \
      v += e_c;                                                                                                    \
    }                                                                                                              \
    if (GELU) v = g.gelu == 2 ? gelu_ggml(v) : gelu_erf(v);                                                        \
    if (RES) v += e_res[q];                                                                                        \
    if (tid < ET && m < g.M && n0 + (tid & 31) < g.N) {                                                            \
      if (second && g.c2_half) (reinterpret_cast<_Float16*>(g.C2) + coff - g.n_split)[(long)m * ldc + enn] = (_Float16)v; \
      else C[(long)m * ldc + enn] = v;                                                                             \
    }                                                                                                              \
  }
// SK_MFMA_F16: f16 step ST of a chunk -- the A pieces 2 ST, 2 ST + 1 (k = 16 lh + 8 st + e for both operands) rounded to
// f16 on the way in, against the eight halves WV.
#define SK_MFMA_F16(ST, WV)                                                                                        \
  {                                                                                                                \
    const half8 av = {(_Float16)ca[2 * (ST)].x, (_Float16)ca[2 * (ST)].y, (_Float16)ca[2 * (ST)].z, (_Float16)ca[2 * (ST)].w,    \
                         (_Float16)ca[2 * (ST) + 1].x, (_Float16)ca[2 * (ST) + 1].y, (_Float16)ca[2 * (ST) + 1].z, (_Float16)ca[2 * (ST) + 1].w}; \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, WV, acc, 0, 0, 0);                                            \
  }
// SK_MFMA_F32: the four f32 steps of A piece Q against the weights WE (an expression in e), with the LayerNorm sums of A.
#define SK_MFMA_F32(Q, WE)                                                                                         \
  {                                                                                                                \
    const float xv[4] = {ca[Q].x, ca[Q].y, ca[Q].z, ca[Q].w};                                                      \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                \
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[e], WE, acc, 0, 0, 0);                                         \
      if (LN) { s0 += xv[e]; q0 = fmaf(xv[e], xv[e], q0); }                                                        \
    }                                                                                                              \
  }

template <bool LN, bool GELU, bool RES, int NW, bool WH = false>
__global__ __launch_bounds__(64 * NW) void gemm_skinny_f32_kernel(GemmArgs g) {
  static_assert(!(WH && LN), "the f16-weight form has no LayerNorm fold");
  constexpr int PF = NW > 12 ? 2 : SK_PF;            // 16 waves: 128 registers per lane, two chunks in flight (three spill 35 - 67 registers even with scalar bases)
  SK_SETUP
  // W: f32 rows loaded like A's; f16 rows (WH) as two pieces per lane: j < 2: row 16 j + (lane >> 2), the 16-byte piece
  // that belongs into slot lane & 3
  const float* __restrict__ W = g.W;
  const char* __restrict__ Wb = WH ? reinterpret_cast<const char*>(reinterpret_cast<const _Float16*>(W) + kbeg)
                                   : reinterpret_cast<const char*>(W + kbeg);
  const char* __restrict__ Ab = reinterpret_cast<const char*>(A + kbeg);
  unsigned wsrc[4], asrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (WH) {
      const int r = 16 * (j & 1) + (lane >> 2);
      wsrc[j] = (unsigned)(((long)min(n0 + r, g.N - 1) * g.ldw + 8 * ((lane & 3) ^ ((r >> 2) & 3))) * 2);
    } else {
      wsrc[j] = (unsigned)(((long)min(n0 + lr + 8 * j, g.N - 1) * g.ldw + 4 * lc) * 4);
    }
    asrc[j] = SK_A_SOURCE(j);
  }
  f32x4* stw = reinterpret_cast<f32x4*>(sk_smem + wave * SK_WAVE_LDS);     // the wave's area: W pieces, then A pieces
  f32x4* sta = stw + 256;
  SK_ACCUMULATOR
  // the chunks in flight.  They are clang vectors, not HIP's float4: copies of the float4 struct between these
  // arrays and LDS kept all six arrays in scratch (400 bytes per lane), whatever the loop structure
  f32x4 w0[4], a0[4], w1[4], a1[4], w2[4], a2[4];
#define SK_REQUEST(WR, AR, KO)                                            \
  _Pragma("unroll") for (int j = 0; j < 4; ++j) {                         \
    if (!WH || j < 2) WR[j] = *reinterpret_cast<const f32x4*>(Wb + (size_t)wsrc[j] + (WH ? 2 : 4) * (KO)); \
    AR[j] = *reinterpret_cast<const f32x4*>(Ab + (size_t)asrc[j] + 4 * (KO)); \
  }
  SK_REQUEST(w0, a0, 0)
  if (PF > 1 && 32 < kper) { SK_REQUEST(w1, a1, 32) }
  if (PF > 2 && 64 < kper) { SK_REQUEST(w2, a2, 64) }
  SK_EPILOGUE_OPERANDS
  // The LayerNorm-fold forms with 12 / 16 waves (128 / 168 registers per lane) have no room to keep these three to six
  // values across the K loop: the compiler parked them in scratch (a store behind a vmcnt wait in the prologue, a
  // reload -- one more memory round trip -- after the loop).  Those forms request them AFTER the loop instead, under
  // the LDS hand-off and the barrier: the same round trip, no scratch (tests/test_build_resources.py).
  constexpr bool LATE_EPI = LN && (NW >= 16 || (NW >= 12 && RES));
  if (!LATE_EPI) request_epilogue();
  SK_DESTINATION
  // one chunk: registers -> LDS, request the chunk PF ahead into the same registers, LDS -> operand order, 16 MFMAs
#define SK_CHUNK(WR, AR, KC)                                                                        \
  {                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) { if (!WH || j < 2) stw[64 * j + lane] = WR[j]; sta[64 * j + lane] = AR[j]; } \
    if ((KC) + 32 * PF < kper) { SK_REQUEST(WR, AR, (KC) + 32 * PF) }                               \
    wave_lds_sync();                                                                                \
    f32x4 cw[4], ca[4];                                                                            \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) { if (!WH) cw[q] = stw[rslot[q]]; ca[q] = sta[rslot[q]]; } \
    if (WH) { cw[0] = stw[li * 4 + ((2 * lh) ^ ((li >> 2) & 3))]; cw[1] = stw[li * 4 + ((2 * lh + 1) ^ ((li >> 2) & 3))]; } \
    wave_lds_sync();                                                                                \
    if (WH) {                                                                                       \
      _Pragma("unroll") for (int st = 0; st < 2; ++st) SK_MFMA_F16(st, __builtin_bit_cast(half8, cw[st]))        \
    } else {                                                                                        \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                               \
        const float wv[4] = {cw[q].x, cw[q].y, cw[q].z, cw[q].w};                                   \
        SK_MFMA_F32(q, wv[e])                                                                       \
      }                                                                                             \
    }                                                                                               \
  }
  for (int kc0 = 0; kc0 < kper; kc0 += 32 * PF) {
    SK_CHUNK(w0, a0, kc0)
    if (PF > 1 && kc0 + 32 < kper) SK_CHUNK(w1, a1, kc0 + 32)
    if (PF > 2 && kc0 + 64 < kper) SK_CHUNK(w2, a2, kc0 + 64)
  }
#undef SK_CHUNK
#undef SK_REQUEST
  if (LATE_EPI) request_epilogue();
  SK_REDUCE_AND_STORE
}

// ---------------------------------------------------------------------------------------------
// The skinny kernel over RESIDENT QUANTISED weights (crispy_asr_load_resident; asr_quant.h).  Same decomposition, same
// A path (row-coalesced loads, transposed through the wave's LDS area), same MFMA order, same epilogue -- the W operand
// is different: a 32-wide K chunk of one output row is exactly ONE ggml block, and the 16 k values lane (row li, half
// lh) contracts are the block's low (lh = 0) or high (lh = 1) nibbles, so every lane fetches its row's block (5 - 6
// dwords, 18 - 24 bytes; two lanes share a block) straight into registers and de-quantises its 16 values there:
// no LDS round trip for W, 0.56 - 1.06 bytes per weight from HBM instead of 2 or 4, and no separate de-quantisation
// launch.  Values are computed with the loader's operations in the loader's order (int -> float, one multiply, one add,
// times gamma[k] for the LayerNorm-folded form -- fold_ln's W' = W . diag(gamma) -- each rounded on its own; then
// rounded to f16 for the WH form), so results equal those of the dense kernels on the de-quantised weights bit for bit.
// ---------------------------------------------------------------------------------------------
template <int TT> struct QFetch {
  static constexpr int NWD = TT == QT_Q8_0 ? 5 : (quant_block_bytes(TT) + 3) / 4;
  unsigned w[NWD];
};
template <int TT>
__device__ __forceinline__ void q_fetch(QFetch<TT>& f, const unsigned char* b, int lh) {
  if (TT == QT_Q8_0) {
    unsigned short dv;
    __builtin_memcpy(&dv, b, 2);
    f.w[0] = dv;
#pragma unroll
    for (int i = 0; i < 4; ++i) f.w[1 + i] = q_u32(b + 2 + 16 * lh + 4 * i);
  } else {
#pragma unroll
    for (int i = 0; i < QFetch<TT>::NWD; ++i) f.w[i] = q_u32(b + 4 * i);      // (the last dword may reach 2 bytes past the block)
  }
}
__device__ __forceinline__ float q_half_bits(unsigned v) {
  const unsigned short u = (unsigned short)(v & 0xffffu);
  _Float16 h;
  __builtin_memcpy(&h, &u, 2);
  return (float)h;
}
// y[s] = weight 16 lh + s of the fetched block, s < 16
template <int TT>
__device__ __forceinline__ void q_half_block(const QFetch<TT>& f, int lh, float (&y)[16]) {
#pragma clang fp contract(off)
  const float d = q_half_bits(f.w[0]);
  if (TT == QT_Q8_0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) y[4 * i + e] = (float)(int)(signed char)((f.w[1 + i] >> (8 * e)) & 0xff) * d;
    return;
  }
  constexpr bool has_m = TT == QT_Q4_1 || TT == QT_Q5_1, has_h = TT == QT_Q5_0 || TT == QT_Q5_1;
  const float m = has_m ? q_half_bits(f.w[0] >> 16) : 0.f;
  unsigned qh = 0u, qs[4];
  if (TT == QT_Q4_0) {          // {d}{qs 16} from byte 2
#pragma unroll
    for (int i = 0; i < 4; ++i) qs[i] = (f.w[i] >> 16) | (f.w[i + 1] << 16);
  } else if (TT == QT_Q4_1) {   // {d, m}{qs} from byte 4
#pragma unroll
    for (int i = 0; i < 4; ++i) qs[i] = f.w[1 + i];
  } else if (TT == QT_Q5_0) {   // {d}{qh 4}{qs} : qh at byte 2, qs at byte 6
    qh = (f.w[0] >> 16) | (f.w[1] << 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) qs[i] = (f.w[1 + i] >> 16) | (f.w[2 + i] << 16);
  } else {                      // q5_1 {d, m}{qh}{qs}
    qh = f.w[1];
#pragma unroll
    for (int i = 0; i < 4; ++i) qs[i] = f.w[2 + i];
  }
  const int sh = 4 * lh;
  const unsigned hb = has_h ? (qh >> (16 * lh)) : 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = 4 * i + e;
      int x = (int)((qs[i] >> (8 * e + sh)) & 0x0fu);
      if (has_h) x |= (int)((hb >> j) & 1u) << 4;
      if (TT == QT_Q4_0) y[j] = (float)(x - 8) * d;
      else if (TT == QT_Q5_0) y[j] = (float)(x - 16) * d;
      else y[j] = (float)x * d + m;
    }
}

template <int TT, bool LN, bool GELU, bool RES, int NW, bool WH>
__global__ __launch_bounds__(64 * NW) void gemm_skinny_q_kernel(GemmArgs g) {
  static_assert(!(WH && LN), "the f16 form has no LayerNorm fold");
  // chunks in flight: A 16 + block 6 (+ gamma 16) registers each; the LayerNorm-folded form with 16 waves has 128 registers
  // per lane and keeps one (its K is 512 or 1024: one or two chunks per wave) -- two spilled 72 - 104 bytes
  constexpr int PF = (LN && NW >= 16) ? 1 : 2;
  constexpr int BB = quant_block_bytes(TT);
  SK_SETUP
  const char* __restrict__ Ab = reinterpret_cast<const char*>(A + kbeg);
  unsigned asrc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) asrc[j] = SK_A_SOURCE(j);
  // this lane's weight row: part p of the row-fused matrix, local row r -> its blocks are contiguous
  const unsigned char* __restrict__ wrow;
  {
    const int row = min(n0 + li, g.N - 1);
    const int p = row / g.wq_rows;
    const unsigned char* base = p == 0 ? g.wq[0] : (p == 1 ? g.wq[1] : g.wq[2]);
    wrow = base + ((long)(row - p * g.wq_rows) * (g.K / 32) + kbeg / 32) * BB;
  }
  const float* __restrict__ gam = LN ? g.wq_gamma + kbeg + 16 * lh : nullptr;
  f32x4* sta = reinterpret_cast<f32x4*>(sk_smem + wave * SK_WAVE_LDS) + 256;     // the A half of the wave's area: W never goes through LDS
  SK_ACCUMULATOR
  f32x4 a0[4], a1[4], g0[4], g1[4];
  QFetch<TT> b0, b1;
#define SKQ_REQUEST(BR, AR, GR, KO)                                                     \
  {                                                                                     \
    q_fetch<TT>(BR, wrow + (long)((KO) / 32) * BB, lh);                                \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                     \
      AR[j] = *reinterpret_cast<const f32x4*>(Ab + (size_t)asrc[j] + 4 * (KO));         \
      if (LN) GR[j] = *reinterpret_cast<const f32x4*>(gam + (KO) + 4 * j);              \
    }                                                                                   \
  }
  SKQ_REQUEST(b0, a0, g0, 0)
  if (PF > 1 && 32 < kper) SKQ_REQUEST(b1, a1, g1, 32)
  SK_EPILOGUE_OPERANDS
  SK_DESTINATION
#define SKQ_CHUNK(BR, AR, GR, KC)                                                                   \
  {                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) sta[64 * j + lane] = AR[j];                       \
    float wy[16];                                                                                   \
    q_half_block<TT>(BR, lh, wy);                                                                   \
    if (LN) {                                                                                       \
      _Pragma("clang fp contract(off)")                                                             \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                               \
        wy[4 * j] = wy[4 * j] * GR[j].x; wy[4 * j + 1] = wy[4 * j + 1] * GR[j].y;                   \
        wy[4 * j + 2] = wy[4 * j + 2] * GR[j].z; wy[4 * j + 3] = wy[4 * j + 3] * GR[j].w;           \
      }                                                                                             \
    }                                                                                               \
    if ((KC) + 32 * PF < kper) SKQ_REQUEST(BR, AR, GR, (KC) + 32 * PF)                              \
    wave_lds_sync();                                                                                \
    f32x4 ca[4];                                                                                    \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) ca[q] = sta[rslot[q]];                            \
    wave_lds_sync();                                                                                \
    if (WH) {                                                                                       \
      _Pragma("unroll") for (int st = 0; st < 2; ++st)                                              \
        SK_MFMA_F16(st, (half8{(_Float16)wy[8 * st], (_Float16)wy[8 * st + 1], (_Float16)wy[8 * st + 2], (_Float16)wy[8 * st + 3],    \
                                  (_Float16)wy[8 * st + 4], (_Float16)wy[8 * st + 5], (_Float16)wy[8 * st + 6], (_Float16)wy[8 * st + 7]})) \
    } else {                                                                                        \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) SK_MFMA_F32(q, wy[4 * q + e])                   \
    }                                                                                               \
  }
  for (int kc0 = 0; kc0 < kper; kc0 += 32 * PF) {
    SKQ_CHUNK(b0, a0, g0, kc0)
    if (PF > 1 && kc0 + 32 < kper) SKQ_CHUNK(b1, a1, g1, kc0 + 32)
  }
#undef SKQ_CHUNK
#undef SKQ_REQUEST
  request_epilogue();             // every form requests them behind the K loop (the dense kernel: its LATE_EPI forms)
  SK_REDUCE_AND_STORE
}
#undef SK_SETUP
#undef SK_A_SOURCE
#undef SK_ACCUMULATOR
#undef SK_EPILOGUE_OPERANDS
#undef SK_DESTINATION
#undef SK_REDUCE_AND_STORE
#undef SK_MFMA_F16
#undef SK_MFMA_F32

// ---------------------------------------------------------------------------------------------
// LayerNorm over the last dimension (eps 1e-5), one wave per row; D <= 1280, multiple of 64
// ---------------------------------------------------------------------------------------------
template <int PER>     // PER = D / 64 columns per lane: compile-time, so the row is requested in one go (no branch per load)
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y,
                                                        long rows) {
  constexpr int D = 64 * PER;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* xr = x + row * D;
  float v[PER], gm[PER], bt[PER];
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < PER; ++q) v[q] = xr[lane + 64 * q];
#pragma unroll
  for (int q = 0; q < PER; ++q) { gm[q] = gamma[lane + 64 * q]; bt[q] = beta[lane + 64 * q]; }
#pragma unroll
  for (int q = 0; q < PER; ++q) s += v[q];
  s = shfl_sum(s);
  const float mean = s / (float)D;
  float s2 = 0.f;
#pragma unroll
  for (int q = 0; q < PER; ++q) { const float d = v[q] - mean; s2 = fmaf(d, d, s2); }
  s2 = shfl_sum(s2);
  const float rstd = 1.f / sqrtf(s2 / (float)D + 1e-5f);
  float* yr = y + row * D;
#pragma unroll
  for (int q = 0; q < PER; ++q) yr[lane + 64 * q] = (v[q] - mean) * rstd * gm[q] + bt[q];
}

// ---------------------------------------------------------------------------------------------
// Host side of the skinny kernels: one description of a product, one way from it to a kernel form.
// ---------------------------------------------------------------------------------------------
// The forms that are built.  kind = LayerNorm fold 4 | GELU 2 | residual 1.
//   dense f32 weights            every kind
//   f16 operands (g.w_half)      residual, bias only, bias + GELU -- over a dense f16 copy and over quantised blocks alike:
//                                the residual projections (attention outputs, MLP second product; precision mode 1), and
//                                behind an explicit LayerNorm (f16 LayerNorm outputs) bias only and bias + GELU
//   quantised blocks, f32        LayerNorm fold (q | k | v, cross q), LayerNorm fold + GELU (MLP first product)
constexpr bool sk_form_exists(int kind, bool wh, bool quant) { return wh ? kind <= 2 : quant ? (kind == 4 || kind == 6) : true; }

struct SkinnyForm {
  bool skinny;      // the product takes the skinny path
  int nw;           // ways K is split = waves of a workgroup
  int kind;
  bool wh;
  bool exists(bool quant) const { return sk_form_exists(kind, wh, quant); }      // over dense (f32, or f16 when wh) / quantised weights
};
SkinnyForm skinny_form(const GemmArgs& g, int batch) {
  SkinnyForm f;
  f.skinny = batch == 1 && g.M <= SKINNY_MAX_M && g.K % 128 == 0 && !g.rowtab && !g.tiled;   // one decode step: latency-bound shape
  // Ways to split K: the widest split the width allows (a wave is left with 1 to 5 chunks: 16 to 80 f32 MFMAs instead
  // of 48 to 160) -- by K alone, for EVERY row count and either kernel.  A row's result depends on how K is split (the
  // order its partial sums are added in), so a split chosen by the number of rows made the arithmetic of a clip depend on
  // the size of the batch it was decoded in.  (Rounds 1 - 2 used 4 waves above 64 rows, "the chip is full": measured again
  // in round 3 the wide split is 2 % faster at 128 tiny clips, equal at 256 base clips, 2 % slower at 512 tiny clips.)
  // With it a clip decodes to the same bits alone, in a batch of 512, and as a row of a multi-position prompt step.
  f.nw = g.K % 512 == 0 ? 16 : g.K % 384 == 0 ? 12 : g.K % 256 == 0 ? 8 : 4;
  f.kind = (g.ln_s ? 4 : 0) | (g.gelu ? 2 : 0) | (g.residual ? 1 : 0);
  f.wh = g.w_half != 0;
  return f;
}

template <auto Kernel, int NW>
hipError_t sk_launch(const GemmArgs& g, hipStream_t s) {
  constexpr size_t smem = NW * (SK_WAVE_LDS + 64) * sizeof(float);
  if (smem > 64 * 1024) {        // above the default dynamic-LDS limit (the CU has 160 KB); first called outside any capture
    // the attribute belongs to the CURRENT device's copy of the kernel: once per device, not once per process
    static std::atomic<unsigned long long> done{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return e;
      done.fetch_or(bit, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(Kernel, dim3((g.N + 31) / 32, (g.M + 31) / 32), dim3(64 * NW), smem, s, g);
  return hipGetLastError();
}
// Run-time description -> template arguments, one step each: weights (TT: a ggml block type, or SK_DENSE), operand width,
// kind, split.  A form that is not built is hipErrorInvalidValue.
constexpr int SK_DENSE = -1;
template <int TT, bool WH, int KIND, int NW>
hipError_t sk_form(const GemmArgs& g, hipStream_t s) {
  constexpr bool LN = (KIND & 4) != 0, GELU = (KIND & 2) != 0, RES = (KIND & 1) != 0;
  if constexpr (!sk_form_exists(KIND, WH, TT != SK_DENSE)) return hipErrorInvalidValue;
  else if constexpr (TT == SK_DENSE) return sk_launch<gemm_skinny_f32_kernel<LN, GELU, RES, NW, WH>, NW>(g, s);
  else return sk_launch<gemm_skinny_q_kernel<TT, LN, GELU, RES, NW, WH>, NW>(g, s);
}
template <int TT, bool WH, int KIND>
hipError_t sk_split(int nw, const GemmArgs& g, hipStream_t s) {
  switch (nw) {
    case 16: return sk_form<TT, WH, KIND, 16>(g, s);
    case 12: return sk_form<TT, WH, KIND, 12>(g, s);
    case 8: return sk_form<TT, WH, KIND, 8>(g, s);
    default: return sk_form<TT, WH, KIND, 4>(g, s);
  }
}
template <int TT, bool WH>
hipError_t sk_kind(const SkinnyForm& f, const GemmArgs& g, hipStream_t s) {
  switch (f.kind) {
    case 0: return sk_split<TT, WH, 0>(f.nw, g, s);
    case 1: return sk_split<TT, WH, 1>(f.nw, g, s);
    case 2: return sk_split<TT, WH, 2>(f.nw, g, s);
    case 3: return sk_split<TT, WH, 3>(f.nw, g, s);
    case 4: return sk_split<TT, WH, 4>(f.nw, g, s);
    case 5: return sk_split<TT, WH, 5>(f.nw, g, s);
    case 6: return sk_split<TT, WH, 6>(f.nw, g, s);
    default: return sk_split<TT, WH, 7>(f.nw, g, s);
  }
}
template <int TT>
hipError_t sk_dispatch(const SkinnyForm& f, const GemmArgs& g, hipStream_t s) {
  return f.wh ? sk_kind<TT, true>(f, g, s) : sk_kind<TT, false>(f, g, s);
}

}  // namespace

// true when the resident-weight skinny kernel has a form for this product (the caller de-quantises into its scratch
// slot and takes the dense kernel otherwise)
bool skinny_q_supported(const GemmArgs& g, int batch) {
  const SkinnyForm f = skinny_form(g, batch);
  return f.skinny && f.exists(true);
}
hipError_t gemm_skinny_q(const GemmArgs& g, hipStream_t s) {
  const SkinnyForm f = skinny_form(g, 1);      // (the shape is the caller's to check: skinny_q_supported)
  switch (g.wq_type) {
    case QT_Q4_0: return sk_dispatch<QT_Q4_0>(f, g, s);
    case QT_Q4_1: return sk_dispatch<QT_Q4_1>(f, g, s);
    case QT_Q5_0: return sk_dispatch<QT_Q5_0>(f, g, s);
    case QT_Q5_1: return sk_dispatch<QT_Q5_1>(f, g, s);
    case QT_Q8_0: return sk_dispatch<QT_Q8_0>(f, g, s);
    default: return hipErrorInvalidValue;
  }
}
hipError_t gemm_f32_nt(const GemmArgs& g, int batch, hipStream_t s) {
  const SkinnyForm f = skinny_form(g, batch);
  if (f.skinny) return sk_dispatch<SK_DENSE>(f, g, s);
  if (g.w_half) return hipErrorInvalidValue;          // an f16 weight copy is only understood by the skinny kernel
  dim3 grid((g.N + GB_N - 1) / GB_N, (g.M + GB_M - 1) / GB_M, batch);
  hipLaunchKernelGGL(gemm_f32_nt_kernel, grid, dim3(256), 0, s, g);
  return hipGetLastError();
}
hipError_t layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, long rows, int D,
                         hipStream_t s) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  switch (D) {     // the widths of the Whisper family (tiny ... large)
    case 384: hipLaunchKernelGGL(layernorm_kernel<6>, grid, block, 0, s, x, gamma, beta, y, rows); break;
    case 512: hipLaunchKernelGGL(layernorm_kernel<8>, grid, block, 0, s, x, gamma, beta, y, rows); break;
    case 768: hipLaunchKernelGGL(layernorm_kernel<12>, grid, block, 0, s, x, gamma, beta, y, rows); break;
    case 1024: hipLaunchKernelGGL(layernorm_kernel<16>, grid, block, 0, s, x, gamma, beta, y, rows); break;
    case 1280: hipLaunchKernelGGL(layernorm_kernel<20>, grid, block, 0, s, x, gamma, beta, y, rows); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace crispy

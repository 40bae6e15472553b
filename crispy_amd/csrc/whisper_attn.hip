// whisper_attn.hip -- attention over f32 activations: the f32 encoder's, and the staged decode step's (gfx950).
//
//   attn_enc_kernel        encoder self-attention (precision mode 0), flash style, non-causal: one wave per 32 queries,
//                          S^T = K . Q^T on v_mfma_f32_32x32x2_f32 so that the soft-max statistics are per lane and P^T
//                          feeds the P . V products from registers.
//   attn_dec_kernel        one query row per (row, head) against a K|V cache: 16 waves split the keys, partial
//                          (max, sum, P . V) triples merged through LDS.  f32 K|V: self- and cross-attention of the f32
//                          decoder; f16 K|V: the staged step when the key bound is unknown or above 1536.
//   attn_dec_x16_kernel    the same over an f16 K|V of <= 1536 keys with every byte requested up front (1 / 2 / 4 / 12 key
//                          slots per wave): self- and cross-attention of the staged step in precision modes 1 and 2.
//   attn_dec_x16g_kernel   attn_dec_x16_kernel's arithmetic for the query rows of ONE clip together (a batched prompt
//                          step's positions, a fallback pass's decoders): the clip's K|V is loaded once per 8 rows.
//
// The three decode kernels partition the keys and merge the partial results in the same way, so a row's bits do not depend
// on which of them the launcher picks.  (The fused and matrix-vector decode paths have attention kernels of their own:
// whisper_dec_fused.hip, whisper_dec_gemv.hip.)
#include "asr_common.h"
#include "wave_ops.h"

namespace crispy {
namespace {

// ---------------------------------------------------------------------------------------------
// Encoder self-attention (non-causal), head dim 64.  qkv: [B][T][3*D] with q | k | v column blocks.
// grid (ceil(T/128), heads, B), 4 waves, wave = 32 queries.
//   S^T[key][q] = sum_d K[key][d] Q[q][d]    (A = K rows, B = Q^T; MFMA step s contracts d = s and s+32)
//   O^T[d][q]  += sum_key V[key][d] P^T[key][q]   (A = V^T, B = P^T straight from the S^T accumulator:
//                register r of lane half h is key (r&3) + 8(r>>2) + 4h, exactly the k-pair of step r)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_enc_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                       int T, int D) {
  __shared__ float stage[4][32 * 65];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * 128 + wave * 32;
  if (q0 >= T) return;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld;
  const float* Qp = base + h * 64;
  const float* Kp = base + D + h * 64;
  const float* Vp = base + 2 * D + h * 64;

  // Q operand: lane (q = li, half lh) holds Q[q][32*lh + s], s = 0..31, pre-scaled by 1/8 (exact)
  float qreg[32];
  {
    const int q = min(q0 + li, T - 1);
    const float4* p = reinterpret_cast<const float4*>(Qp + (long)q * ld + 32 * lh);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float4 t = p[c];
      qreg[4 * c] = t.x * 0.125f; qreg[4 * c + 1] = t.y * 0.125f;
      qreg[4 * c + 2] = t.z * 0.125f; qreg[4 * c + 3] = t.w * 0.125f;
    }
  }
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  // K rows of the next tile are loaded while the current tile's P.V MFMAs run, V rows before the softmax arithmetic:
  // with two waves per SIMD an exposed HBM/L2 round trip per product left the matrix pipe 40 % idle
  float kreg[32];
  auto load_k = [&](int k0) {
    const int key = min(k0 + li, T - 1);
    const float4* p = reinterpret_cast<const float4*>(Kp + (long)key * ld + 32 * lh);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float4 t = p[c];
      kreg[4 * c] = t.x; kreg[4 * c + 1] = t.y; kreg[4 * c + 2] = t.z; kreg[4 * c + 3] = t.w;
    }
  };
  load_k(0);
  for (int k0 = 0; k0 < T; k0 += 32) {
    // ---- S^T tile ----
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int st = 0; st < 32; ++st) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kreg[st], qreg[st], s, 0, 0, 0);
    // V rows of this tile and K rows of the next one go out now
    float v0[16], v1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = min(k0 + acc_row(r, lane), T - 1);
      const float* vp = Vp + (long)key * ld;
      v0[r] = vp[li];
      v1[r] = vp[32 + li];
    }
    if (k0 + 32 < T) load_k(k0 + 32);
    // ---- online softmax over this lane's 16 keys + the partner half's 16 ----
    float mloc = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, lane);
      if (key >= T) s[r] = -1e30f;
      mloc = fmaxf(mloc, s[r]);
    }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float m_new = fmaxf(m_run, mloc);
    const float alpha = __expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __expf(s[r] - m_new);
      s[r] = p;
      psum += p;
    }
    psum += __shfl_xor(psum, 32, 64);
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
    // ---- O^T += V^T . P^T ----
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[r], s[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[r], s[r], o1, 0, 0, 0);
    }
  }
  // ---- normalise, transpose through LDS, store rows of 64 floats ----
  const float inv = 1.f / l_run;
  float* st = stage[wave];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = acc_row(r, lane);
    st[li * 65 + d] = o0[r] * inv;
    st[li * 65 + 32 + d] = o1[r] * inv;
  }
  wave_lds_sync();
  for (int idx = lane; idx < 32 * 64; idx += 64) {
    const int q = idx >> 6, d = idx & 63;
    if (q0 + q < T) out[((long)b * T + q0 + q) * D + h * 64 + d] = st[q * 65 + d];
  }
}

// ---------------------------------------------------------------------------------------------
// Decoder attention for ONE query per (clip, head): scores against n_keys cached keys, softmax, P.V.
// q: [B][D] (row stride ldq), K/V: [B][n_ctx][ldkv] with this head's 64 columns at koff/voff + h*64.
// grid (heads, B), 4 waves: the keys are split four ways (flash-decoding style) and the partial
// (max, sum, P.V) triples are merged through LDS.  n_keys = n_keys_base + *pos_dev (graph replay keeps
// the launch arguments fixed while the position advances on the device).  Memory-bound on K/V.
// ---------------------------------------------------------------------------------------------
#ifndef AD_WAVES_N
#define AD_WAVES_N 16
#endif
constexpr int AD_WAVES = AD_WAVES_N;   // key partitions per (clip, head): 1.2 GB of cross K|V per step want many loads in flight
// NT: non-temporal request (the K|V stream of a decode step over many clips, see attn_dec_x16_kernel)
template <class KV, bool NT> __device__ __forceinline__ float4 ld4(const KV* p);
template <> __device__ __forceinline__ float4 ld4<float, false>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 ld4<float, true>(const float* p) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ float4 ld4<_Float16, false>(const _Float16* p) {
  const half4 h = *reinterpret_cast<const half4*>(p);
  return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
template <> __device__ __forceinline__ float4 ld4<_Float16, true>(const _Float16* p) {
  const half4 h = __builtin_nontemporal_load(reinterpret_cast<const half4*>(p));
  return make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
}
// KV = float (self-attention cache, default cross K|V) or _Float16 (cross K|V in precision mode 1: half the bytes of
// the stream that dominates a decode step; whisper.cpp keeps its KV caches in f16 as well)
template <class KV, bool STREAM_KV = false>
__global__ __launch_bounds__(64 * AD_WAVES) void attn_dec_kernel(const float* __restrict__ q, long ldq,
                                                       const KV* __restrict__ kv, long kv_batch_stride,
                                                       long ldkv, long head_stride, long koff, long voff, int n_keys_base,
                                                       const int* __restrict__ pos_dev, float* __restrict__ out, long ldo,
                                                       AttnRows rows) {
  __shared__ float p_s[1536];
  __shared__ __attribute__((aligned(16))) float q_s[64];
  __shared__ __attribute__((aligned(16))) float part_o[AD_WAVES][64];
  __shared__ float part_m[AD_WAVES], part_l[AD_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h = blockIdx.x, b = blockIdx.y;
  // rows.group query rows per clip (asr_common.h: AttnRows): row b belongs to clip b / group and reads that clip's K|V
  const int clip = b / rows.group;
  // rows.key_off: the clip's keys start at cache row key_off[clip] (left-padded prompts); the partition below then runs
  // over the same key COUNT from a shifted base -- the arithmetic of the un-padded clip, bit for bit
  const int k_off = rows.key_off ? rows.key_off[clip] : 0;
  const int n_keys = n_keys_base + (pos_dev ? *pos_dev : 0) + rows.key_step * (b % rows.group) - k_off;
  if (n_keys <= 0) {                    // a padding row in front of the clip's prompt: nothing to attend to, never read
    if (tid < 64) out[(long)b * ldo + h * 64 + tid] = 0.f;
    return;
  }
  if (tid < 64) q_s[tid] = q[(long)b * ldq + h * 64 + tid] * 0.125f;
  __syncthreads();
  const KV* Kb = kv + (long)clip * kv_batch_stride + koff + h * head_stride + (long)k_off * ldkv;
  const KV* Vb = kv + (long)clip * kv_batch_stride + voff + h * head_stride + (long)k_off * ldkv;
  const int per = (n_keys + AD_WAVES - 1) / AD_WAVES;
  const int k_lo = wave * per, k_hi = min(n_keys, k_lo + per);
  // scores: 16 lanes share one key row (coalesced 256-byte reads, 4 keys per wave instruction), the
  // 16 partial dot products are summed inside the DPP row
  float mloc = -1e30f;
  {
    const int c = lane & 15, sub = lane >> 4;
    const float4 qv = *reinterpret_cast<const float4*>(&q_s[4 * c]);
    constexpr int SU = 8;                                  // independent 1-KB loads in flight per wave
    for (int kb = k_lo; kb < k_hi; kb += 4 * SU) {
      float sacc[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int k = kb + 4 * u + sub;
        sacc[u] = 0.f;
        if (k < k_hi) {
          const float4 t = ld4<KV, STREAM_KV>(Kb + (long)k * ldkv + 4 * c);
          sacc[u] = t.x * qv.x;
          sacc[u] = fmaf(t.y, qv.y, sacc[u]);
          sacc[u] = fmaf(t.z, qv.z, sacc[u]);
          sacc[u] = fmaf(t.w, qv.w, sacc[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        float v = sacc[u];
        v = row_sum16(v);
        const int k = kb + 4 * u + sub;
        if (k < k_hi) {
          if (c == 0) p_s[k] = v;
          mloc = fmaxf(mloc, v);
        }
      }
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mloc = fmaxf(mloc, __shfl_xor(mloc, off, 64));
  float lsum = 0.f;
  for (int k = k_lo + lane; k < k_hi; k += 64) {
    const float p = __expf(p_s[k] - mloc);
    p_s[k] = p;
    lsum += p;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
  wave_lds_sync();
  // P.V with the same access shape as the scores: 16 lanes share one 256-byte V row (4 dims each), 4 rows per wave
  // instruction, SU instructions (8 KB) in flight per wave -- the one-float-per-lane version kept 2 KB in flight and
  // spent most of the kernel waiting on it.  The four key residues are summed across the DPP rows at the end.
  {
    const int c = lane & 15, sub = lane >> 4;
    constexpr int SU = 8;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kb = k_lo; kb < k_hi; kb += 4 * SU) {
      float4 t[SU];
      float p[SU];
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        const int k = kb + 4 * u + sub;
        t[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        p[u] = 0.f;
        if (k < k_hi) {
          t[u] = ld4<KV, STREAM_KV>(Vb + (long)k * ldkv + 4 * c);
          p[u] = p_s[k];
        }
      }
#pragma unroll
      for (int u = 0; u < SU; ++u) {
        acc.x = fmaf(p[u], t[u].x, acc.x);
        acc.y = fmaf(p[u], t[u].y, acc.y);
        acc.z = fmaf(p[u], t[u].z, acc.z);
        acc.w = fmaf(p[u], t[u].w, acc.w);
      }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      acc.x += __shfl_xor(acc.x, off, 64);
      acc.y += __shfl_xor(acc.y, off, 64);
      acc.z += __shfl_xor(acc.z, off, 64);
      acc.w += __shfl_xor(acc.w, off, 64);
    }
    if (sub == 0) *reinterpret_cast<float4*>(&part_o[wave][4 * c]) = acc;
  }
  if (lane == 0) { part_m[wave] = mloc; part_l[wave] = lsum; }
  __syncthreads();
  if (wave == 0) {
    float m = part_m[0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) m = fmaxf(m, part_m[w]);
    float o = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float sc = __expf(part_m[w] - m);   // empty partitions have m = -1e30 -> scale 0
      o = fmaf(part_o[w][lane], sc, o);
      l = fmaf(part_l[w], sc, l);
    }
    out[(long)b * ldo + h * 64 + lane] = o / l;
  }
}

// ---------------------------------------------------------------------------------------------
// Cross-attention of a decode step over an f16 K|V (precision mode 1), <= 1536 keys: every byte is requested before
// anything is computed.  A (clip, head) has 1500 keys x 128 bytes of K and as much of V; its 16 waves take 94 keys
// each -- 12 KB of K and 12 KB of V, which is 48 + 48 registers per lane.  So a wave issues its 24 sixteen-byte loads
// per lane back to back (8 lanes per key row, 8 keys per instruction: 1 KB per instruction), and the kernel is one
// round trip to HBM with the whole K|V of the layer in flight, instead of the generic kernel's K pass, softmax, V pass
// with 4 KB per wave in flight.  V does not wait for the scores; nothing goes through LDS but the 16 partial results.
// Same partitioning and merge as attn_dec_kernel (per-wave max / sum / P.V merged by wave 0).
// ---------------------------------------------------------------------------------------------
// ADX_SLOTS = key slots of 8 keys per wave: 12 for the cross-attention (16 waves x 96 keys >= 1536); 1 / 2 / 4 for the
// self-attention over the f16 K|V cache of mode 1 (<= 128 / 256 / 512 positions; the bound is known when the step is
// captured, the key count itself comes from the device counter).
template <int ADX_SLOTS, bool STREAM_KV>
__global__ __launch_bounds__(64 * AD_WAVES) void attn_dec_x16_kernel(const float* __restrict__ q, long ldq,
                                                       const _Float16* __restrict__ kv, long kv_batch_stride,
                                                       long ldkv, long head_stride, long koff, long voff, int n_keys_base,
                                                       const int* __restrict__ pos_dev, float* __restrict__ out, long ldo,
                                                       AttnRows rows) {
  // rows.group query rows per clip (asr_common.h: AttnRows): row b belongs to clip b / group and reads that clip's K|V
  const int b = blockIdx.y;
  const int clip = b / rows.group;
  const int k_off = rows.key_off ? rows.key_off[clip] : 0;       // see attn_dec_kernel
  const int n_keys = n_keys_base + (pos_dev ? *pos_dev : 0) + rows.key_step * (b % rows.group) - k_off;
  __shared__ __attribute__((aligned(16))) float part_o[AD_WAVES][64];
  __shared__ float part_m[AD_WAVES], part_l[AD_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h = blockIdx.x;
  if (n_keys <= 0) {
    if (tid < 64) out[(long)b * ldo + h * 64 + tid] = 0.f;
    return;
  }
  const int c = lane & 7, r = lane >> 3;
  const _Float16* Kb = kv + (long)clip * kv_batch_stride + koff + h * head_stride + 8 * c + (long)k_off * ldkv;
  const _Float16* Vb = kv + (long)clip * kv_batch_stride + voff + h * head_stride + 8 * c + (long)k_off * ldkv;
  const int per = (n_keys + AD_WAVES - 1) / AD_WAVES;
  const int k_lo = wave * per, k_hi = min(n_keys, k_lo + per);
  const int k_last = max(k_hi - 1, 0);          // clamp target of the slots past the partition (weight 0)
  half8 kr[ADX_SLOTS], vr[ADX_SLOTS];
  // rows.stream_kv: the K|V of a decode step over many clips is a one-pass stream (0.6 GB per position at 64 tiny clips):
  // requested non-temporally it no longer pushes the decoder's weights (3 MB per XCD, re-read every step) out of the
  // L2s: 11.25 -> 10.45 ms per 36 positions at 64 tiny clips, 46.4 -> 43.7 ms at 256 base clips.  For a few clips the
  // K|V itself is what stays cached from step to step, and the plain loads are 9 % faster (one clip: 5.95 vs 6.5 ms).
  // (a template parameter: a run-time choice between the two kinds of load -- select or branch -- is folded into one plain
  // load by the optimiser)
#pragma unroll
  for (int i = 0; i < ADX_SLOTS; ++i) {
    const half8* p = reinterpret_cast<const half8*>(Kb + (long)min(k_lo + 8 * i + r, k_last) * ldkv);
    kr[i] = STREAM_KV ? __builtin_nontemporal_load(p) : *p;
  }
#pragma unroll
  for (int i = 0; i < ADX_SLOTS; ++i) {
    const half8* p = reinterpret_cast<const half8*>(Vb + (long)min(k_lo + 8 * i + r, k_last) * ldkv);
    vr[i] = STREAM_KV ? __builtin_nontemporal_load(p) : *p;
  }
  __builtin_amdgcn_sched_barrier(0);            // the scheduler would otherwise keep 9 loads in flight and interleave the rest
  float qv[8];
  {
    const float4 q0 = *reinterpret_cast<const float4*>(q + (long)b * ldq + h * 64 + 8 * c);
    const float4 q1 = *reinterpret_cast<const float4*>(q + (long)b * ldq + h * 64 + 8 * c + 4);
    qv[0] = q0.x; qv[1] = q0.y; qv[2] = q0.z; qv[3] = q0.w;
    qv[4] = q1.x; qv[5] = q1.y; qv[6] = q1.z; qv[7] = q1.w;
    if (rows.attn16) {       // the query as ggml's K.q sees it: rounded BEFORE the scaling (q / 8 may be an f16 subnormal where q is not)
#pragma unroll
      for (int e = 0; e < 8; ++e) qv[e] = (float)(_Float16)qv[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] *= 0.125f;
  }
  float sc[ADX_SLOTS];
  float mloc = -1e30f;
#pragma unroll
  for (int i = 0; i < ADX_SLOTS; ++i) {
    float v = (float)kr[i][0] * qv[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) v = fmaf((float)kr[i][e], qv[e], v);
    v = row_sum8(v);       // the 8 lanes of a key row
    const bool valid = k_lo + 8 * i + r < k_hi;
    sc[i] = valid ? v : -1e30f;
    mloc = fmaxf(mloc, sc[i]);
  }
  mloc = shfl_max<8, 32>(mloc);
  float lsum = 0.f;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  float inv16 = 0.f;           // attn16: 1 / (sum over ALL keys); the maximum is the row's, not the wave's
  if (rows.attn16) {
    if (lane == 0) part_m[wave] = mloc;
    __syncthreads();
    float m = part_m[0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) m = fmaxf(m, part_m[w]);
    mloc = m;
    float ls = 0.f;
#pragma unroll
    for (int i = 0; i < ADX_SLOTS; ++i) ls += k_lo + 8 * i + r < k_hi ? __expf(sc[i] - mloc) : 0.f;
#pragma unroll
    for (int off = 8; off <= 32; off <<= 1) ls += __shfl_xor(ls, off, 64);     // the eight lanes of a key hold the same score
    if (lane == 0) part_l[wave] = ls;
    __syncthreads();
    float l = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) l += part_l[w];
    inv16 = 1.f / l;
    __syncthreads();           // part_m / part_l are written again below
  }
#pragma unroll
  for (int i = 0; i < ADX_SLOTS; ++i) {
    float pw = k_lo + 8 * i + r < k_hi ? __expf(sc[i] - mloc) : 0.f;
    if (rows.attn16) pw = (float)(_Float16)(pw * inv16);      // the normalised probability as ggml's P.V sees it
    lsum += pw;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pw, (float)vr[i][e], acc[e]);
  }
#pragma unroll
  for (int off = 8; off <= 32; off <<= 1) {
    lsum += __shfl_xor(lsum, off, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], off, 64);
  }
  if (r == 0) {
    *reinterpret_cast<float4*>(&part_o[wave][8 * c]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(&part_o[wave][8 * c + 4]) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
  if (lane == 0) { part_m[wave] = mloc; part_l[wave] = lsum; }
  __syncthreads();
  if (wave == 0) {
    float m = part_m[0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) m = fmaxf(m, part_m[w]);
    float o = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float scl = __expf(part_m[w] - m);   // empty partitions have m = -1e30 -> scale 0
      o = fmaf(part_o[w][lane], scl, o);
      l = fmaf(part_l[w], scl, l);
    }
    // attn16: the probabilities were normalised before they were rounded (every wave's maximum is the row's: scl = 1)
    out[(long)b * ldo + h * 64 + lane] = rows.attn16 ? o : o / l;
  }
}

// ---------------------------------------------------------------------------------------------
// The same cross-attention for the query rows of ONE clip together (rows.group > 1, every row over the same keys:
// the positions of a batched prompt step, the decoders of a fallback pass): one workgroup per (head, clip, chunk of
// ADG_ROWS rows) holds the clip's K and V of the head in registers once and takes its rows one after the other -- with
// a workgroup per row the clip's K | V reaches the CUs once per row (from the XCD's L2 after the first), and a prompt
// step over 64 clips x 4 positions was 85 us per layer against 30 for the bytes from HBM.  Per row exactly
// attn_dec_x16_kernel's arithmetic (partition, per-wave triples, merge), so a row's bits do not depend on the form.
// The row loop is kept rolled and the f16 -> f32 conversions pinned inside it (hoisted, they are 96 more registers).
// ---------------------------------------------------------------------------------------------
constexpr int ADG_ROWS = 8;
template <bool STREAM_KV>
__global__ __launch_bounds__(64 * AD_WAVES) void attn_dec_x16g_kernel(const float* __restrict__ q, long ldq, const _Float16* __restrict__ kv,
                                                                      long kv_batch_stride, long ldkv, long head_stride, long koff, long voff,
                                                                      int n_keys, float* __restrict__ out, long ldo, AttnRows rows) {
  constexpr int SL = 12;
  __shared__ __attribute__((aligned(16))) float part_o[ADG_ROWS][AD_WAVES][64];
  __shared__ float part_m[ADG_ROWS][AD_WAVES], part_l[ADG_ROWS][AD_WAVES];
  __shared__ float wave_m[ADG_ROWS][AD_WAVES], wave_l[ADG_ROWS][AD_WAVES];
  __shared__ float sc_s[ADG_ROWS][AD_WAVES][SL][8];          // the scores: 6 KB per row (in registers they do not fit beside the keys)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int h = blockIdx.x, clip = blockIdx.y;
  const int r_lo = blockIdx.z * ADG_ROWS, n_r = min(ADG_ROWS, rows.group - r_lo);
  const int c = lane & 7, r = lane >> 3;
  const _Float16* Kb = kv + (long)clip * kv_batch_stride + koff + h * head_stride + 8 * c;
  const _Float16* Vb = kv + (long)clip * kv_batch_stride + voff + h * head_stride + 8 * c;
  const int per = (n_keys + AD_WAVES - 1) / AD_WAVES;
  const int k_lo = wave * per, k_hi = min(n_keys, k_lo + per);
  const int k_last = max(k_hi - 1, 0);
  half8 kr[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const half8* p = reinterpret_cast<const half8*>(Kb + (long)min(k_lo + 8 * i + r, k_last) * ldkv);
    kr[i] = STREAM_KV ? __builtin_nontemporal_load(p) : *p;
  }
  __builtin_amdgcn_sched_barrier(0);
  // scores of every row of the chunk from the keys in registers
#pragma unroll 1
  for (int j = 0; j < n_r; ++j) {
    const long b = (long)clip * rows.group + r_lo + j;
    float qv[8];
    const float4 q0 = *reinterpret_cast<const float4*>(q + b * ldq + h * 64 + 8 * c);
    const float4 q1 = *reinterpret_cast<const float4*>(q + b * ldq + h * 64 + 8 * c + 4);
    qv[0] = q0.x; qv[1] = q0.y; qv[2] = q0.z; qv[3] = q0.w;
    qv[4] = q1.x; qv[5] = q1.y; qv[6] = q1.z; qv[7] = q1.w;
    if (rows.attn16) {
#pragma unroll
      for (int e = 0; e < 8; ++e) qv[e] = (float)(_Float16)qv[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] *= 0.125f;
    float mloc = -1e30f;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      asm volatile("" : "+v"(kr[i]));
      float v = (float)kr[i][0] * qv[0];
#pragma unroll
      for (int e = 1; e < 8; ++e) v = fmaf((float)kr[i][e], qv[e], v);
      v = row_sum8(v);       // the 8 lanes of a key row
      const float sc = k_lo + 8 * i + r < k_hi ? v : -1e30f;
      if (c == 0) sc_s[j][wave][i][r] = sc;
      mloc = fmaxf(mloc, sc);
    }
    mloc = shfl_max<8, 32>(mloc);
    if (lane == 0) wave_m[j][wave] = mloc;
  }
  // the values, into the registers the keys leave
  __builtin_amdgcn_sched_barrier(0);
  half8 vr[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const half8* p = reinterpret_cast<const half8*>(Vb + (long)min(k_lo + 8 * i + r, k_last) * ldkv);
    vr[i] = STREAM_KV ? __builtin_nontemporal_load(p) : *p;
  }
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();
  if (rows.attn16) {             // mode 2: every row's maximum and sum over ALL keys before a probability is rounded
#pragma unroll 1
    for (int j = 0; j < n_r; ++j) {
      float m = wave_m[j][0];
#pragma unroll
      for (int w = 1; w < AD_WAVES; ++w) m = fmaxf(m, wave_m[j][w]);
      float ls = 0.f;
#pragma unroll
      for (int i = 0; i < SL; ++i) ls += k_lo + 8 * i + r < k_hi ? __expf(sc_s[j][wave][i][r] - m) : 0.f;
#pragma unroll
      for (int off = 8; off <= 32; off <<= 1) ls += __shfl_xor(ls, off, 64);
      if (lane == 0) wave_l[j][wave] = ls;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int j = 0; j < n_r; ++j) {
    float mloc = wave_m[j][wave], inv16 = 0.f;
    if (rows.attn16) {
      float l = 0.f;
      mloc = wave_m[j][0];
#pragma unroll
      for (int w = 1; w < AD_WAVES; ++w) mloc = fmaxf(mloc, wave_m[j][w]);
#pragma unroll
      for (int w = 0; w < AD_WAVES; ++w) l += wave_l[j][w];
      inv16 = 1.f / l;
    }
    float lsum = 0.f;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      float pw = k_lo + 8 * i + r < k_hi ? __expf(sc_s[j][wave][i][r] - mloc) : 0.f;
      if (rows.attn16) pw = (float)(_Float16)(pw * inv16);
      lsum += pw;
      asm volatile("" : "+v"(vr[i]));
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(pw, (float)vr[i][e], acc[e]);
    }
#pragma unroll
    for (int off = 8; off <= 32; off <<= 1) {
      lsum += __shfl_xor(lsum, off, 64);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], off, 64);
    }
    if (r == 0) {
      *reinterpret_cast<float4*>(&part_o[j][wave][8 * c]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(&part_o[j][wave][8 * c + 4]) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
    if (lane == 0) { part_m[j][wave] = mloc; part_l[j][wave] = lsum; }
  }
  __syncthreads();
  if (wave < n_r) {              // row `wave` of the chunk: the merge of its 16 triples
    float m = part_m[wave][0];
#pragma unroll
    for (int w = 1; w < AD_WAVES; ++w) m = fmaxf(m, part_m[wave][w]);
    float o = 0.f, l = 0.f;
#pragma unroll
    for (int w = 0; w < AD_WAVES; ++w) {
      const float scl = __expf(part_m[wave][w] - m);
      o = fmaf(part_o[wave][w][lane], scl, o);
      l = fmaf(part_l[wave][w], scl, l);
    }
    out[((long)clip * rows.group + r_lo + wave) * ldo + h * 64 + lane] = rows.attn16 ? o : o / l;
  }
}

}  // namespace

hipError_t attn_encoder_f32(const float* qkv, float* out, int B, int T, int D, int heads, hipStream_t s) {
  hipLaunchKernelGGL(attn_enc_kernel, dim3((T + 127) / 128, heads, B), dim3(256), 0, s, qkv, out, T, D);
  return hipGetLastError();
}
hipError_t attn_decoder_f32(const float* q, long ldq, const float* kv, long kv_batch_stride, long ldkv, long head_stride,
                            long koff, long voff, int n_keys_base, const int* pos_dev, float* out, long ldo, int B, int heads,
                            hipStream_t s, AttnRows rows) {
  if (rows.group < 1) return hipErrorInvalidValue;
  if (rows.stream_kv)
    hipLaunchKernelGGL((attn_dec_kernel<float, true>), dim3(heads, B), dim3(64 * AD_WAVES), 0, s, q, ldq, kv, kv_batch_stride, ldkv, head_stride, koff,
                       voff, n_keys_base, pos_dev, out, ldo, rows);
  else
    hipLaunchKernelGGL((attn_dec_kernel<float, false>), dim3(heads, B), dim3(64 * AD_WAVES), 0, s, q, ldq, kv, kv_batch_stride, ldkv, head_stride, koff,
                       voff, n_keys_base, pos_dev, out, ldo, rows);
  return hipGetLastError();
}
hipError_t attn_decoder_kv16(const float* q, long ldq, const void* kv, long kv_batch_stride, long ldkv, long head_stride,
                             long koff, long voff, int n_keys_base, const int* pos_dev, float* out, long ldo, int B, int heads,
                             hipStream_t s, int max_keys, AttnRows rows) {
  if (rows.group < 1) return hipErrorInvalidValue;
  const int bound = max_keys > 0 ? max_keys : n_keys_base + rows.key_step * (rows.group - 1);
  if ((max_keys > 0 || !pos_dev) && bound <= AD_WAVES * 8 * 12 && AD_WAVES == 16) {   // every byte of K|V requested up front
    const _Float16* kvh = reinterpret_cast<const _Float16*>(kv);
#define CRISPY_ADX(SL) hipLaunchKernelGGL((attn_dec_x16_kernel<SL, false>), dim3(heads, B), dim3(64 * AD_WAVES), 0, s, q, ldq, kvh, \
                                          kv_batch_stride, ldkv, head_stride, koff, voff, n_keys_base, pos_dev, out, ldo, rows)
    // several rows per clip over the same keys (a prompt step's positions, a pass's decoders): the clip's K | V once per chunk of rows
    // (worth it once the one-workgroup-per-row grid is several rounds of the CUs: a row's pass is a latency chain of its own)
    if (rows.group > 1 && rows.key_step == 0 && !rows.key_off && !pos_dev && B % rows.group == 0 && bound > AD_WAVES * 32 && n_keys_base > 0 &&
        (long)heads * B > 512) {
      const dim3 grid(heads, B / rows.group, (rows.group + ADG_ROWS - 1) / ADG_ROWS);
      if (rows.stream_kv)
        hipLaunchKernelGGL((attn_dec_x16g_kernel<true>), grid, dim3(64 * AD_WAVES), 0, s, q, ldq, kvh, kv_batch_stride, ldkv, head_stride, koff,
                           voff, n_keys_base, out, ldo, rows);
      else
        hipLaunchKernelGGL((attn_dec_x16g_kernel<false>), grid, dim3(64 * AD_WAVES), 0, s, q, ldq, kvh, kv_batch_stride, ldkv, head_stride, koff,
                           voff, n_keys_base, out, ldo, rows);
      return hipGetLastError();
    }
    if (rows.stream_kv && bound > AD_WAVES * 32) {     // the cross-attention of a step over many clips
      hipLaunchKernelGGL((attn_dec_x16_kernel<12, true>), dim3(heads, B), dim3(64 * AD_WAVES), 0, s, q, ldq, kvh, kv_batch_stride,
                         ldkv, head_stride, koff, voff, n_keys_base, pos_dev, out, ldo, rows);
      return hipGetLastError();
    }
    if (bound <= AD_WAVES * 8) CRISPY_ADX(1);
    else if (bound <= AD_WAVES * 16) CRISPY_ADX(2);
    else if (bound <= AD_WAVES * 32) CRISPY_ADX(4);
    else CRISPY_ADX(12);
#undef CRISPY_ADX
    return hipGetLastError();
  }
  if (rows.attn16) return hipErrorInvalidValue;      // only the all-keys-up-front kernel above rounds inside the attention
  hipLaunchKernelGGL((attn_dec_kernel<_Float16, false>), dim3(heads, B), dim3(64 * AD_WAVES), 0, s, q, ldq,
                     reinterpret_cast<const _Float16*>(kv), kv_batch_stride, ldkv, head_stride, koff, voff, n_keys_base, pos_dev, out, ldo, rows);
  return hipGetLastError();
}

}  // namespace crispy

// pk_attn_f16.hip -- attention mode 1 of the Parakeet encoder for MI355X (gfx950): the three products of the relative-position
// attention -- (Q + u) . K^T, the position band product (Q + v) . R^T and P . V -- with operands rounded once to IEEE binary16
// (round to nearest even, subnormals kept, overflow to infinity) and f32 sums on v_mfma_f32_32x32x16_f16.  The definition is in
// include/crispy_hip.h ("Parakeet encoder, attention mode 1"); the key tile of its soft-max is CRISPY_PK_ATTN_KEY_TILE = 32.
//
// One workgroup (four waves) per (clip, head, 128 queries); wave w owns queries 32 w ... 32 w + 31 and keeps Q + u and Q + v as
// B operands in registers (64 VGPRs) for the whole workgroup.  Keys come in tiles of 32.  K and V tiles and the band of R sit in
// LDS as halves, rounded on the way in, in [row][128] images with padded rows (272 bytes where rows are read with ds_read_b128, 320 for
// V, which is read with ds_read_b64_tr_b16): both kinds of read are conflict-free and every address is a base and a constant.
//
// The scores are formed transposed, S^T = K . (Q + u)^T: the accumulator has one query per lane column and 16 of the tile's 32
// keys in its registers, the other 16 in lane ^ 32.  So the row maximum and sum are register operations and one exchange, and
// the registers, rounded to f16, are the B operand of O^T = V^T . P^T as they stand: registers 8 s ... 8 s + 7 are k-step s, whose
// element j of lane half h is key 16 s + 8 (j >> 2) + 4 h + (j & 3); the V^T operand is read from the [key][dim] image in that
// key order by two transposed reads per step.  P never goes through LDS.
//
// The position term of query i and key j is the band product's entry at d = i - j.  For the workgroup's queries i0 ... i0 + 127
// and the tile's keys j0 ... j0 + 31 that is d = i0 - j0 - 31 ... i0 - j0 + 127: five blocks of 32 rows of R, of which the next
// tile needs four again.  They live in a ring of five blocks (40 KB), one new block per tile.  Wave w multiplies the two blocks
// that hold its 63 distances by (Q + v)^T; each 32 x 32 result goes through the wave's own 4 KB of LDS as [band row][query], from
// which lane (query i, key j) takes row i - j + 31 (stride 32: the skewed read is conflict-free).
//
// LDS: 8.5 (K) + 10 (V) + 16 (the waves' band results) + 42.5 KB (the ring) = 77 KB, two workgroups per CU.  The rows of tile t + 1 are requested once the scores are formed, where their registers are free, and are in
// flight during P . V and the barrier; the other workgroup of the CU covers the rest of their latency.
// Everything is indexed from the clip's own first frame; keys behind its last are zeros whose scores are masked, queries behind
// it are never stored: a clip's frames do not depend on the batch or on its neighbours.
#include <cmath>

#include "pk_internal.h"
#include "wave_ops.h"

namespace crispy {
namespace pk {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 tr16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));      // what the transposed read's builtin returns

constexpr int kD = kHeadDim, kQ = kAttnF16Q, kT = kAttnF16K, kRing = 5;
static_assert(kD == 128 && kQ == 128 && kT == 32 && kT == CRISPY_PK_ATTN_KEY_TILE, "the wave roles below are written for 128 queries x 32 keys of 128-wide heads");
// bytes: K [32][128] halves, V [32][128] halves, the ring of R [5 x 32][128] halves, per wave [32 band rows][32 queries] floats
// Row strides: 256 bytes of halves and a pad, so that every address is one base and a constant.  272 (17 chunks of 16 bytes): the
// 16 rows of each lane group of a ds_read_b128 start in 16 different chunks modulo 16.  320: the four rows of a transposed read's
// block are 16 banks apart, and its 32 lanes' 8 bytes (16 tq + 8 tg + 2 tp) fill the 64 banks once.
constexpr int kRowK = kD * 2 + 16, kRowV = kD * 2 + 64;
constexpr int kSkew = 32 * 32 * (int)sizeof(float);      // one wave's [band row][query] floats
constexpr int kOffK = 0, kOffV = kOffK + kT * kRowK, kOffS = kOffV + kT * kRowV, kOffR = kOffS + 4 * kSkew, kLdsBytes = kOffR + kRing * 32 * kRowK;
static_assert(kLdsBytes == 78848 && 2 * kLdsBytes <= 160 * 1024, "two workgroups per CU");
static_assert(kOffS >= kSkew && kRing * 32 * kRowK >= kSkew, "the skewed reads stay inside the allocation");

// four floats of row `row`, dims 4 c4 ... 4 c4 + 3, rounded to halves
template <int STRIDE>
__device__ __forceinline__ void put4(char* img, int row, int c4, const float4& v) {
  f16x4 h;
  h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
  *reinterpret_cast<f16x4*>(img + row * STRIDE + 8 * c4) = h;
}

__device__ __forceinline__ float4 keep(bool in, const float4& v) { return make_float4(in ? v.x : 0.0f, in ? v.y : 0.0f, in ? v.z : 0.0f, in ? v.w : 0.0f); }

__device__ __forceinline__ int mod_ring(int b) { return ((b % kRing) + kRing) % kRing; }

__global__ __launch_bounds__(256, 2) void pk_attn_f16_kernel(const float* __restrict__ qkv, const float* __restrict__ r, const float* __restrict__ bias_u,
                                                             const float* __restrict__ bias_v, float* __restrict__ out, const int* __restrict__ off,
                                                             int H, int tmax) {
  extern __shared__ __attribute__((aligned(16))) char sm[];
  char* ks = sm + kOffK;      // [key][dim]
  char* vs = sm + kOffV;      // [key][dim]
  char* rs = sm + kOffR;      // [ring block][row][dim]: block b holds d = 32 b - 31 ... 32 b
  const int clip = blockIdx.z, head = blockIdx.y, i0 = blockIdx.x * kQ;
  const int r0 = off[clip], n = off[clip + 1] - r0;
  if (i0 >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, lh = lane >> 5;
  const size_t ld = (size_t)3 * H;
  const float* qbase = qkv + (size_t)r0 * ld + (size_t)head * kD;
  const float* rbase = r + (size_t)head * kD;
  const int srow = tid >> 5, sc4 = tid & 31;      // this thread's row (and row + 8 it) and float4 of a 32-row block it stages

  float4 pk[4], pv[4], pr[4];      // the next tile's K and V rows and its new block of R, in flight
  // keys behind the clip's last: zeros (the clip's row 0 is read in their place), and their scores are masked
  auto load_k = [&](int j0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int j = j0 + srow + 8 * it;
      pk[it] = keep(j < n, *reinterpret_cast<const float4*>(qbase + (size_t)(j < n ? j : 0) * ld + H + 4 * sc4));
    }
  };
  auto load_v = [&](int j0) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int j = j0 + srow + 8 * it;
      pv[it] = keep(j < n, *reinterpret_cast<const float4*>(qbase + (size_t)(j < n ? j : 0) * ld + 2 * H + 4 * sc4));
    }
  };
  // block b of R: rows for d = 32 b - 31 + row, at p = d + tmax - 1 of the table; zeros outside it
  auto load_r = [&](int b) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int p = 32 * b - 31 + srow + 8 * it + (tmax - 1);
      const bool in = p >= 0 && p < 2 * tmax - 1;
      pr[it] = keep(in, *reinterpret_cast<const float4*>(rbase + (size_t)(in ? p : 0) * H + 4 * sc4));
    }
  };
  auto store_r = [&](int b) {
    const int slot = mod_ring(b);
#pragma unroll
    for (int it = 0; it < 4; ++it) put4<kRowK>(rs, slot * 32 + srow + 8 * it, sc4, pr[it]);
  };

  // tile t (keys from j0 = 32 t) needs blocks beta ... beta + 4 with beta = i0 / 32 - t; wave w blocks beta + w and beta + w + 1
  const int beta0 = i0 / 32;
  for (int b = 1; b < kRing; ++b) {
    load_r(beta0 + b);
    store_r(beta0 + b);
  }
  asm volatile("" ::: "memory");      // before the operands below take their registers

  // this lane's B operands of the eight 16-deep steps: query 32 wave + li, dims 16 s + 8 lh + j in element j
  f16x8 qu[kD / 16], qv[kD / 16];
  {
    const int i = i0 + 32 * wave + li;
    const bool in = i < n;
    const float* qrow = qbase + (size_t)(in ? i : 0) * ld;
#pragma unroll
    for (int s = 0; s < kD / 16; ++s) {
      const int d0 = 16 * s + 8 * lh;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const float4 q = *reinterpret_cast<const float4*>(qrow + d0 + 4 * half);      // of row 0 when not `in`: dropped below
        const float4 u = *reinterpret_cast<const float4*>(bias_u + head * kD + d0 + 4 * half);
        const float4 v = *reinterpret_cast<const float4*>(bias_v + head * kD + d0 + 4 * half);
        // rows behind the clip's last are zeros: never stored
        qu[s][4 * half + 0] = in ? (_Float16)(q.x + u.x) : (_Float16)0.0f;
        qu[s][4 * half + 1] = in ? (_Float16)(q.y + u.y) : (_Float16)0.0f;
        qu[s][4 * half + 2] = in ? (_Float16)(q.z + u.z) : (_Float16)0.0f;
        qu[s][4 * half + 3] = in ? (_Float16)(q.w + u.w) : (_Float16)0.0f;
        qv[s][4 * half + 0] = in ? (_Float16)(q.x + v.x) : (_Float16)0.0f;
        qv[s][4 * half + 1] = in ? (_Float16)(q.y + v.y) : (_Float16)0.0f;
        qv[s][4 * half + 2] = in ? (_Float16)(q.z + v.z) : (_Float16)0.0f;
        qv[s][4 * half + 3] = in ? (_Float16)(q.w + v.w) : (_Float16)0.0f;
      }
      asm volatile("" : "+v"(qu[s]), "+v"(qv[s]) : : "memory");      // one step at a time, finished: as f32, hoisted together, they cost 192 registers
    }
  }

  load_k(0);
  load_v(0);
  load_r(beta0);

  const float scale = 0.08838834764831845f;      // 128^-1/2
  float* sb = reinterpret_cast<float*>(sm + kOffS) + wave * (32 * 32);
  // [li - key + 31 - 32 hf][li] at skew[32 (27 - (key - 4 lh)) + 1024 (1 - hf)]: one address, constant offsets
  const float* skew = sb + (li + 31 - 4 * lh - 27 - 32) * 32 + li;
  float m_run = -INFINITY, l_run = 0.0f;
  f32x16 o[4];      // O^T: dims 32 blk + (reg & 3) + 8 (reg >> 2) + 4 lh of query li
#pragma unroll
  for (int blk = 0; blk < 4; ++blk)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[blk][i] = 0.0f;

  for (int j0 = 0, beta = beta0; j0 < n; j0 += kT, --beta) {
    __syncthreads();      // the tile before, and the block that `beta` replaces in the ring, have been read
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      put4<kRowK>(ks, srow + 8 * it, sc4, pk[it]);
      put4<kRowV>(vs, srow + 8 * it, sc4, pv[it]);
    }
    store_r(beta);
    __syncthreads();
    const bool more = j0 + kT < n;

    // the band first: block beta + wave + hf holds this wave's band rows c = 32 hf ... 32 hf + 31, and entry (query i, key j) is
    // row c = i - j + 31.  Lane (query li), register i: key (i & 3) + 8 (i >> 2) + 4 lh
    float bd[16];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int row = mod_ring(beta + wave + hf) * 32 + li;
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
      for (int s = 0; s < kD / 16; ++s) {
        const f16x8 a = *reinterpret_cast<const f16x8*>(rs + row * kRowK + 16 * lh + 32 * s);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qv[s], acc, 0, 0, 0);
      }
      wave_lds_sync();      // the reads of the half before
      float* put = sb + 4 * lh * 32 + li;      // [band row (reg & 3) + 8 (reg >> 2) + 4 lh][li]
      asm volatile("" : "+v"(put));            // one address and 16 constant offsets, not 16 addresses kept across the loop
#pragma unroll
      for (int i = 0; i < 16; ++i) put[((i & 3) + 8 * (i >> 2)) * 32] = acc[i];
      wave_lds_sync();
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        // row c - 32 hf of this half with c = li - key + 31: mine when it is one of the half's 32 rows (hf 0: li <= key, hf 1:
        // li > key).  The other reads land in the neighbouring 4 KB on either side (the V image, the ring) and are dropped.  By design
        // they race with the writes of the wave that owns those bytes: whatever they return is never used, not even in arithmetic.
        const int key = (i & 3) + 8 * (i >> 2) + 4 * lh;
        const float v = skew[32 * (27 - (key - 4 * lh)) + 1024 * (1 - hf)];
        if (hf == 0) bd[i] = v;
        else bd[i] = li > key ? v : bd[i];
      }
    }
    // S^T = K . (Q + u)^T, in the same registers' key order
    f32x16 ac;
#pragma unroll
    for (int i = 0; i < 16; ++i) ac[i] = 0.0f;
#pragma unroll
    for (int s = 0; s < kD / 16; ++s) {
      const f16x8 a = *reinterpret_cast<const f16x8*>(ks + li * kRowK + 16 * lh + 32 * s);
      ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qu[s], ac, 0, 0, 0);
    }
    // the tile's step of the soft-max, per query: 16 keys here, 16 in lane ^ 32
    float sc[16], mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = j0 + (i & 3) + 8 * (i >> 2) + 4 * lh;
      sc[i] = j < n ? (ac[i] + bd[i]) * scale : -INFINITY;
      mx = fmaxf(mx, sc[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);      // finite: key j0 is the clip's own
    const float alpha = expf(m_run - m_new);
    float sum = 0.0f;
    f16x8 pf[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float p = expf(sc[i] - m_new);
      sum += p;
      pf[i >> 3][i & 7] = (_Float16)p;
    }
    sum += __shfl_xor(sum, 32, 64);
    l_run = fmaf(l_run, alpha, sum);
    m_run = m_new;
    // O^T = O^T alpha + V^T . P^T: step s takes keys 16 s + 8 (j >> 2) + 4 lh + (j & 3) in element j, the order of P's registers
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[blk][i] *= alpha;
    if (more) {      // the next tile's rows, in flight during P . V: the scores' registers are free again
      load_k(j0 + kT);
      load_v(j0 + kT);
      load_r(beta - 1);
    }
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;      // the transposed read: row q of the block, columns 4 p ... 4 p + 3
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int blk = 0; blk < 4; ++blk) {
        tr16x4 part[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const char* at = vs + (4 * lh + tq) * kRowV + 32 * tg + 8 * tp + (16 * s + 8 * u) * kRowV + 64 * blk;
          part[u] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) tr16x4*)(at));
        }
        const f16x4 lo = __builtin_bit_cast(f16x4, part[0]), hi = __builtin_bit_cast(f16x4, part[1]);
        f16x8 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a[j] = lo[j];
          a[4 + j] = hi[j];
        }
        o[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[s], o[blk], 0, 0, 0);
      }
    }
  }
  const int i = i0 + 32 * wave + li;
  if (i < n) {
    float* row = out + (size_t)(r0 + i) * H + (size_t)head * kD;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4*>(row + 32 * blk + 8 * g + 4 * lh) =
            make_float4(o[blk][4 * g] / l_run, o[blk][4 * g + 1] / l_run, o[blk][4 * g + 2] / l_run, o[blk][4 * g + 3] / l_run);
  }
}

}  // namespace

hipError_t launch_attention_f16(const PkLayer& l, const PkTables& t, const float* d_qkv, const float* d_r, int tmax, int heads, float* d_out, hipStream_t st) {
  if (t.n_clips < 1 || t.max_len[3] < 1 || tmax < t.max_len[3] || heads < 1) return hipErrorInvalidValue;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pk_attn_f16_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pk_attn_f16_kernel, dim3((t.max_len[3] + kQ - 1) / kQ, heads, t.n_clips), dim3(256), kLdsBytes, st, d_qkv, d_r, l.bias_u, l.bias_v,
                     d_out, t.off[3], heads * kD, tmax);
  return hipGetLastError();
}

// The encoder's form: the handle's attention mode picks the f32 kernel of pk_attn.hip or the f16-operand one above.
hipError_t launch_attention(int mode, const PkLayer& l, const PkTables& t, const float* d_qkv, const float* d_r, int tmax, int heads, float* d_out,
                            hipStream_t st) {
  if (mode == 1) return launch_attention_f16(l, t, d_qkv, d_r, tmax, heads, d_out, st);
  if (mode != 0) return hipErrorInvalidValue;
  return launch_attention(l, t, d_qkv, d_r, tmax, heads, d_out, st);
}

}  // namespace pk
}  // namespace crispy

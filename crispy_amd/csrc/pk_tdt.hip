// pk_tdt.hip -- the greedy TDT decoding loop of Parakeet for MI355X (gfx950) in exact f32: the LSTM prediction network, the joint
// head with its two arg-maxes and the per-clip advance (include/crispy_hip.h, "Parakeet TDT decoder"; host side pk_tdt_api.cpp).
//
// All three matrix products are skinny -- up to 4096 clips by a [K][N] matrix that is read once per 16 clips -- and run in one form:
// a workgroup of four waves owns 64 output columns and 16 clips; k goes through LDS in blocks of 128, of which wave w takes
// k 32 w ... 32 w + 31 in ascending order into one accumulator per clip, and the four waves' sums are added in wave order.  A
// column's sum therefore runs in an order that depends on K alone: not on the clip's row in the tile, not on the clip count.
// No workgroup reads the state of a clip outside its tile, and nothing a step decides leaves the device.
#include <climits>
#include <cmath>

#include "pk_internal.h"
#include "wave_ops.h"

namespace crispy {
namespace pk {
namespace {

constexpr int R = kTdtRows, NC = kTdtCols, KB = kTdtKBlock;

struct Tile {
  __attribute__((aligned(16))) float xs[KB][R];      // the inputs of one k block, [k][clip]: a wave reads one k of all clips as four b128
  float red[4][R][NC];                               // each wave's sums
  const float* xa[R];                                // per clip of the tile: where its inputs come from (NULL: takes no part)
  const float* xb[R];
};

// acc[r] of wave w = sum over its k of x[r][k] W[k][col0 + lane], left in s.red[w][r][lane]; loadx(r, k) is x[r][k]
template <class LoadX>
__device__ __forceinline__ void skinny_product(const float* __restrict__ W, int N, int K, int col0, LoadX loadx, Tile& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = 0.0f;
  const int kw = wave * (KB / 4);
  const float* wp = W + (size_t)kw * N + col0 + lane;
  const int fk = tid & (KB - 1), fr = (tid >> 7) * (R / 2);      // this thread fills k fk of clips fr ... fr + 7
  // A block's 32 weights of this lane are requested one block ahead, so that the requests of two blocks are in flight while one is
  // multiplied: the launch has few waves (640 for an LSTM layer on 64 clips) and is paced by how many bytes each keeps on the way.
  float w[KB / 4], wn[KB / 4];
#pragma unroll
  for (int kk = 0; kk < KB / 4; ++kk) w[kk] = wp[(size_t)kk * N];
  for (int k0 = 0; k0 < K; k0 += KB) {
    lds_barrier();      // the previous block's reads are over; only LDS is handed from wave to wave
    float v[R / 2];
#pragma unroll
    for (int r = 0; r < R / 2; ++r) v[r] = loadx(fr + r, k0 + fk);
    if (k0 + KB < K) {
#pragma unroll
      for (int kk = 0; kk < KB / 4; ++kk) wn[kk] = wp[(size_t)(k0 + KB + kk) * N];
    }
    *reinterpret_cast<float4*>(&s.xs[fk][fr]) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(&s.xs[fk][fr + 4]) = make_float4(v[4], v[5], v[6], v[7]);
    lds_barrier();
#pragma unroll
    for (int kk = 0; kk < KB / 4; ++kk) {
      const float4* x = reinterpret_cast<const float4*>(s.xs[kw + kk]);
#pragma unroll
      for (int q = 0; q < R / 4; ++q) {
        const float4 xv = x[q];
        acc[4 * q] = fmaf(xv.x, w[kk], acc[4 * q]);
        acc[4 * q + 1] = fmaf(xv.y, w[kk], acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(xv.z, w[kk], acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(xv.w, w[kk], acc[4 * q + 3]);
      }
    }
#pragma unroll
    for (int kk = 0; kk < KB / 4; ++kk) w[kk] = wn[kk];
  }
#pragma unroll
  for (int r = 0; r < R; ++r) s.red[wave][r][lane] = acc[r];
  lds_barrier();
}

__device__ __forceinline__ float waves_sum(const Tile& s, int r, int col) {
  return ((s.red[0][r][col] + s.red[1][r][col]) + s.red[2][r][col]) + s.red[3][r][col];
}

__device__ __forceinline__ bool tile_idle(const Tile& s) {
  bool any = false;
#pragma unroll
  for (int r = 0; r < R; ++r) any |= s.xa[r] != nullptr;
  return !any;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ void tdt_init_kernel(TdtState d, int blank) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.n_clips) return;
  const long budget = d.step_off[c + 1] - d.step_off[c];
  const int fin = budget <= 0;
  d.t[c] = 0;
  d.tok[c] = blank;
  d.budget[c] = (int)budget;
  d.done[c] = fin;
  d.run[c] = !fin;
  d.n_steps[c] = 0;
  if (fin) atomicAdd(d.finished, 1);
}

// LSTM layer `layer` on the clips whose run flag is set: gates = [x ; h] W + b, c = f c + i g, hn = o tanh(c).  x is the embedding
// of the clip's token (layer 0) or the layer below's hn of this step.  The new h goes to hn because other workgroups of this launch
// still read h; the launch that reads hn next (the layer above or the projector) commits it to h, where nobody in that launch reads it.
__global__ __launch_bounds__(256) void tdt_lstm_kernel(TdtState d, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* __restrict__ emb, int D, int layer) {
  __shared__ Tile s;
  if (*d.finished >= d.n_clips) return;
  const int tid = threadIdx.x, clip0 = blockIdx.y * R, col0 = blockIdx.x * NC, n = d.n_clips;
  if (tid < R) {
    const int c = clip0 + tid;
    const bool on = c < n && d.run[c] != 0;
    s.xa[tid] = !on ? nullptr : layer == 0 ? emb + (size_t)d.tok[c] * D : d.hn + ((size_t)(layer - 1) * n + c) * D;
    s.xb[tid] = !on ? nullptr : d.h + ((size_t)layer * n + c) * D;
  }
  __syncthreads();
  if (tile_idle(s)) return;
  skinny_product(W, 4 * D, 2 * D, col0, [&](int r, int k) -> float {
    const float* src = k < D ? s.xa[r] : s.xb[r];      // uniform over a k block: D is a multiple of it
    return src ? src[k < D ? k : k - D] : 0.0f;
  }, s);
  const int r = tid >> 4, u = tid & 15, c = clip0 + r;
  if (s.xa[r] == nullptr) return;
  const int j = col0 / 4 + u;      // the unit
  const float gi = waves_sum(s, r, 4 * u) + bias[col0 + 4 * u], gf = waves_sum(s, r, 4 * u + 1) + bias[col0 + 4 * u + 1],
              gg = waves_sum(s, r, 4 * u + 2) + bias[col0 + 4 * u + 2], go = waves_sum(s, r, 4 * u + 3) + bias[col0 + 4 * u + 3];
  const size_t at = ((size_t)layer * n + c) * D + j;
  const float cell = fmaf(sigmoidf(gf), d.c[at], sigmoidf(gi) * tanhf(gg));
  d.c[at] = cell;
  d.hn[at] = sigmoidf(go) * tanhf(cell);
  if (layer > 0) {
    const size_t below = ((size_t)(layer - 1) * n + c) * D + j;
    d.h[below] = d.hn[below];
  }
}

// g = decoder_projector(hn of the last layer) on the same clips; commits the last layer's h
__global__ __launch_bounds__(256) void tdt_dproj_kernel(TdtState d, const float* __restrict__ W, const float* __restrict__ bias, int D, int L) {
  __shared__ Tile s;
  if (*d.finished >= d.n_clips) return;
  const int tid = threadIdx.x, clip0 = blockIdx.y * R, col0 = blockIdx.x * NC, n = d.n_clips;
  if (tid < R) {
    const int c = clip0 + tid;
    s.xa[tid] = c < n && d.run[c] != 0 ? d.hn + ((size_t)(L - 1) * n + c) * D : nullptr;
  }
  __syncthreads();
  if (tile_idle(s)) return;
  skinny_product(W, D, D, col0, [&](int r, int k) -> float { return s.xa[r] ? s.xa[r][k] : 0.0f; }, s);
  const int col = tid & 63;
#pragma unroll
  for (int i = 0; i < R / 4; ++i) {
    const int r = (tid >> 6) * (R / 4) + i, c = clip0 + r;
    if (s.xa[r] == nullptr) continue;
    d.g[(size_t)c * D + col0 + col] = waves_sum(s, r, col) + bias[col0 + col];
    const size_t at = ((size_t)(L - 1) * n + c) * D + col0 + col;
    d.h[at] = d.hn[at];
  }
}

// logits = relu(p[t] + g) head + bias on the unfinished clips: the tap row of this step, the duration logits, and the largest token
// logit of this workgroup's 64 columns with its column (the lowest on a tie)
__global__ __launch_bounds__(256) void tdt_joint_kernel(TdtState d, const float* __restrict__ W, const float* __restrict__ bias, int D, int V,
                                                        int n_dur, int n_pad) {
  __shared__ Tile s;
  if (*d.finished >= d.n_clips) return;
  const int tid = threadIdx.x, clip0 = blockIdx.y * R, col0 = blockIdx.x * NC, n = d.n_clips;
  if (tid < R) {
    const int c = clip0 + tid;
    const bool on = c < n && d.done[c] == 0;
    s.xa[tid] = on ? d.p + ((size_t)d.off[c] + d.t[c]) * D : nullptr;
    s.xb[tid] = on ? d.g + (size_t)c * D : nullptr;
  }
  __syncthreads();
  if (tile_idle(s)) return;
  skinny_product(W, n_pad, D, col0, [&](int r, int k) -> float { return s.xa[r] ? fmaxf(s.xa[r][k] + s.xb[r][k], 0.0f) : 0.0f; }, s);
  float (*logit)[NC] = reinterpret_cast<float (*)[NC]>(&s.xs[0][0]);      // [R][64] over the input block: every wave is past its reads
  const int col = tid & 63, width = V + n_dur;
#pragma unroll
  for (int i = 0; i < R / 4; ++i) {
    const int r = (tid >> 6) * (R / 4) + i, c = clip0 + r;
    if (s.xa[r] == nullptr) continue;
    const float v = waves_sum(s, r, col) + bias[col0 + col];
    logit[r][col] = v;
    const int o = col0 + col;
    if (o < width && d.logits_tap) d.logits_tap[(size_t)(d.step_off[c] + d.n_steps[c]) * width + o] = v;
    if (o >= V && o < width) d.dur_logit[(size_t)c * kTdtMaxDurations + (o - V)] = v;
  }
  __syncthreads();
  if (tid < R && s.xa[tid] != nullptr) {
    float best = -INFINITY;
    int at = INT_MAX;
    const int cols = min(NC, V - col0);      // token columns of this tile; <= 0 behind the vocabulary
    for (int q = 0; q < cols; ++q) {
      const float v = logit[tid][q];
      if (v > best || at == INT_MAX) {
        best = v;
        at = col0 + q;
      }
    }
    d.part_val[(size_t)(clip0 + tid) * d.tiles + blockIdx.x] = best;
    d.part_idx[(size_t)(clip0 + tid) * d.tiles + blockIdx.x] = at;
  }
}

__device__ __forceinline__ bool better(float v, int i, float best, int at) { return i != INT_MAX && (at == INT_MAX || v > best || (v == best && i < at)); }

// One wave per unfinished clip: the token arg-max over the column tiles in index order, the duration arg-max, the duration rule, the
// step log, the frame pointer, the next input token and the flags.
__global__ __launch_bounds__(64) void tdt_advance_kernel(TdtState d, TdtModel m) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (d.done[c]) return;
  float best = -INFINITY;
  int at = INT_MAX;
  for (int tile = lane; tile < d.tiles; tile += 64) {
    const float v = d.part_val[(size_t)c * d.tiles + tile];
    const int i = d.part_idx[(size_t)c * d.tiles + tile];
    if (better(v, i, best, at)) {
      best = v;
      at = i;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float v = __shfl_xor(best, o, 64);
    const int i = __shfl_xor(at, o, 64);
    if (better(v, i, best, at)) {
      best = v;
      at = i;
    }
  }
  if (lane != 0) return;
  const int k = at == INT_MAX ? m.blank : at;
  int di = 0;
  float dv = d.dur_logit[(size_t)c * kTdtMaxDurations];
  for (int q = 1; q < m.n_dur; ++q) {
    const float v = d.dur_logit[(size_t)c * kTdtMaxDurations + q];
    if (v > dv) {
      dv = v;
      di = q;
    }
  }
  int dur = m.dur[di];
  if (k == m.blank && dur == 0) dur = 1;
  const int t = d.t[c], frames = d.off[c + 1] - d.off[c];
  int* row = d.steps + (size_t)(d.step_off[c] + d.n_steps[c]) * 3;
  row[0] = k;
  row[1] = t;
  row[2] = dur;
  d.n_steps[c] += 1;
  d.t[c] = t + dur;
  const int left = d.budget[c] - 1;
  d.budget[c] = left;
  const bool fin = t + dur >= frames || left <= 0;
  d.tok[c] = k;
  d.run[c] = k != m.blank && !fin;
  if (fin) {
    d.done[c] = 1;
    atomicAdd(d.finished, 1);
  }
}

}  // namespace

hipError_t launch_tdt_init(const TdtModel& m, const TdtState& s, hipStream_t st) {
  const size_t state = (size_t)m.L * s.n_clips * m.D * sizeof(float);
  hipError_t e = hipMemsetAsync(s.finished, 0, sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(s.h, 0, state, st);
  if (e == hipSuccess) e = hipMemsetAsync(s.c, 0, state, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tdt_init_kernel, dim3((s.n_clips + 255) / 256), dim3(256), 0, st, s, m.blank);
  return hipGetLastError();
}

hipError_t launch_tdt_predict(const TdtModel& m, const TdtState& s, hipStream_t st) {
  const unsigned row_tiles = (s.n_clips + kTdtRows - 1) / kTdtRows;
  for (int l = 0; l < m.L; ++l)
    hipLaunchKernelGGL(tdt_lstm_kernel, dim3(4 * m.D / kTdtCols, row_tiles), dim3(256), 0, st, s, m.lstm_w[l], m.lstm_b[l], m.emb, m.D, l);
  hipLaunchKernelGGL(tdt_dproj_kernel, dim3(m.D / kTdtCols, row_tiles), dim3(256), 0, st, s, m.dp_w, m.dp_b, m.D, m.L);
  return hipGetLastError();
}

hipError_t launch_tdt_joint(const TdtModel& m, const TdtState& s, hipStream_t st) {
  const unsigned row_tiles = (s.n_clips + kTdtRows - 1) / kTdtRows;
  hipLaunchKernelGGL(tdt_joint_kernel, dim3(s.tiles, row_tiles), dim3(256), 0, st, s, m.head_w, m.head_b, m.D, m.V, m.n_dur, m.n_pad);
  return hipGetLastError();
}

hipError_t launch_tdt_advance(const TdtModel& m, const TdtState& s, hipStream_t st) {
  hipLaunchKernelGGL(tdt_advance_kernel, dim3(s.n_clips), dim3(64), 0, st, s, m);
  return hipGetLastError();
}

}  // namespace pk
}  // namespace crispy

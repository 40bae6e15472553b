// whisper_align.hip -- word-level timestamps from cross-attention alignment (crispy_asr_opts::dtw_token_timestamps):
// openai-whisper's word_timestamps=True (timing.py: find_alignment), whisper.cpp's dtw_token_timestamps [UPSTREAM-RECALL].
// For the diarization path, which gives every word to a speaker by its midpoint (managers/diarization.rs:656-700,
// format_diarized_text) from TranscriptionManager::transcribe_with_timestamps (managers/transcription.rs:200-249).
//
// Per round of the seek loop, for every clip whose window kept text:
//   1. ONE teacher-forced prefill (decode_steps.cpp: prefill) over sot sequence + <|notimestamps|> + the text tokens +
//      <|endoftext|> of all such clips, left-padded as decode_ts pads; its own cross K|V of the window (a best-of pass may
//      have left another clip set's there).  layer_cross_and_mlp copies the cross-q rows of the alignment layers aside
//      (AlignWs) -- exactly the rows the layer's own cross-attention multiplies.
//   2. align_rowstats_kernel: per (clip, head) the soft-max maximum and sum of every row over the first F = n_frames / 2
//      keys (cropped BEFORE the soft-max, openai's order); the head's K is read once per workgroup.
//   3. align_matrix_kernel: per (clip, tile of 32 frames + 3 on each side) the scores again, normalised by the row
//      statistics, standardised per frame over the rows (population std), the 7-wide median along the frames (reflect
//      padding at both ends of the cropped range), the mean over the heads.  Only the [rows][F] matrix reaches HBM.
//   4. align_dtw_kernel: one workgroup per clip, DTW on minus the matrix rows of <|notimestamps|> and the text tokens, one
//      anti-diagonal per step (a thread per row, the two last diagonals in LDS, the trace at 2 bits per cell in LDS), one
//      lane walks the backtrace and records where the path enters every row.
// Nothing reduces across clips: a clip's alignment is its own whatever the batch.
#include "whisper_internal.h"
#include "wave_ops.h"

namespace crispy {
namespace asr {
namespace {

constexpr int kHd = 64;                 // head width of every Whisper model
constexpr int kTile = 32;               // output frames per matrix workgroup
constexpr int kHalo = 3;                // the median filter's half width
constexpr int kSpan = kTile + 2 * kHalo;
constexpr int kDtwMaxRows = kAlignDtwMaxRows;

// Per-clip arguments of the three kernels (device array [batch]).
struct AlignClip {
  int off;          // first token row of the clip in the padded pass (q rows [off, n_rows))
  int rows;         // token rows R
  int n_keys;       // F = n_frames / 2
  int row0;         // first matrix row the DTW reads (n_sot)
  int dtw_rows;     // R - n_sot - 1
};

struct AlignArgs {
  const float* q;           // AlignWs::q
  long q_slot_stride;       // clips x rows x dt
  long q_clip_stride;       // rows x dt
  int dt;
  const void* kv;           // cross K|V of all layers: f32 (mode 0) or f16
  int kv16;                 // 1: f16 K
  int q16;                  // 1: q rounded to f16 inside the attention (precision mode 2)
  long kv_layer_stride;     // elements: clips x Tn x 2 dt
  long kv_clip_stride;      // Tn x 2 dt
  int Tn;
  const int2* heads;        // [n_heads] (slot of the layer in q, head)
  const int* head_layer;    // [n_heads] decoder layer
  int n_heads;
  const AlignClip* clips;
  float2* stats;            // [batch][n_heads][n_rows] (max, sum)
  int n_rows;               // padded rows of the pass
  float* matrix;            // [batch][ld_rows][ld_f]
  float* probs;             // nullable [batch][n_heads][ld_rows][ld_f]
  int ld_rows, ld_f;
};

// one cross-attention score: q . k / 8, the products in dimension order (the row statistics and the matrix kernel call
// the same function, so a score has the same bits in both)
__device__ __forceinline__ float score(const float (&q)[kHd], const float* __restrict__ k) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < kHd; d += 4) {
    const float4 kk = *reinterpret_cast<const float4*>(k + d);
    acc = fmaf(q[d], kk.x, acc);
    acc = fmaf(q[d + 1], kk.y, acc);
    acc = fmaf(q[d + 2], kk.z, acc);
    acc = fmaf(q[d + 3], kk.w, acc);
  }
  return acc * 0.125f;
}

__device__ __forceinline__ void load_q(const AlignArgs& a, int b, int hh, int r, float (&q)[kHd]) {
  const AlignClip c = a.clips[b];
  const int2 hd = a.heads[hh];
  const float* src = a.q + hd.x * a.q_slot_stride + b * a.q_clip_stride + (long)(c.off + r) * a.dt + hd.y * kHd;
#pragma unroll
  for (int d = 0; d < kHd; d += 4) {
    const float4 v = *reinterpret_cast<const float4*>(src + d);
    q[d] = v.x; q[d + 1] = v.y; q[d + 2] = v.z; q[d + 3] = v.w;
  }
  if (a.q16) {
#pragma unroll
    for (int d = 0; d < kHd; ++d) q[d] = (float)(_Float16)q[d];
  }
}

// K row `key` of head hh of clip b into LDS (64 floats), by 16 threads of 4 floats each
__device__ __forceinline__ void stage_k(const AlignArgs& a, int b, int hh, int key, int part, float* dst) {
  const long base = (long)a.head_layer[hh] * a.kv_layer_stride + b * a.kv_clip_stride + (long)a.heads[hh].y * a.Tn * kHd +
                    (long)key * kHd + part * 4;
  float4 v;
  if (a.kv16) {
    const _Float16* k = reinterpret_cast<const _Float16*>(a.kv) + base;
    v = make_float4((float)k[0], (float)k[1], (float)k[2], (float)k[3]);
  } else {
    v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(a.kv) + base);
  }
  *reinterpret_cast<float4*>(dst + part * 4) = v;
}

// grid (n_heads, batch), 256 threads: thread = token row (rows beyond 256 in further passes); the keys in tiles of 64
// through LDS.  Online soft-max statistics over the first F keys.
__global__ __launch_bounds__(256) void align_rowstats_kernel(AlignArgs a) {
  __shared__ __attribute__((aligned(16))) float ks[64 * kHd];
  const int hh = blockIdx.x, b = blockIdx.y;
  const AlignClip c = a.clips[b];
  for (int r0 = 0; r0 < c.rows; r0 += 256) {
    const int r = r0 + threadIdx.x;
    const bool live = r < c.rows;
    float q[kHd];
    if (live) load_q(a, b, hh, r, q);
    else
      for (int d = 0; d < kHd; ++d) q[d] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < c.n_keys; k0 += 64) {
      const int nk = min(64, c.n_keys - k0);
      lds_barrier();
      for (int e = threadIdx.x; e < nk * 16; e += 256) stage_k(a, b, hh, k0 + e / 16, e % 16, ks + (e / 16) * kHd);
      lds_barrier();
      if (live) {
        for (int k = 0; k < nk; ++k) {
          const float s = score(q, ks + k * kHd);
          if (s > m) { l = l * expf(m - s) + 1.f; m = s; }
          else l += expf(s - m);
        }
      }
    }
    if (live) a.stats[((long)b * a.n_heads + hh) * a.n_rows + r] = make_float2(m, l);
  }
}

__device__ __forceinline__ void cswap(float& x, float& y) {
  const float lo = fminf(x, y), hi = fmaxf(x, y);
  x = lo; y = hi;
}

// the middle of 7 values: a 16-comparator sorting network in registers
__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5, float v6) {
  cswap(v0, v6); cswap(v2, v3); cswap(v4, v5);
  cswap(v0, v2); cswap(v1, v4); cswap(v3, v6);
  cswap(v0, v1); cswap(v2, v5); cswap(v3, v4);
  cswap(v1, v2); cswap(v4, v6);
  cswap(v2, v3); cswap(v4, v5);
  cswap(v1, v2); cswap(v3, v4); cswap(v5, v6);
  return v3;
}

// grid (frame tiles, batch), 256 threads; dynamic LDS: K [kSpan][64], P [R][kSpan], acc [R][kTile], column mean / std.
__global__ __launch_bounds__(256) void align_matrix_kernel(AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int b = blockIdx.y;
  const AlignClip c = a.clips[b];
  const int F = c.n_keys, R = c.rows, f0 = blockIdx.x * kTile;
  if (f0 >= F) return;
  float* ks = sm;                                   // [kSpan][64]
  float* P = ks + kSpan * kHd;                      // [R][kSpan]
  float* acc = P + (size_t)R * kSpan;               // [R][kTile]
  float* mu = acc + (size_t)R * kTile;              // [kSpan]
  float* sd = mu + kSpan;                           // [kSpan]
  for (int hh = 0; hh < a.n_heads; ++hh) {
    lds_barrier();                                  // the previous head's readers are done with ks / P / mu / sd
    for (int e = threadIdx.x; e < kSpan * 16; e += 256) {
      int g = f0 - kHalo + e / 16;                  // reflect padding of the cropped range (torch's mode="reflect")
      if (g < 0) g = -g;
      if (g >= F) g = 2 * (F - 1) - g;
      // a tile wider than the range (F < kSpan / 2) reflects past its other end: those columns feed no output (a median
      // of frame f < F reads frames up to f + 3), so they only need to stay inside the clip's keys
      g = min(max(g, 0), F - 1);
      stage_k(a, b, hh, g, e % 16, ks + (e / 16) * kHd);
    }
    lds_barrier();
    for (int r = threadIdx.x; r < R; r += 256) {
      float q[kHd];
      load_q(a, b, hh, r, q);
      const float2 st = a.stats[((long)b * a.n_heads + hh) * a.n_rows + r];
      float* prow = a.probs ? a.probs + (((long)b * a.n_heads + hh) * a.ld_rows + r) * a.ld_f : nullptr;
      for (int t = 0; t < kSpan; ++t) {
        const float p = expf(score(q, ks + t * kHd) - st.x) / st.y;
        P[r * kSpan + t] = p;
        const int f = f0 - kHalo + t;
        if (prow && t >= kHalo && t < kHalo + kTile && f < F) prow[f] = p;
      }
    }
    lds_barrier();
    if (threadIdx.x < kSpan) {                      // standardise every frame over the token rows
      const int t = threadIdx.x;
      float s = 0.f;
      for (int r = 0; r < R; ++r) s += P[r * kSpan + t];
      const float mean = s / (float)R;
      float v = 0.f;
      for (int r = 0; r < R; ++r) { const float d = P[r * kSpan + t] - mean; v = fmaf(d, d, v); }
      mu[t] = mean;
      sd[t] = sqrtf(v / (float)R);
    }
    lds_barrier();
    for (int e = threadIdx.x; e < R * kTile; e += 256) {
      const int r = e / kTile, u = e % kTile;
      const float* pr = P + r * kSpan + u;
      float z[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) z[k] = (pr[k] - mu[u + k]) / sd[u + k];
      const float med = median7(z[0], z[1], z[2], z[3], z[4], z[5], z[6]);
      acc[e] = hh == 0 ? med : acc[e] + med;
    }
  }
  lds_barrier();
  for (int e = threadIdx.x; e < R * kTile; e += 256) {
    const int r = e / kTile, u = e % kTile, f = f0 + u;
    if (f < F) a.matrix[((long)b * a.ld_rows + r) * a.ld_f + f] = acc[e] / (float)a.n_heads;
  }
}

struct DtwArgs {
  const float* x;           // cost source: x[b * clip_stride + (row0 + i) * ld + j]
  long clip_stride, ld;
  const AlignClip* clips;   // row0 = first row, dtw_rows = N, n_keys = M
  int negate;               // 1: DTW on -x (the alignment matrix)
  int* jumps;               // [batch][ld_jumps]: entry column of every row, rows 0 .. N - 1 (the first N jumps)
  int ld_jumps;
  int* path;                // nullable [batch][2][N + M]: (row, column) pairs in BACKWARD order
  long ld_path;
  int* n_path;              // nullable [batch]
};

// One workgroup per clip.  Step s = i + j of the 1-based cost array: row i's thread computes cost[i][s - i] from
// cost[i-1][j-1] (what it read from row i-1 one step earlier), cost[i-1][j] (row i-1's value of the previous step, LDS)
// and cost[i][j-1] (its own register).  openai's dtw_cpu: cost[0][0] = 0, inf elsewhere on the border, the f32 sum of x
// and the chosen predecessor; ties: diagonal only when strictly below both, up only when strictly below both, else left.
// x is requested 8 steps ahead of its use.
__global__ __launch_bounds__(kDtwMaxRows) void align_dtw_kernel(DtwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned dsm[];
  const int b = blockIdx.x;
  const AlignClip c = a.clips[b];
  const int N = c.dtw_rows, M = c.n_keys, W = (M + 15) / 16;
  unsigned* trace = dsm;                                          // [N][W]: 16 cells of a row per word
  float* diag = reinterpret_cast<float*>(dsm + (size_t)N * W);    // [2][kDtwMaxRows]
  int* jb = reinterpret_cast<int*>(diag + 2 * kDtwMaxRows);       // [N + M]: entry columns, backward
  const int i = threadIdx.x + 1;
  const bool active = i <= N;
  const float* xrow = a.x + b * a.clip_stride + (long)(c.row0 + (active ? i : 1) - 1) * a.ld - 1;   // xrow[j] = x[i-1][j-1]
  const float sign = a.negate ? -1.f : 1.f;
  float xr[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int j = 2 + u - i;
    xr[u] = active && j >= 1 && j <= M ? xrow[j] : 0.f;
  }
  float left = INFINITY, upl = INFINITY;
  unsigned tw = 0;
  for (int s0 = 2; s0 <= N + M; s0 += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int s = s0 + u, j = s - i;
      const float xv = xr[u];
      {
        const int jn = j + 8;
        xr[u] = active && jn >= 1 && jn <= M ? xrow[jn] : 0.f;
      }
      if (active && j >= 1 && j <= M) {
        float c0, c1;
        if (i == 1) { c0 = j == 1 ? 0.f : INFINITY; c1 = INFINITY; }
        else { c1 = diag[((s - 1) & 1) * kDtwMaxRows + i - 2]; c0 = j == 1 ? INFINITY : upl; }
        const float c2 = j == 1 ? INFINITY : left;
        upl = c1;
        float cm;
        unsigned t;
        if (c0 < c1 && c0 < c2) { cm = c0; t = 0; }
        else if (c1 < c0 && c1 < c2) { cm = c1; t = 1; }
        else { cm = c2; t = 2; }
        const float cost = sign * xv + cm;
        left = cost;
        diag[(s & 1) * kDtwMaxRows + i - 1] = cost;
        tw |= t << (2 * ((j - 1) & 15));
        if (((j - 1) & 15) == 15 || j == M) { trace[(size_t)(i - 1) * W + (j - 1) / 16] = tw; tw = 0; }
      }
      lds_barrier();
    }
  }
  __shared__ int n_jb;
  if (threadIdx.x == 0) {
    // openai's backtrace: trace[0][:] = left, trace[:][0] = up; a path position is a jump where its row differs from the
    // position before it (and the first position is one) -- walking backwards, where the next cell is in another row
    int ii = N, jj = M, n = 0, nj = 0;
    while (ii > 0 || jj > 0) {
      if (a.path) {
        a.path[b * a.ld_path + n] = ii - 1;
        a.path[b * a.ld_path + (N + M) + n] = jj - 1;
      }
      ++n;
      unsigned t;
      if (ii == 0) t = 2;
      else if (jj == 0) t = 1;
      else t = (trace[(size_t)(ii - 1) * W + (jj - 1) / 16] >> (2 * ((jj - 1) & 15))) & 3u;
      const int ci = ii, cj = jj;
      if (t == 0) { --ii; --jj; }
      else if (t == 1) --ii;
      else --jj;
      if (ii != ci || (ii == 0 && jj == 0)) jb[nj++] = cj - 1;
    }
    n_jb = nj;
    if (a.n_path) a.n_path[b] = n;
  }
  lds_barrier();
  const int nj = n_jb;
  for (int k = threadIdx.x; k < N && k < nj; k += blockDim.x) a.jumps[b * a.ld_jumps + k] = jb[nj - 1 - k];
}

// dynamic LDS above the default 64 KB: the attribute belongs to the current device's copy of the kernel and is set to
// the size of this launch (the two kernels' sizes depend on the rows and frames of the call)
hipError_t lds_limit(const void* fn, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

size_t matrix_lds(int R) { return ((size_t)kSpan * kHd + (size_t)R * kSpan + (size_t)R * kTile + 2 * kSpan) * sizeof(float); }
size_t dtw_lds(int N, int M) { return ((size_t)N * ((M + 15) / 16) + 2 * kDtwMaxRows + (size_t)(N + M)) * 4; }

// device workspace of the alignment: grown on demand, carved in 256-byte pieces
struct Carve {
  char* p;
  size_t used = 0;
  template <class T> T* take(size_t n) {
    T* r = reinterpret_cast<T*>(p + used);
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};

int resolve_heads(const crispy_asr* h, const int* heads, int n_heads, std::vector<int>& out) {
  const int L = h->hp.n_text_layer, H = h->hp.n_text_head;
  out.clear();
  if (!heads) {
    if (n_heads != 0) return fail(CRISPY_ERR_INVALID_ARG, "alignment heads: NULL list of %d heads", n_heads);
    for (int l = L / 2; l < L; ++l)                // openai's default alignment_heads: the last half of the layers
      for (int hd = 0; hd < H; ++hd) { out.push_back(l); out.push_back(hd); }
    return CRISPY_OK;
  }
  if (n_heads <= 0) return fail(CRISPY_ERR_INVALID_ARG, "alignment heads: %d heads", n_heads);
  for (int k = 0; k < n_heads; ++k) {
    const int l = heads[2 * k], hd = heads[2 * k + 1];
    if (l < 0 || l >= L || hd < 0 || hd >= H)
      return fail(CRISPY_ERR_INVALID_ARG, "alignment head (%d, %d) outside %d layers x %d heads", l, hd, L, H);
    out.push_back(l); out.push_back(hd);
  }
  return CRISPY_OK;
}

// The whole alignment of `batch` clips: prefill, row statistics, matrix, DTW.  rows[b] = clip b's token rows; heads =
// resolved (layer, head) pairs.  d_probs / d_matrix_out: the stage entry point's optional outputs ([batch][n_heads][ld_rows]
// [ld_f] / [batch][ld_rows][ld_f]); time_idx receives the first N entry columns per clip.  logp (nullable; crispy_asr_set_confidence):
// the same prefill also projects its rows onto the vocabulary and leaves every text token's log-probability (conf_begin).
int run_alignment(crispy_asr* h, const float* d_enc, const std::vector<std::vector<int>>& rows, int n_sot, const std::vector<int>& n_frames,
                  const std::vector<int>& heads, float* d_probs, float* d_matrix_out, int ld_rows, std::vector<std::vector<int>>* time_idx,
                  std::vector<std::vector<float>>* logp = nullptr) {
  const int batch = (int)rows.size();
  if (batch == 0) return CRISPY_OK;
  // Tn: keys per clip of the cross K | V the prefill builds (the handle's audio context); Tm: the model's own -- the bound of
  // n_frames / 2 and the leading dimension of d_probs / d_matrix, which does not move with the setting
  const int dt = h->hp.n_text_state, Tn = h->audio_ctx, Tm = h->hp.n_audio_ctx, L = h->hp.n_text_layer, C = h->hp.n_text_ctx;
  auto keys_of = [&](int b) { return std::min(n_frames[b] / 2, Tn); };      // F: the frames a clip is aligned over
  if (dt % kHd != 0) return fail(CRISPY_ERR_UNSUPPORTED, "alignment: n_text_state %d is not whole 64-wide heads", dt);
  int n_rows = 0;
  for (int b = 0; b < batch; ++b) {
    const int R = (int)rows[b].size();
    if (R < n_sot + 2 || R > C) return fail(CRISPY_ERR_INVALID_ARG, "alignment: clip %d has %d token rows (%d ... %d)", b, R, n_sot + 2, C);
    for (int t : rows[b])
      if (t < 0 || t >= h->hp.n_vocab) return fail(CRISPY_ERR_INVALID_ARG, "alignment: token %d out of range", t);
    const int F = keys_of(b);
    if (F < 4 || n_frames[b] / 2 > Tm)
      return fail(CRISPY_ERR_INVALID_ARG, "alignment: clip %d has %d frames over %d keys (8 ... %d frames, >= 4 keys)", b, n_frames[b], Tn, 2 * Tm);
    const int N = R - n_sot - 1;
    if (!align_dtw_fits(N, F))
      return fail(CRISPY_ERR_UNSUPPORTED, "alignment: %d x %d DTW cells exceed the LDS trace", N, F);
    n_rows = std::max(n_rows, R);
  }
  if (ld_rows < n_rows) return fail(CRISPY_ERR_INVALID_ARG, "alignment: ld_tokens %d < %d rows", ld_rows, n_rows);
  const int n_heads = (int)heads.size() / 2;
  if (matrix_lds(n_rows) > 160 * 1024) return fail(CRISPY_ERR_UNSUPPORTED, "alignment: %d token rows exceed the matrix kernel's LDS", n_rows);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  AlignWs& A = h->align;
  // layers with an alignment head -> slots of the q buffer
  A.slot.assign((size_t)L, -1);
  int n_slots = 0;
  for (int k = 0; k < n_heads; ++k)
    if (A.slot[heads[2 * k]] < 0) A.slot[heads[2 * k]] = n_slots++;
  HIP_TRY(A.q.grow((size_t)n_slots * batch * n_rows * dt * sizeof(float)));
  const int ld_f = Tm;
  int max_n = 0;
  for (int b = 0; b < batch; ++b) max_n = std::max(max_n, (int)rows[b].size() - n_sot - 1 + keys_of(b));
  const size_t need = 256 * 8 + (size_t)batch * n_heads * n_rows * sizeof(float2) + (d_matrix_out ? 0 : (size_t)batch * ld_rows * ld_f * sizeof(float)) +
                      (size_t)batch * n_rows * sizeof(int) + (size_t)batch * sizeof(AlignClip) + (size_t)n_heads * (sizeof(int2) + sizeof(int));
  HIP_TRY(A.ws.grow(need));
  Carve cv{A.ws.as<char>()};
  float2* d_stats = cv.take<float2>((size_t)batch * n_heads * n_rows);
  float* d_matrix = d_matrix_out ? d_matrix_out : cv.take<float>((size_t)batch * ld_rows * ld_f);
  int* d_jumps = cv.take<int>((size_t)batch * n_rows);
  AlignClip* d_clips = cv.take<AlignClip>((size_t)batch);
  int2* d_heads = cv.take<int2>((size_t)n_heads);
  int* d_head_layer = cv.take<int>((size_t)n_heads);
  std::vector<AlignClip> hc((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    const int R = (int)rows[b].size();
    hc[b] = AlignClip{n_rows - R, R, keys_of(b), n_sot, R - n_sot - 1};      // (the left padding begin_pass gives the row)
  }
  std::vector<int2> hh((size_t)n_heads);
  std::vector<int> hl((size_t)n_heads);
  for (int k = 0; k < n_heads; ++k) { hh[k] = make_int2(A.slot[heads[2 * k]], heads[2 * k + 1]); hl[k] = heads[2 * k]; }
  HIP_TRY(hipMemcpyAsync(d_clips, hc.data(), sizeof(AlignClip) * batch, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_heads, hh.data(), sizeof(int2) * n_heads, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_head_layer, hl.data(), sizeof(int) * n_heads, hipMemcpyHostToDevice, s));
  // the pass: decode_ts's left padding, one cross K|V per clip (the window's own), a fixed key bound (not the batch's
  // longest row: a clip's arithmetic must not depend on its neighbours).  Its wait for the row offsets is the wait for
  // the three uploads above too.
  PassStart ps;
  int rc = begin_pass(h, "alignment:", rows, 1, 0, C, true, &ps);
  if (rc != CRISPY_OK) {
    (void)hipStreamSynchronize(s);      // the uploads above read host vectors of this frame
    return rc;
  }
  std::vector<int> row_len((size_t)batch);
  for (int b = 0; b < batch; ++b) row_len[b] = (int)rows[b].size();
  if (logp && (rc = conf_begin(h, ps.tok_mat.data(), batch, n_rows, row_len.data(), n_sot, s)) != CRISPY_OK) return rc;
  {
    struct Guard { crispy_asr* h; ~Guard() { h->align.on = false; h->align.rows = 0; conf_end(h); } } guard{h};
    A.rows = n_rows;
    A.on = true;
    int pos = 0;
    rc = prefill(h, ps.pass, d_enc, ps.tok_mat.data(), n_rows, s, &pos);
    if (rc != CRISPY_OK) return rc;
  }
  AlignArgs a{};
  a.q = A.q; a.q_clip_stride = (long)n_rows * dt; a.q_slot_stride = (long)batch * a.q_clip_stride; a.dt = dt;
  a.kv16 = h->enc_precision == 1 ? 1 : 0;
  a.kv = a.kv16 ? static_cast<const void*>(h->dw.xkv_h) : static_cast<const void*>(h->dw.xkv);
  a.q16 = h->dec_attn16 && h->enc_precision == 1 ? 1 : 0;
  a.kv_layer_stride = (long)batch * Tn * 2 * dt; a.kv_clip_stride = (long)Tn * 2 * dt; a.Tn = Tn;
  a.heads = d_heads; a.head_layer = d_head_layer; a.n_heads = n_heads; a.clips = d_clips;
  a.stats = d_stats; a.n_rows = n_rows; a.matrix = d_matrix; a.probs = d_probs; a.ld_rows = ld_rows; a.ld_f = ld_f;
  int max_f = 0;
  for (int b = 0; b < batch; ++b) max_f = std::max(max_f, keys_of(b));
  hipLaunchKernelGGL(align_rowstats_kernel, dim3(n_heads, batch), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(lds_limit(reinterpret_cast<const void*>(align_matrix_kernel), matrix_lds(n_rows)));
  hipLaunchKernelGGL(align_matrix_kernel, dim3((max_f + kTile - 1) / kTile, batch), dim3(256), matrix_lds(n_rows), s, a);
  HIP_TRY(hipGetLastError());
  if (time_idx) {
    int max_dtw = 0;
    for (int b = 0; b < batch; ++b) max_dtw = std::max(max_dtw, hc[b].dtw_rows);
    size_t lds = 0;
    for (int b = 0; b < batch; ++b) lds = std::max(lds, dtw_lds(hc[b].dtw_rows, hc[b].n_keys));
    DtwArgs d{};
    d.x = d_matrix; d.clip_stride = (long)ld_rows * ld_f; d.ld = ld_f; d.clips = d_clips; d.negate = 1;
    d.jumps = d_jumps; d.ld_jumps = n_rows;
    HIP_TRY(lds_limit(reinterpret_cast<const void*>(align_dtw_kernel), lds));
    hipLaunchKernelGGL(align_dtw_kernel, dim3(batch), dim3((max_dtw + 63) / 64 * 64), lds, s, d);
    HIP_TRY(hipGetLastError());
    std::vector<int> jumps((size_t)batch * n_rows);
    HIP_TRY(hipMemcpyAsync(jumps.data(), d_jumps, jumps.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    time_idx->assign((size_t)batch, {});
    for (int b = 0; b < batch; ++b)
      (*time_idx)[b].assign(jumps.begin() + (size_t)b * n_rows, jumps.begin() + (size_t)b * n_rows + hc[b].dtw_rows);
  }
  if (logp) return conf_read(h, batch, n_rows, row_len.data(), n_sot, s, logp);
  return CRISPY_OK;
}

int align_round(crispy_asr* h, const float* d_enc, const std::vector<std::vector<int>>& rows, int n_sot, const std::vector<int>& n_frames,
                const std::vector<int>& heads, std::vector<std::vector<int>>& time_idx, std::vector<std::vector<float>>* logp) {
  std::vector<int> hv;
  const int rc = resolve_heads(h, heads.empty() ? nullptr : heads.data(), (int)heads.size() / 2, hv);
  if (rc != CRISPY_OK) return rc;
  int ld = 0;
  for (const auto& r : rows) ld = std::max(ld, (int)r.size());
  return run_alignment(h, d_enc, rows, n_sot, n_frames, hv, nullptr, nullptr, ld, &time_idx, logp);
}

[[maybe_unused]] const bool kInstalled = (g_align_round = &align_round, true);

}  // namespace
}  // namespace asr
}  // namespace crispy

using namespace crispy;
using namespace crispy::asr;

extern "C" {

int crispy_asr_align_device(crispy_asr* h, const float* d_enc, int batch, const int* tokens, const int* n_tokens, int ld_tokens,
                            int n_sot, const int* n_frames, const int* heads, int n_heads, float* d_probs, float* d_matrix,
                            float* jump_times) try {
  if (!h || !d_enc || batch <= 0 || !tokens || !n_tokens || !n_frames || ld_tokens <= 0)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_align_device: NULL argument or empty batch");
  if (!h->finalized) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_align_device: model not finalized");
  if (n_sot < 1) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_align_device: n_sot %d", n_sot);
  std::vector<int> hv;
  int rc = resolve_heads(h, heads, n_heads, hv);
  if (rc != CRISPY_OK) return rc;
  std::vector<std::vector<int>> rows((size_t)batch);
  std::vector<int> nf(n_frames, n_frames + batch);
  for (int b = 0; b < batch; ++b) {
    if (n_tokens[b] < 0 || n_tokens[b] > ld_tokens) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_align_device: n_tokens[%d] = %d", b, n_tokens[b]);
    rows[b].assign(tokens + (size_t)b * ld_tokens, tokens + (size_t)b * ld_tokens + n_tokens[b]);
  }
  std::vector<std::vector<int>> ti;
  rc = run_alignment(h, d_enc, rows, n_sot, nf, hv, d_probs, d_matrix, ld_tokens, jump_times ? &ti : nullptr);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (jump_times)
    for (int b = 0; b < batch; ++b)
      for (size_t k = 0; k < ti[b].size(); ++k) jump_times[(size_t)b * ld_tokens + k] = (float)(ti[b][k] * 0.02);
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_align_device")

int crispy_asr_dtw_device(crispy_asr* h, const float* d_x, int n_rows, int n_cols, long ld, int* text_idx, int* time_idx,
                          int* n_path) try {
  if (!h || !d_x || !text_idx || !time_idx || !n_path) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_dtw_device: NULL argument");
  if (n_rows < 1 || n_cols < 1 || ld < n_cols) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_dtw_device: %d x %d, ld %ld", n_rows, n_cols, ld);
  if (!align_dtw_fits(n_rows, n_cols))
    return fail(CRISPY_ERR_UNSUPPORTED, "crispy_asr_dtw_device: %d x %d exceeds the LDS trace", n_rows, n_cols);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  AlignWs& A = h->align;
  const size_t L = (size_t)n_rows + n_cols;
  HIP_TRY(A.ws.grow(256 * 4 + L * 2 * sizeof(int) + (size_t)n_rows * sizeof(int) + sizeof(int) + sizeof(AlignClip)));
  Carve cv{A.ws.as<char>()};
  int* d_path = cv.take<int>(L * 2);
  int* d_jumps = cv.take<int>((size_t)n_rows);
  int* d_n = cv.take<int>(1);
  AlignClip* d_clip = cv.take<AlignClip>(1);
  const AlignClip hc{0, n_rows, n_cols, 0, n_rows};
  HIP_TRY(hipMemcpyAsync(d_clip, &hc, sizeof hc, hipMemcpyHostToDevice, s));
  HIP_TRY(lds_limit(reinterpret_cast<const void*>(align_dtw_kernel), dtw_lds(n_rows, n_cols)));
  DtwArgs d{};
  d.x = d_x; d.clip_stride = 0; d.ld = ld; d.clips = d_clip; d.negate = 0; d.jumps = d_jumps; d.ld_jumps = n_rows;
  d.path = d_path; d.ld_path = (long)L * 2; d.n_path = d_n;
  hipLaunchKernelGGL(align_dtw_kernel, dim3(1), dim3((n_rows + 63) / 64 * 64), dtw_lds(n_rows, n_cols), s, d);
  HIP_TRY(hipGetLastError());
  std::vector<int> path(L * 2);
  int n = 0;
  HIP_TRY(hipMemcpyAsync(path.data(), d_path, path.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (n < 0 || (size_t)n > L) return fail(CRISPY_ERR_HIP, "crispy_asr_dtw_device: path of %d cells", n);
  for (int k = 0; k < n; ++k) {          // the kernel walked backwards
    text_idx[k] = path[(size_t)(n - 1 - k)];
    time_idx[k] = path[L + (size_t)(n - 1 - k)];
  }
  *n_path = n;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_dtw_device")

}  // extern "C"

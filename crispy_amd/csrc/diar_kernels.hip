// diar_kernels.hip -- device side of the speaker clustering (include/crispy_hip.h, "Speaker clustering"): nme_sc of
// src-tauri/src/managers/diarization.rs:412-626.  Affinity, ranking and Laplacians reproduce the reference's f32
// arithmetic bit for bit, so nothing in this file may be contracted into a fused multiply-add: Rust does not fuse.
#pragma clang fp contract(off)

#include <cfloat>

#include "diar_internal.h"

namespace crispy {
namespace diar {
namespace {

// ---- affinity: cosine_similarity (:412-414, 613-626) of every pair ------------------------------------------------
// One thread per pair, 16 x 16 pairs per workgroup, the rows staged through LDS 64 dimensions at a time; each pair's
// three sums run over the dimensions in index order whatever the tiling.
constexpr int kAffT = 16, kAffD = 64;

__global__ __launch_bounds__(kAffT* kAffT) void affinity_kernel(const float* __restrict__ emb, int n, int dim,
                                                               float* __restrict__ aff) {
  __shared__ float sa[kAffT][kAffD + 1], sb[kAffT][kAffD + 1];
  const int tx = threadIdx.x % kAffT, ty = threadIdx.x / kAffT;
  const int i = blockIdx.y * kAffT + ty, j = blockIdx.x * kAffT + tx;
  float dot = 0.0f, na = 0.0f, nb = 0.0f;
  for (int d0 = 0; d0 < dim; d0 += kAffD) {
    const int nd = min(kAffD, dim - d0);
    for (int e = threadIdx.x; e < kAffT * kAffD; e += kAffT * kAffT) {
      const int r = e / kAffD, d = e % kAffD;
      const int ri = blockIdx.y * kAffT + r, rj = blockIdx.x * kAffT + r;
      sa[r][d] = (ri < n && d < nd) ? emb[(size_t)ri * dim + d0 + d] : 0.0f;
      sb[r][d] = (rj < n && d < nd) ? emb[(size_t)rj * dim + d0 + d] : 0.0f;
    }
    __syncthreads();
    for (int d = 0; d < nd; ++d) {
      const float x = sa[ty][d], y = sb[tx][d];
      dot += x * y;
      na += x * x;
      nb += y * y;
    }
    __syncthreads();
  }
  if (i >= n || j >= n) return;
  float sim = 0.0f;
  if (i != j) {
    float dist = 1.0f;
    if (!(na == 0.0f || nb == 0.0f)) dist = fmaxf(1.0f - dot / (sqrtf(na) * sqrtf(nb)), 0.0f);
    sim = fminf(fmaxf(1.0f - dist, 0.0f), 1.0f);
  }
  aff[(size_t)i * n + j] = sim;
}

__global__ void nonfinite_kernel(const float* __restrict__ x, size_t count, int* __restrict__ flag) {
  bool bad = false;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x)
    bad |= !isfinite(x[e]);
  if (bad) *flag = 1;
}

// ---- ranking (:426-434) -------------------------------------------------------------------------------------------
// rank[i][j]: how many j' != i a stable descending sort of row i puts before j.  One workgroup per row.
__global__ __launch_bounds__(256) void rank_kernel(const float* __restrict__ aff, int n, unsigned short* __restrict__ rank) {
  __shared__ float row[kMaxN];
  const int i = blockIdx.x;
  for (int j = threadIdx.x; j < n; j += blockDim.x) row[j] = aff[(size_t)i * n + j];
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    const float v = row[j];
    int cnt = 0;
    for (int o = 0; o < n; ++o) cnt += (o != i) & ((row[o] > v) | ((row[o] == v) & (o < j)));
    rank[(size_t)i * n + j] = (unsigned short)(j == i ? 0xFFFF : cnt);
  }
}
// sym[i][j] = min(rank[i][j], rank[j][i]): the edge survives the pruning to p neighbours and the symmetrisation by max
// (:437-443) exactly when sym < p, and then carries aff[i][j] (the affinity is symmetric and not negative).
__global__ void symrank_kernel(const unsigned short* __restrict__ rank, int n, unsigned short* __restrict__ sym) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n) return;
  const unsigned short a = rank[(size_t)i * n + j], b = rank[(size_t)j * n + i];
  sym[(size_t)i * n + j] = a < b ? a : b;
}

// ---- Laplacians (:444-453) ----------------------------------------------------------------------------------------
// Laplacian e of a launch has p = p0 + e.
// dinv[e][i] = 1 / sqrt(max(row sum, 1e-9)), the sum over ALL j in index order (pruned entries add 0.0); the thread of
// row i walks column i of the symmetric matrices, which the threads of a wave read side by side.
__global__ void dinv_kernel(const float* __restrict__ aff, const unsigned short* __restrict__ sym, int n, int p0,
                            float* __restrict__ dinv) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, e = blockIdx.y;
  if (i >= n) return;
  const int p = p0 + e;
  float sum = 0.0f;
  for (int j = 0; j < n; ++j) sum += sym[(size_t)j * n + i] < p ? aff[(size_t)j * n + i] : 0.0f;
  dinv[(size_t)e * n + i] = 1.0f / sqrtf(fmaxf(sum, 1e-9f));
}
__global__ void laplacian_kernel(const float* __restrict__ aff, const unsigned short* __restrict__ sym, int n, int p0,
                                 const float* __restrict__ dinv, float* __restrict__ lap) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, e = blockIdx.z;
  if (j >= n) return;
  const int p = p0 + e;
  const float a = sym[(size_t)i * n + j] < p ? aff[(size_t)i * n + j] : 0.0f;
  const float x = dinv[(size_t)e * n + i] * a * dinv[(size_t)e * n + j];
  lap[((size_t)e * n + i) * n + j] = i == j ? 1.0f - x : -x;
}

// ---- symmetric eigensolver: cyclic Jacobi, round-robin ordering (diar_jacobi.h) -----------------------------------
__global__ void eig_init_kernel(EigDesc* __restrict__ descs) {
  EigDesc& d = descs[blockIdx.y];
  if (!d.V) return;
  const size_t nn = (size_t)d.n * d.n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nn; e += (size_t)gridDim.x * blockDim.x)
    d.V[e] = (e / d.n == e % d.n) ? 1.0f : 0.0f;
}

// The sum of one value per thread, in an order that depends on the workgroup's size alone.
template <int NT>
__device__ double block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}
// off <= n * eps * diag on the sums of squares.  The squares and their sums are double: the square of any finite f32 lies
// inside its range, so the test reads the same whatever the scale of the matrix (in f32 the squares of entries above
// 1.8e19 are inf and those of entries below 1e-23 are 0, and either way the test passed at once).
__device__ inline bool converged(double off2, double diag2, int n) {
  const double tol = (double)n * (double)kEps;
  return off2 <= tol * tol * diag2;
}

// Form 1: one workgroup per matrix of order <= kLdsN, the matrix in LDS (the vectors, where wanted, in global memory).
constexpr int kLdsThreads = 512;
constexpr size_t kLdsRedAt = ((size_t)kLdsN * kLdsN + 3 * (kLdsN / 2 + 1) + 1) / 2 * 2;      // in floats, even: red is double
__global__ __launch_bounds__(kLdsThreads) void eig_lds_kernel(EigDesc* __restrict__ descs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  EigDesc& d = descs[blockIdx.x];
  const int n = d.n, m = rr_steps(n), K = rr_pairs(n), tid = threadIdx.x;
  float* a = lds;                        // [n][n]
  float* cs = a + (size_t)kLdsN * kLdsN;  // [K][3]: c, s, t
  double* red = reinterpret_cast<double*>(lds + kLdsRedAt);  // [kLdsThreads]
  for (int e = tid; e < n * n; e += kLdsThreads) a[e] = d.A[e];
  __syncthreads();
  int status = 1;
  bool last = false;      // the convergence test has passed: one more sweep, which takes the off-diagonal to rounding level
  for (int sweep = 0; sweep <= kMaxSweeps; ++sweep) {
    double off2 = 0.0, diag2 = 0.0;
    for (int e = tid; e < n * n; e += kLdsThreads) {
      const double v = (double)a[e] * (double)a[e];
      if (e / n == e % n) diag2 += v; else off2 += v;
    }
    off2 = block_sum<kLdsThreads>(off2, red);
    diag2 = block_sum<kLdsThreads>(diag2, red);
    if (last) break;
    if (converged(off2, diag2, n)) { status = 0; last = true; }
    else if (sweep == kMaxSweeps) break;
    for (int t = 0; t < m; ++t) {
      for (int l = tid; l < K; l += kLdsThreads) {
        int p, q;
        rr_pair(n, t, l, &p, &q);
        float c = 1.0f, s = 0.0f, tn = 0.0f;
        if (q >= 0) jacobi_cs(a[p * n + p], a[q * n + q], a[p * n + q], &c, &s, &tn);
        cs[3 * l] = c;
        cs[3 * l + 1] = s;
        cs[3 * l + 2] = tn;
      }
      __syncthreads();
      for (int e = tid; e < K * K; e += kLdsThreads) {
        const int k = e / K, l = e % K;
        int p, q, r, u;
        rr_pair(n, t, k, &p, &q);
        rr_pair(n, t, l, &r, &u);
        float x_pr = a[p * n + r], x_ps = u >= 0 ? a[p * n + u] : 0.0f;
        float x_qr = q >= 0 ? a[q * n + r] : 0.0f, x_qs = (q >= 0 && u >= 0) ? a[q * n + u] : 0.0f;
        if (k == l) rot_diag(x_pr, x_ps, x_qr, x_qs, cs[3 * k + 2]);
        else rot_block(x_pr, x_ps, x_qr, x_qs, cs[3 * k], cs[3 * k + 1], cs[3 * l], cs[3 * l + 1]);
        a[p * n + r] = x_pr;
        if (u >= 0) a[p * n + u] = x_ps;
        if (q >= 0) a[q * n + r] = x_qr;
        if (q >= 0 && u >= 0) a[q * n + u] = x_qs;
      }
      if (d.V) {
        for (int e = tid; e < n * K; e += kLdsThreads) {
          const int i = e / K, l = e % K;
          int r, u;
          rr_pair(n, t, l, &r, &u);
          if (u < 0) continue;
          float x = d.V[(size_t)i * n + r], y = d.V[(size_t)i * n + u];
          rot_vec(x, y, cs[3 * l], cs[3 * l + 1]);
          d.V[(size_t)i * n + r] = x;
          d.V[(size_t)i * n + u] = y;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += kLdsThreads) d.A[(size_t)i * n + i] = a[i * n + i];
  if (tid == 0) { d.status = status; d.active = 0; }
}

// Form 2: the matrices in global memory, every workgroup a slice of one.  Per sweep one eig_norm_kernel; per rotation
// set one eig_cs_kernel and one eig_apply_kernel over all matrices (a matrix that is done or has fewer steps sits out).
constexpr int kNormThreads = 1024;
__global__ __launch_bounds__(kNormThreads) void eig_norm_kernel(EigDesc* __restrict__ descs, int* __restrict__ n_active) {
  __shared__ double red[kNormThreads];
  EigDesc& d = descs[blockIdx.x];
  if (!d.active) return;
  const int n = d.n;
  double off2 = 0.0, diag2 = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = threadIdx.x; j < n; j += kNormThreads) {
      const double v = d.A[(size_t)i * n + j];
      if (i == j) diag2 += v * v; else off2 += v * v;
    }
  off2 = block_sum<kNormThreads>(off2, red);
  diag2 = block_sum<kNormThreads>(diag2, red);
  if (threadIdx.x == 0) {      // active 2: the test has passed, one more sweep follows (as in the LDS form)
    if (d.active == 2) d.active = 0;
    else {
      if (converged(off2, diag2, n)) { d.active = 2; d.status = 0; }
      atomicAdd(n_active, 1);
    }
  }
}
__global__ void eig_cs_kernel(EigDesc* __restrict__ descs, int t) {
  const EigDesc& d = descs[blockIdx.y];
  const int n = d.n, l = blockIdx.x * blockDim.x + threadIdx.x;
  if (!d.active || t >= rr_steps(n) || l >= rr_pairs(n)) return;
  int p, q;
  rr_pair(n, t, l, &p, &q);
  float c = 1.0f, s = 0.0f, tn = 0.0f;
  if (q >= 0) jacobi_cs(d.A[(size_t)p * n + p], d.A[(size_t)q * n + q], d.A[(size_t)p * n + q], &c, &s, &tn);
  d.cs[3 * l] = c;
  d.cs[3 * l + 1] = s;
  d.cs[3 * l + 2] = tn;
}
// blockIdx.y < kb: 16 x 16 blocks (k, l) of the matrix; beyond: 16 rows of the vectors each
constexpr int kApT = 16;
__global__ __launch_bounds__(kApT* kApT) void eig_apply_kernel(EigDesc* __restrict__ descs, int t, int kb) {
  const EigDesc& d = descs[blockIdx.z];
  const int n = d.n, K = rr_pairs(n);
  if (!d.active || t >= rr_steps(n)) return;
  const int tx = threadIdx.x % kApT, ty = threadIdx.x / kApT;
  const int l = blockIdx.x * kApT + tx;
  if (l >= K) return;
  int r, u;
  rr_pair(n, t, l, &r, &u);
  const float cl = d.cs[3 * l], sl = d.cs[3 * l + 1];
  if ((int)blockIdx.y < kb) {
    const int k = blockIdx.y * kApT + ty;
    if (k >= K) return;
    int p, q;
    rr_pair(n, t, k, &p, &q);
    float* A = d.A;
    float x_pr = A[(size_t)p * n + r], x_ps = u >= 0 ? A[(size_t)p * n + u] : 0.0f;
    float x_qr = q >= 0 ? A[(size_t)q * n + r] : 0.0f, x_qs = (q >= 0 && u >= 0) ? A[(size_t)q * n + u] : 0.0f;
    if (k == l) rot_diag(x_pr, x_ps, x_qr, x_qs, d.cs[3 * k + 2]);
    else rot_block(x_pr, x_ps, x_qr, x_qs, d.cs[3 * k], d.cs[3 * k + 1], cl, sl);
    A[(size_t)p * n + r] = x_pr;
    if (u >= 0) A[(size_t)p * n + u] = x_ps;
    if (q >= 0) A[(size_t)q * n + r] = x_qr;
    if (q >= 0 && u >= 0) A[(size_t)q * n + u] = x_qs;
  } else {
    const int i = ((int)blockIdx.y - kb) * kApT + ty;
    if (!d.V || i >= n || u < 0) return;
    float x = d.V[(size_t)i * n + r], y = d.V[(size_t)i * n + u];
    rot_vec(x, y, cl, sl);
    d.V[(size_t)i * n + r] = x;
    d.V[(size_t)i * n + u] = y;
  }
}

// Eigenvalues ascending (equal ones in the order of their index), the vectors' columns with them.
__global__ __launch_bounds__(256) void eig_sort_kernel(EigDesc* __restrict__ descs) {
  __shared__ float dg[kMaxN];
  __shared__ unsigned short pos[kMaxN];
  const EigDesc& d = descs[blockIdx.x];
  const int n = d.n;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dg[i] = d.A[(size_t)i * n + i];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float v = dg[i];
    int cnt = 0;
    for (int o = 0; o < n; ++o) cnt += (dg[o] < v) | ((dg[o] == v) & (o < i));
    pos[i] = (unsigned short)cnt;
    d.evals[cnt] = v;
  }
  if (!d.evecs) return;
  __syncthreads();
  for (size_t e = threadIdx.x; e < (size_t)n * n; e += blockDim.x) {
    const int row = (int)(e / n), c = (int)(e % n);
    d.evecs[(size_t)row * n + pos[c]] = d.V[e];
  }
}

// ---- decision (:459-471, 570-582): one thread per recording ---------------------------------------------------------
__global__ void decide_kernel(const ClusterDesc* __restrict__ recs, crispy_diar_info* __restrict__ infos) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (int)gridDim.x * (int)blockDim.x) return;
  const ClusterDesc& c = recs[r];
  if (c.n <= 2) return;
  const int n = c.n, lim = min(c.kmax + 1, n);
  bool have = false;
  float best_ratio = 0.0f, gap_at = 0.0f;
  int best_p = 1, best_k = 1;
  for (int p = 1; p <= c.p_max; ++p) {
    const float* ev = c.evals + (size_t)(p - 1) * n;
    int k = 1;
    float gap = -FLT_MAX;
    for (int i = 1; i < lim; ++i) {
      const float g = ev[i] - ev[i - 1];
      if (g > gap) { gap = g; k = i; }
    }
    gap = fmaxf(gap, 0.0f);
    const float ratio = ((float)p / (float)n) / fmaxf(gap, 1e-6f);
    if (!have || ratio < best_ratio) { have = true; best_ratio = ratio; best_p = p; best_k = k; gap_at = gap; }
  }
  crispy_diar_info& o = infos[c.index];
  o.p_star = best_p;
  o.k = min(max(best_k, 1), c.kmax);
  o.ratio = best_ratio;
  o.gap = gap_at;
  o.p_max = c.p_max;
}

// ---- spectral rows (:598-609) and kmeans (:474-534): one workgroup per recording --------------------------------------
constexpr int kKmThreads = 256;
__device__ inline float sq_dist(const float* a, const float* b, int dim) {
  float s = 0.0f;
  for (int d = 0; d < dim; ++d) {
    const float t = a[d] - b[d];
    s += t * t;
  }
  return s;
}
__global__ __launch_bounds__(kKmThreads) void kmeans_kernel(const ClusterDesc* __restrict__ recs, const crispy_diar_info* __restrict__ infos) {
  __shared__ float mind[kMaxN];
  __shared__ float red_d[kKmThreads];
  __shared__ int red_i[kKmThreads];
  __shared__ int changed;
  const ClusterDesc& c = recs[blockIdx.x];
  const int n = c.n, k = infos[c.index].k, tid = threadIdx.x;
  if (k <= 1 || k >= n) {      // (:476-481) before a point is read: a recording of a cluster call has 1 <= k < n
    for (int i = tid; i < n; i += kKmThreads) c.labels[i] = k <= 1 ? 0 : i;
    return;
  }
  float* pts = c.pts;          // [n][k]
  float* ctr = c.centers;      // [k][k]
  for (int i = tid; i < n; i += kKmThreads) {
    float ss = 0.0f;
    for (int d = 0; d < k; ++d) {
      const float x = c.evecs[(size_t)i * n + d];
      ss += x * x;
    }
    const float norm = sqrtf(ss);
    for (int d = 0; d < k; ++d) {
      const float x = c.evecs[(size_t)i * n + d];
      pts[(size_t)i * k + d] = norm > 1e-9f ? x / norm : x;
    }
    mind[i] = FLT_MAX;
    c.labels[i] = 0;
  }
  __syncthreads();
  for (int d = tid; d < k; d += kKmThreads) ctr[d] = pts[d];
  __syncthreads();
  for (int nc = 1; nc < k; ++nc) {      // the point farthest from its nearest centre, the first of equals
    float bd = -1.0f;
    int bi = 0;
    for (int i = tid; i < n; i += kKmThreads) {
      const float dd = fminf(mind[i], sq_dist(pts + (size_t)i * k, ctr + (size_t)(nc - 1) * k, k));
      mind[i] = dd;
      if (dd > bd) { bd = dd; bi = i; }
    }
    red_d[tid] = bd;
    red_i[tid] = bi;
    __syncthreads();
    for (int s = kKmThreads / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const float od = red_d[tid + s];
        const int oi = red_i[tid + s];
        if (od > red_d[tid] || (od == red_d[tid] && oi < red_i[tid])) { red_d[tid] = od; red_i[tid] = oi; }
      }
      __syncthreads();
    }
    const int best = red_i[0];
    for (int d = tid; d < k; d += kKmThreads) ctr[(size_t)nc * k + d] = pts[(size_t)best * k + d];
    __syncthreads();
  }
  for (int it = 0; it < 50; ++it) {
    if (tid == 0) changed = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kKmThreads) {
      int bc = 0;
      float bd = FLT_MAX;
      for (int cc = 0; cc < k; ++cc) {
        const float dd = sq_dist(pts + (size_t)i * k, ctr + (size_t)cc * k, k);
        if (dd < bd) { bd = dd; bc = cc; }
      }
      if (c.labels[i] != bc) { c.labels[i] = bc; changed = 1; }
    }
    __syncthreads();
    for (int e = tid; e < k * k; e += kKmThreads) {
      const int cc = e / k, d = e % k;
      float sum = 0.0f;
      int count = 0;
      for (int i = 0; i < n; ++i)
        if (c.labels[i] == cc) { sum += pts[(size_t)i * k + d]; ++count; }
      if (count > 0) ctr[e] = sum / (float)count;
    }
    __syncthreads();
    if (!changed) break;
    __syncthreads();
  }
}

hipError_t lds_limit(const void* fn, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

hipError_t launch_affinity(const float* d_emb, int n, int dim, float* d_aff, hipStream_t st) {
  const int g = (n + kAffT - 1) / kAffT;
  affinity_kernel<<<dim3(g, g), kAffT * kAffT, 0, st>>>(d_emb, n, dim, d_aff);
  return hipGetLastError();
}
hipError_t launch_nonfinite(const float* d_x, size_t count, int* d_flag, hipStream_t st) {
  const int g = (int)std::min<size_t>((count + 255) / 256, 2048);
  nonfinite_kernel<<<g, 256, 0, st>>>(d_x, count, d_flag);
  return hipGetLastError();
}
hipError_t launch_rank(const float* d_aff, int n, unsigned short* d_rank, unsigned short* d_sym, hipStream_t st) {
  rank_kernel<<<n, 256, 0, st>>>(d_aff, n, d_rank);
  symrank_kernel<<<dim3((n + 255) / 256, n), 256, 0, st>>>(d_rank, n, d_sym);
  return hipGetLastError();
}
hipError_t launch_laplacians(const float* d_aff, const unsigned short* d_sym, int n, int p0, int count,
                             float* d_dinv, float* d_lap, hipStream_t st) {
  dinv_kernel<<<dim3((n + 63) / 64, count), 64, 0, st>>>(d_aff, d_sym, n, p0, d_dinv);
  laplacian_kernel<<<dim3((n + 255) / 256, n, count), 256, 0, st>>>(d_aff, d_sym, n, p0, d_dinv, d_lap);
  return hipGetLastError();
}
hipError_t launch_eig_init(EigDesc* d_descs, int count, hipStream_t st) {
  eig_init_kernel<<<dim3(64, count), 256, 0, st>>>(d_descs);
  return hipGetLastError();
}
size_t eig_lds_bytes() { return kLdsRedAt * sizeof(float) + kLdsThreads * sizeof(double); }
hipError_t launch_eig_lds(EigDesc* d_descs, int count, hipStream_t st) {
  const hipError_t e = lds_limit(reinterpret_cast<const void*>(eig_lds_kernel), eig_lds_bytes());
  if (e != hipSuccess) return e;
  eig_lds_kernel<<<count, kLdsThreads, eig_lds_bytes(), st>>>(d_descs);
  return hipGetLastError();
}
hipError_t launch_eig_norm(EigDesc* d_descs, int count, int* d_n_active, hipStream_t st) {
  eig_norm_kernel<<<count, kNormThreads, 0, st>>>(d_descs, d_n_active);
  return hipGetLastError();
}
hipError_t launch_eig_step(EigDesc* d_descs, int count, int max_n, bool vectors, int t, hipStream_t st) {
  const int K = rr_pairs(max_n), kb = (K + kApT - 1) / kApT;
  eig_cs_kernel<<<dim3((K + 255) / 256, count), 256, 0, st>>>(d_descs, t);
  eig_apply_kernel<<<dim3(kb, kb + (vectors ? (max_n + kApT - 1) / kApT : 0), count), kApT * kApT, 0, st>>>(d_descs, t, kb);
  return hipGetLastError();
}
hipError_t launch_eig_sort(EigDesc* d_descs, int count, hipStream_t st) {
  eig_sort_kernel<<<count, 256, 0, st>>>(d_descs);
  return hipGetLastError();
}
hipError_t launch_decide(const ClusterDesc* d_recs, int count, crispy_diar_info* d_infos, hipStream_t st) {
  decide_kernel<<<count, 1, 0, st>>>(d_recs, d_infos);
  return hipGetLastError();
}
hipError_t launch_kmeans(const ClusterDesc* d_recs, int count, const crispy_diar_info* d_infos, hipStream_t st) {
  kmeans_kernel<<<count, kKmThreads, 0, st>>>(d_recs, d_infos);
  return hipGetLastError();
}

}  // namespace diar
}  // namespace crispy

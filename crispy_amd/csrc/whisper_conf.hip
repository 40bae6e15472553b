// whisper_conf.hip -- confidence numbers read off logits rows that are already in HBM (crispy_asr_set_confidence):
//   tok_logprob_kernel   the log-probability of one target id per row under the soft-max over the first `n_cols` ids of the
//                        row: logit[target] - (max + log sum exp(. - max)).  softmax_prob_kernel (whisper_pick.hip) with a
//                        target per row, a column limit and a log-domain result -- openai-whisper's
//                        `logits[len(sot):, :eot].softmax(-1)` of the teacher-forced alignment pass (timing.py: find_alignment)
//                        [UPSTREAM-RECALL]; the exponential is taken on the host, only where a probability is published.
//   lang_probs_kernel    soft-max over the contiguous language ids [lang0, lang0 + n_lang) of a row: whisper.cpp's
//                        whisper_lang_auto_detect `lang_probs` [UPSTREAM-RECALL].  One wave per row (99 / 100 values).
// Both reduce within a wave by shuffles (DPP) and, the first, across the waves of the workgroup through LDS, in a fixed order:
// a row's result depends on the row alone, never on the rows launched with it.
// decode_steps.cpp reaches the two launchers through a table this file installs at static initialisation (g_conf_kernels).
#include "whisper_internal.h"
#include "wave_ops.h"

namespace crispy {
namespace {

constexpr int kLpThreads = 1024, kLpWaves = kLpThreads / 64;

// grid (rows), 1024 threads.  Row r of the launch is position pos + r % P of clip r / P (the rows of a multi-position prompt
// step); its target and its result live at [clip][ld_t] + position.  target < 0: the row has nothing to predict (left padding,
// the last position) and is skipped.  Columns >= n_cols -- the specials from <|endoftext|> on, the padding of a row -- are
// never read.  Rows are 16-byte aligned (ld % 4 == 0): float4 loads over the whole quads, the tail singly.
__global__ __launch_bounds__(kLpThreads) void tok_logprob_kernel(const float* __restrict__ logits, long ld, int n_cols,
                                                                 const int* __restrict__ target, float* __restrict__ logp, int ld_t,
                                                                 int P, int pos) {
  __shared__ float s_r[kLpWaves];
  const int r = blockIdx.x, tid = threadIdx.x;
  const long at = (long)(r / P) * ld_t + pos + r % P;
  const int t = target[at];
  if (t < 0 || t >= n_cols) return;                  // (uniform over the workgroup)
  const float* lg = logits + (long)r * ld;
  const float4* lg4 = reinterpret_cast<const float4*>(lg);
  const int n4 = n_cols / 4;
  float m = -INFINITY;
  for (int v = tid; v < n4; v += kLpThreads) {
    const float4 x = lg4[v];
    m = fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w));
  }
  if (tid < n_cols - 4 * n4) m = fmaxf(m, lg[4 * n4 + tid]);
  m = shfl_max(m);
  if ((tid & 63) == 0) s_r[tid >> 6] = m;
  __syncthreads();
  m = s_r[0];
#pragma unroll
  for (int w = 1; w < kLpWaves; ++w) m = fmaxf(m, s_r[w]);
  __syncthreads();
  float sum = 0.f;
  for (int v = tid; v < n4; v += kLpThreads) {
    const float4 x = lg4[v];
    sum += (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
  }
  if (tid < n_cols - 4 * n4) sum += expf(lg[4 * n4 + tid] - m);
  sum = shfl_sum(sum);
  if ((tid & 63) == 0) s_r[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < kLpWaves; ++w) tot += s_r[w];
    logp[at] = lg[t] - (m + logf(tot));
  }
}

// grid (ceil(rows / 4)), 256 threads: wave w of a workgroup takes row 4 * blockIdx.x + w; lane l the ids lang0 + l and
// lang0 + 64 + l (n_lang <= 128).  probs [rows][n_lang].
__global__ __launch_bounds__(256) void lang_probs_kernel(const float* __restrict__ logits, long ld, int lang0, int n_lang,
                                                         float* __restrict__ probs, int rows) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;                             // (uniform over the wave)
  const float* lg = logits + (long)r * ld + lang0;
  const float a = lane < n_lang ? lg[lane] : -INFINITY;
  const float b = lane + 64 < n_lang ? lg[lane + 64] : -INFINITY;
  const float m = shfl_max(fmaxf(a, b));
  const float ea = lane < n_lang ? expf(a - m) : 0.f;
  const float eb = lane + 64 < n_lang ? expf(b - m) : 0.f;
  const float tot = shfl_sum(ea + eb);
  if (lane < n_lang) probs[(long)r * n_lang + lane] = ea / tot;
  if (lane + 64 < n_lang) probs[(long)r * n_lang + lane + 64] = eb / tot;
}

}  // namespace

hipError_t tok_logprob_f32(const float* logits, long ld, int n_cols, const int* target, float* logp, int ld_t, int P, int pos,
                           int rows, hipStream_t s) {
  if (rows < 1 || P < 1 || rows % P != 0 || pos < 0 || pos + P > ld_t || n_cols < 1 || n_cols > ld || ld % 4 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tok_logprob_kernel, dim3(rows), dim3(kLpThreads), 0, s, logits, ld, n_cols, target, logp, ld_t, P, pos);
  return hipGetLastError();
}

hipError_t lang_probs_f32(const float* logits, long ld, int lang0, int n_lang, float* probs, int rows, hipStream_t s) {
  if (rows < 1 || n_lang < 1 || n_lang > 128 || lang0 < 0 || lang0 + n_lang > ld) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lang_probs_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, ld, lang0, n_lang, probs, rows);
  return hipGetLastError();
}

namespace asr {
namespace {
const ConfKernels kConfKernels = {&tok_logprob_f32, &lang_probs_f32};
[[maybe_unused]] const bool kInstalled = (g_conf_kernels = &kConfKernels, true);
}  // namespace
}  // namespace asr

}  // namespace crispy

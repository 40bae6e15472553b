// whisper_pick.hip -- both ends of a decode step: the token embedding that starts it and the pick that ends it (gfx950).
//
//   embed_kernel           x = tok_emb[token] + pos_emb[position]: the prompt steps (a fused pick embeds its own token).
//   argmax_kernel          greedy pick under a suppression mask, one 1024-thread workgroup per row: plain greedy
//                          decoding and language detection.
//   ts_pick_kernel         greedy pick under the timestamp rules, with the pick's log-probability: whisper_full's
//                          greedy pass.
//   ts_sample_kernel       the sampling pick at a temperature > 0 (fallback passes), and the candidate draws of a beam
//                          search step (n_cand > 0).
//   beam_advance_kernel    one beam-search step per clip, decided on the device: deals the candidates to the decoders.
//   beam_kv_copy_kernel    moves the parents' self K|V rows behind it (beam_kv_reorder: gather, then scatter).
//   softmax_prob_kernel    the probability of one token over the unfiltered row (no_speech_prob).
//
// With StepFuse::x set, argmax / ts_pick / ts_sample / beam_advance also start the next step (step_fuse_*: embedding of
// the pick, counters moved on by the last workgroup), so a captured step is replayed without the host.  The launchers are
// called from decode_steps.cpp alone, whichever kernels run the layers of the step.
#include "asr_common.h"
#include "asr_quant.h"
#include "wave_ops.h"

namespace crispy {
namespace {

// token + positional embedding for one decode step: x[b][:] = tok_emb[token[b]] + pos_emb[pos]
__global__ __launch_bounds__(256) void embed_kernel(const int* __restrict__ tokens, const float* __restrict__ tok_emb,
                                                    const float* __restrict__ pos_emb, int pos,
                                                    const int* __restrict__ pos_dev, float* __restrict__ x, int D, int rpc,
                                                    const int* __restrict__ row_off) {
  const int b = blockIdx.x;
  const int tok = tokens[b];
  if (pos_dev) pos = *pos_dev;
  pos += b % rpc;                       // rpc rows per clip (the batched prompt step): consecutive positions
  if (row_off) pos = max(pos - row_off[b / rpc], 0);      // left-padded prompts: cache row -> position of this clip
  for (int c = threadIdx.x; c < D; c += 256) x[(long)b * D + c] = tok_emb[(long)tok * D + c] + pos_emb[(long)pos * D + c];
}

// greedy pick: argmax over the vocabulary with a suppression mask (mask[v] != 0 -> -inf); ties -> lowest id.
// One 1024-thread block per clip; every thread walks the row in float4 / uchar4 steps with four loads in flight
// (the 256-thread, one-float-per-iteration version ran at 0.1 TB/s: 118 us for 64 x 51865 logits).
constexpr int PICK_UNROLL = 13;                // float4 per thread of a 1024-thread pick: 53 248 logits in one round of requests
__device__ __forceinline__ unsigned load_u32_unaligned(const unsigned char* p) {
  unsigned v;
  __builtin_memcpy(&v, p, 4);                  // global memory takes unaligned dword loads; the compiler emits one
  return v;
}
// the tail of a fused pick: embedding of the pick for the next step, then the counters by the last workgroup to finish
__device__ __forceinline__ void step_fuse_embed(const StepFuse& f, int tok, int pos, int b, int tid) {
  const int pe = f.row_off ? pos - f.row_off[b] : pos;    // cache row `pos` is position pos - row_off[b] of a left-padded clip
  if (f.tok_emb_q) {
    for (int c = tid; c < f.D; c += (int)blockDim.x)
      f.x[(long)b * f.D + c] = q_elem(f.tok_emb_q, f.tok_emb_ttype, (long)tok * f.D + c) + f.pos_emb[(long)pe * f.D + c];
  } else {
    for (int c = tid; c < f.D; c += (int)blockDim.x) f.x[(long)b * f.D + c] = f.tok_emb[(long)tok * f.D + c] + f.pos_emb[(long)pe * f.D + c];
  }
}
__device__ __forceinline__ void step_fuse_ticket(const StepFuse& f, int pos, int step, int tid) {
  if (tid == 0) {
    // No fence: nothing of this kernel is read by another workgroup of it -- the ticket only elects the workgroup that
    // stores the counters, every workgroup has consumed the old values long before its own increment, and the
    // kernels behind read everything after the kernel boundary.  (A device-scope fence here writes back and
    // invalidates the XCD's L2 once per workgroup and step.)
    const unsigned t = atomicAdd(reinterpret_cast<unsigned*>(f.counters + 2), 1u);
    if (t == gridDim.x - 1) {              // everyone else has finished, so everyone has read the old counters
      f.counters[0] = pos;
      f.counters[1] = step + 1;
      f.counters[2] = 0;
    }
  }
}
__device__ __forceinline__ void step_fuse_tail(const StepFuse& f, int tok, int pos, int step, int b, int tid) {
  step_fuse_embed(f, tok, pos, b, tid);
  step_fuse_ticket(f, pos, step, tid);
}

__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ mask,
                                                      const unsigned char* __restrict__ mask_first,
                                                      const int* __restrict__ step_dev, int V, long ld, int* __restrict__ tokens_out,
                                                      int* __restrict__ tokens_all, float* __restrict__ best_logit,
                                                      int eot, int* __restrict__ finished, int* __restrict__ done_count, StepFuse fuse) {
  __shared__ float sv[16];
  __shared__ int si[16];
  __shared__ int s_tok;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int step = fuse.x ? fuse.counters[1] : step_dev ? *step_dev : 0;
  const int pos = fuse.x ? fuse.counters[0] + 1 : 0;
  if (step == 0 && mask_first) mask = mask_first;
  const float* lg = logits + (long)b * ld;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  auto consider = [&](float x, int v) {
    if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
  };
  // rows start 4-byte aligned only (V is odd): scalar head up to the first 16-byte boundary, vector body, scalar tail
  const int head = (int)(((16 - ((size_t)lg & 15)) & 15) >> 2);
  if (tid < head && tid < V) consider((mask && mask[tid]) ? -INFINITY : lg[tid], tid);
  const int nvec = (V - head) >> 2;
  const float4* lg4 = reinterpret_cast<const float4*>(lg + head);
  // The whole row in flight at once: PICK_UNROLL x 1024 float4 cover 53 248 logits, requested from clamped addresses
  // before any is looked at (with `unroll 4` the scan was four dependent round trips), and the four mask bytes of a
  // float4 as ONE unaligned 32-bit load (rows and so v0 are only 4-byte aligned in the logits, 1-byte in the mask).
  {
    float4 xs[PICK_UNROLL];
    unsigned ms[PICK_UNROLL];
#pragma unroll
    for (int u = 0; u < PICK_UNROLL; ++u) {
      const int q = min(tid + 1024 * u, nvec - 1);
      xs[u] = lg4[q];
      ms[u] = mask ? load_u32_unaligned(mask + head + 4 * q) : 0u;
    }
#pragma unroll
    for (int u = 0; u < PICK_UNROLL; ++u) {
      const int q = tid + 1024 * u;
      if (q < nvec) {
        const int v0 = head + 4 * q;
        consider((ms[u] & 0xffu) ? -INFINITY : xs[u].x, v0);
        consider((ms[u] & 0xff00u) ? -INFINITY : xs[u].y, v0 + 1);
        consider((ms[u] & 0xff0000u) ? -INFINITY : xs[u].z, v0 + 2);
        consider((ms[u] & 0xff000000u) ? -INFINITY : xs[u].w, v0 + 3);
      }
    }
  }
  for (int q = tid + 1024 * PICK_UNROLL; q < nvec; q += 1024) {          // vocabularies beyond 53 248 entries
    const float4 x = lg4[q];
    const int v0 = head + 4 * q;
    unsigned char m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    if (mask) { m0 = mask[v0]; m1 = mask[v0 + 1]; m2 = mask[v0 + 2]; m3 = mask[v0 + 3]; }
    consider(m0 ? -INFINITY : x.x, v0);
    consider(m1 ? -INFINITY : x.y, v0 + 1);
    consider(m2 ? -INFINITY : x.z, v0 + 2);
    consider(m3 ? -INFINITY : x.w, v0 + 3);
  }
  for (int v = head + 4 * nvec + tid; v < V; v += 1024) consider((mask && mask[v]) ? -INFINITY : lg[v], v);
  // wave arg-max (ties -> lowest id), then the 16 wave results
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
  }
  if ((tid & 63) == 0) { sv[tid >> 6] = bv; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w)
      if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
    tokens_out[b] = bi;
    if (tokens_all) tokens_all[(long)step * gridDim.x + b] = bi;
    if (best_logit) best_logit[(long)step * gridDim.x + b] = bv;
    // first EOT of this clip: the host polls done_count and stops replaying the step graph once every clip has one
    if (finished && bi == eot && !finished[b]) { finished[b] = 1; atomicAdd(done_count, 1); }
    s_tok = bi;
  }
  if (fuse.x) {
    __syncthreads();
    step_fuse_tail(fuse, s_tok, pos, step, b, tid);
  }
}

// What may be picked next in a window under the timestamp rules (oracle/whisper_oracle.py: _apply_rules), from the
// window's state; uniform per clip and step.
struct TsRule {
  const unsigned char* mask;
  int beg, not_tok, ts_lo, ts_hi;     // timestamps below ts_lo and above ts_hi are not allowed
  bool no_ts, forced_ts, text_allowed;
  __device__ __forceinline__ TsRule(const TsPickArgs& a, const TsState& st) {
    mask = (st.n == 0 && a.mask_first) ? a.mask_first : a.mask;
    beg = a.beg; not_tok = a.not_tok;
    const bool last_ts = st.n >= 1 && st.last >= a.beg;
    const bool pen_ts = st.n < 2 || st.prev >= a.beg;
    ts_lo = a.beg; ts_hi = a.V - 1;
    if (st.last_ts >= 0) ts_lo = (a.rules == TS_RULES_OPENAI && !(last_ts && !pen_ts)) ? st.last_ts + 1 : st.last_ts;
    const bool initial = st.n == 0;
    if (initial && a.max_initial_ts > 0) ts_hi = a.beg + a.max_initial_ts;
    no_ts = last_ts && pen_ts;
    forced_ts = initial && a.rules == TS_RULES_OPENAI;      // the first pick is a timestamp
    text_allowed = !(last_ts && !pen_ts) && !forced_ts;     // ids < eot
  }
  // ids >= eot (EOT, specials, timestamps)
  __device__ __forceinline__ bool masked_hi(int v) const {
    if (mask && mask[v]) return true;
    if (v == not_tok) return true;
    if (v >= beg) return no_ts || v < ts_lo || v > ts_hi;
    return forced_ts;
  }
  __device__ __forceinline__ bool allowed(int v, int eot) const {
    if (v < eot) return text_allowed && !(mask && mask[v]);
    return !masked_hi(v);
  }
  // the same with the id's suppression byte already loaded (the sampling pick reads eight at a time)
  __device__ __forceinline__ bool allowed_m(int v, int eot, bool masked) const {
    if (masked) return false;
    if (v < eot) return text_allowed;
    if (v == not_tok) return false;
    if (v >= beg) return !(no_ts || v < ts_lo || v > ts_hi);
    return !forced_ts;
  }
};

// record a pick and move the window's state on (thread 0 of the clip's workgroup)
__device__ __forceinline__ void ts_commit(const TsPickArgs& a, TsState& st, int b, int step, int pick, int tsid, float plog) {
  a.tokens_out[b] = pick;
  a.tokens_all[(long)step * gridDim.x + b] = pick;
  a.tids_all[(long)step * gridDim.x + b] = tsid;
  if (a.plog_all) a.plog_all[(long)step * gridDim.x + b] = plog;
  st.prev = st.last;
  st.last = pick;
  st.n += 1;
  if (a.rules == TS_RULES_OPENAI ? pick >= a.beg : pick > a.beg) st.last_ts = pick;
  bool done = pick == a.eot;
  if (a.rules == TS_RULES_WCPP && st.last_ts >= 0 && st.seek + 2 * (st.last_ts - a.beg) + a.delta_min >= st.seek_end) done = true;
  if (done) { st.done = 1; atomicAdd(a.done_count, 1); }
  a.st[b] = st;
}

// greedy pick under the timestamp rules: one 1024-thread block per clip.  Plain text tokens [0, eot) are either all
// subject to the suppression mask only or not allowed at all (uniform per clip and step), so they are scanned in
// float4 steps or skipped; the ~1600 special and timestamp ids take the per-id rule path.  The row stays in registers
// between the two passes: maxima (the pick, the reference point of the exponentials), then the two sums -- over
// everything allowed (the pick's log-probability, whisper_token_data::plog) and over the allowed timestamps (the
// probability-mass rule).
__global__ __launch_bounds__(1024) void ts_pick_kernel(TsPickArgs a) {
  __shared__ float s_v[2][16];
  __shared__ int s_i[2][16];
  __shared__ float s_sum[2][16];
  __shared__ int s_tok;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int step = a.fuse.x ? a.fuse.counters[1] : a.step_dev ? *a.step_dev : 0;
  const int pos = a.fuse.x ? a.fuse.counters[0] + 1 : 0;
  TsState st = a.st[b];
  if (st.done) {   // finished window: keep feeding EOT so that the batch stays in lock step
    if (tid == 0) {
      a.tokens_out[b] = a.eot;
      a.tokens_all[(long)step * gridDim.x + b] = a.eot;
      a.tids_all[(long)step * gridDim.x + b] = a.beg;
      if (a.plog_all) a.plog_all[(long)step * gridDim.x + b] = 0.f;
    }
    if (a.fuse.x) step_fuse_tail(a.fuse, a.eot, pos, step, b, tid);
    return;
  }
  const float* lg = a.logits + (long)b * a.ld;
  const TsRule rule(a, st);
  const unsigned char* mask = rule.mask;
  const bool text_allowed = rule.text_allowed;
  // the text range [0, eot): scalar head up to the first 16-byte boundary, float4 body in registers, scalar tail
  const int head = min((int)(((16 - ((size_t)lg & 15)) & 15) >> 2), a.eot);
  const int nvec = (a.eot - head) >> 2;
  const float4* lg4 = reinterpret_cast<const float4*>(lg + head);
  float4 xs[PICK_UNROLL];
  if (text_allowed) {                          // the whole text range in flight at once (see argmax_kernel)
    unsigned ms[PICK_UNROLL];
#pragma unroll
    for (int u = 0; u < PICK_UNROLL; ++u) {
      const int q = min(tid + 1024 * u, nvec - 1);
      xs[u] = lg4[q];
      ms[u] = mask ? load_u32_unaligned(mask + head + 4 * q) : 0u;
    }
#pragma unroll
    for (int u = 0; u < PICK_UNROLL; ++u) {
      if (ms[u] & 0xffu) xs[u].x = -INFINITY;
      if (ms[u] & 0xff00u) xs[u].y = -INFINITY;
      if (ms[u] & 0xff0000u) xs[u].z = -INFINITY;
      if (ms[u] & 0xff000000u) xs[u].w = -INFINITY;
    }
  }
  // the ids from EOT up (EOT, specials, timestamps: 1 608 of them, two per thread): value and rule evaluated once, kept in
  // registers for both passes (re-loading them in the second pass was another exposed round trip to the logits)
  float hx[2];
  bool hok[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = a.eot + tid + 1024 * k;
    hok[k] = v < a.V && !rule.masked_hi(min(v, a.V - 1));
    hx[k] = lg[min(v, a.V - 1)];
  }
  // every allowed (value, id) of this thread's share of the row: the plain text ids through FT(x, v), the ids from EOT up
  // through FH(x, v).  (A macro, not a lambda: closures that capture the running maxima by reference ended up in scratch.)
#define TS_SCAN(FT, FH)                                                                                              \
  do {                                                                                                               \
    if (text_allowed) {                                                                                              \
      if (tid < head) { const float x_ = (mask && mask[tid]) ? -INFINITY : lg[tid]; FT(x_, tid); }                   \
      _Pragma("unroll") for (int u = 0; u < PICK_UNROLL; ++u) {                                                      \
        const int q = tid + 1024 * u;                                                                                \
        if (q < nvec) {                                                                                              \
          const int v0 = head + 4 * q;                                                                               \
          FT(xs[u].x, v0); FT(xs[u].y, (v0 + 1)); FT(xs[u].z, (v0 + 2)); FT(xs[u].w, (v0 + 3));                      \
        }                                                                                                            \
      }                                                                                                              \
      for (int q = tid + 1024 * PICK_UNROLL; q < nvec; q += 1024) { /* vocabularies beyond 53 248 entries */         \
        float4 x = lg4[q];                                                                                           \
        const int v0 = head + 4 * q;                                                                                 \
        if (mask) {                                                                                                  \
          if (mask[v0]) x.x = -INFINITY;                                                                             \
          if (mask[v0 + 1]) x.y = -INFINITY;                                                                         \
          if (mask[v0 + 2]) x.z = -INFINITY;                                                                         \
          if (mask[v0 + 3]) x.w = -INFINITY;                                                                         \
        }                                                                                                            \
        FT(x.x, v0); FT(x.y, (v0 + 1)); FT(x.z, (v0 + 2)); FT(x.w, (v0 + 3));                                        \
      }                                                                                                              \
      for (int v = head + 4 * nvec + tid; v < a.eot; v += 1024) {                                                    \
        const float x_ = (mask && mask[v]) ? -INFINITY : lg[v];                                                      \
        FT(x_, v);                                                                                                   \
      }                                                                                                              \
    }                                                                                                                \
    _Pragma("unroll") for (int k = 0; k < 2; ++k)                                                                    \
      if (hok[k]) FH(hx[k], (a.eot + tid + 1024 * k));                                                               \
    for (int v = a.eot + tid + 2048; v < a.V; v += 1024)      /* more than 2 048 ids from EOT up: no such vocabulary */ \
      if (!rule.masked_hi(v)) { const float x_ = lg[v]; FH(x_, v); }                                                 \
  } while (0)
  float tv = -INFINITY, xv = -INFINITY;   // best text (v < beg) and best timestamp
  int ti = 0x7fffffff, xi = 0x7fffffff;
#define TS_MAX_T(x, v) do { if ((x) > tv || ((x) == tv && (v) < ti)) { tv = (x); ti = (v); } } while (0)
#define TS_MAX_H(x, v) do { if ((v) < a.beg) TS_MAX_T(x, v); else if ((x) > xv || ((x) == xv && (v) < xi)) { xv = (x); xi = (v); } } while (0)
  TS_SCAN(TS_MAX_T, TS_MAX_H);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    float ov = __shfl_xor(tv, off, 64); int oi = __shfl_xor(ti, off, 64);
    if (ov > tv || (ov == tv && oi < ti)) { tv = ov; ti = oi; }
    ov = __shfl_xor(xv, off, 64); oi = __shfl_xor(xi, off, 64);
    if (ov > xv || (ov == xv && oi < xi)) { xv = ov; xi = oi; }
  }
  if ((tid & 63) == 0) { s_v[0][tid >> 6] = tv; s_i[0][tid >> 6] = ti; s_v[1][tid >> 6] = xv; s_i[1][tid >> 6] = xi; }
  __syncthreads();
  float max_text = s_v[0][0], max_ts = s_v[1][0];
  int arg_text = s_i[0][0], arg_ts = s_i[1][0];
#pragma unroll
  for (int w = 1; w < 16; ++w) {
    if (s_v[0][w] > max_text || (s_v[0][w] == max_text && s_i[0][w] < arg_text)) { max_text = s_v[0][w]; arg_text = s_i[0][w]; }
    if (s_v[1][w] > max_ts || (s_v[1][w] == max_ts && s_i[1][w] < arg_ts)) { max_ts = s_v[1][w]; arg_ts = s_i[1][w]; }
  }
  // sums of exponentials: everything allowed against the overall maximum, the allowed timestamps against theirs
  const float max_all = fmaxf(max_text, max_ts);
  float sum_all = 0.f, sum = 0.f;
#define TS_SUM_T(x, v) do { (void)(v); sum_all += __expf((x) - max_all); } while (0)      /* (a masked value is -inf: adds 0) */
#define TS_SUM_H(x, v) do { sum_all += __expf((x) - max_all); if ((v) >= a.beg) sum += expf((x) - max_ts); } while (0)
  if (max_all > -INFINITY) TS_SCAN(TS_SUM_T, TS_SUM_H);
#undef TS_SUM_T
#undef TS_SUM_H
#undef TS_MAX_T
#undef TS_MAX_H
#undef TS_SCAN
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off, 64); sum_all += __shfl_xor(sum_all, off, 64); }
  if ((tid & 63) == 0) { s_sum[0][tid >> 6] = sum; s_sum[1][tid >> 6] = sum_all; }
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f, tot_all = 0.f;
    for (int w = 0; w < 16; ++w) { tot += s_sum[0][w]; tot_all += s_sum[1][w]; }
    const float lse_ts = max_ts > -INFINITY ? max_ts + logf(tot) : -INFINITY;
    int pick;
    if (lse_ts > max_text) pick = arg_ts;                       // timestamps carry more mass than any text token
    else pick = (max_ts > max_text) ? arg_ts : arg_text;        // plain arg-max, ties -> lowest id (text ids are lower)
    if (pick == 0x7fffffff) pick = a.eot;                       // everything masked: cannot happen with sane masks
    const int tsid = pick >= a.beg ? pick : (max_ts > -INFINITY ? arg_ts : a.beg);
    const float plog = (pick >= a.beg ? max_ts : max_text) - (max_all + logf(tot_all));
    ts_commit(a, st, b, step, pick, tsid, plog);
    s_tok = pick;
  }
  if (a.fuse.x) {
    __syncthreads();
    step_fuse_tail(a.fuse, s_tok, pos, step, b, tid);
  }
}

// The sampling form of the pick (whisper_sample_token(best = false) at a temperature > 0 [UPSTREAM-RECALL]): logits /
// temperature, the same rules, probabilities = exp(log-softmax) with the text tokens removed when the probability-mass
// rule fires, then std::discrete_distribution -- the first id whose cumulative share of the (re-normalised) probability
// reaches the uniform variate u the host drew for this (step, row).  Only the fallback path of whisper_full comes here
// (a window the greedy pass failed on), so the kernel is plain: thread t owns the ids [t * chunk, (t + 1) * chunk),
// three passes over them (maxima, sums, probabilities), cumulative sums in double.
// The sampling pick: 1024 threads per row.  Ids are dealt out in blocks of 8192: thread t owns the eight consecutive ids
// 8192 j + 8 t .. + 7 of every block j (7 blocks cover n_vocab <= 57 344: the launcher checks), so a wave's loads are two
// contiguous float4 runs per block -- and one 8-byte run of the suppression mask -- instead of 64 scattered lines per id
// (the first form, one contiguous range of ids per thread: 148 us per pick, most of a call that falls back through the
// temperature ladder).  Three passes over the row (maximum; sums; probabilities), each re-reading it from the L2 it was
// just written to: keeping the row in registers across the passes was tried in three shapes and spilled in all of them
// (56 - 104 values per lane beside three inlined expf per value).  The cumulative distribution runs in id order =
// (block, thread, element): per block an inclusive scan of the threads' eight-id sums in double, block bases from a
// 7 x 16 table of wave totals; the thread whose run contains u walks its eight ids.
constexpr int TS_THREADS = 1024, TS_WAVES = TS_THREADS / 64, TS_E = 8, TS_BLK = TS_THREADS * TS_E, TS_NB = 7;
static_assert(TS_SCRATCH_ROW == TS_NB * TS_BLK, "asr_common.h sizes the sampling pick's row scratch");
// x[e] = logit / T where the rules allow id v0 + e, -inf where they do not or past the row
__device__ __forceinline__ void ts_load_run(const TsRule& rule, const float* __restrict__ lg, int V, int eot, float T, int v0, float (&x)[TS_E]) {
  float raw[TS_E];
  unsigned char mk[TS_E];
  if (v0 + TS_E <= V) {                 // whole run inside the row: rows are 16-byte aligned (ld % 4 == 0), so is v0
    const float4 q0 = *reinterpret_cast<const float4*>(lg + v0), q1 = *reinterpret_cast<const float4*>(lg + v0 + 4);
    raw[0] = q0.x; raw[1] = q0.y; raw[2] = q0.z; raw[3] = q0.w; raw[4] = q1.x; raw[5] = q1.y; raw[6] = q1.z; raw[7] = q1.w;
    uint2 m8 = make_uint2(0u, 0u);
    if (rule.mask) m8 = *reinterpret_cast<const uint2*>(rule.mask + v0);
#pragma unroll
    for (int e = 0; e < TS_E; ++e) mk[e] = (unsigned char)((e < 4 ? m8.x >> (8 * e) : m8.y >> (8 * (e - 4))) & 0xffu);
  } else {
#pragma unroll
    for (int e = 0; e < TS_E; ++e) {
      const int v = v0 + e;
      raw[e] = v < V ? lg[v] : 0.f;
      mk[e] = (v < V && rule.mask) ? rule.mask[v] : 0;
    }
  }
#pragma unroll
  for (int e = 0; e < TS_E; ++e) {
    const int v = v0 + e;
    x[e] = (v < V && rule.allowed_m(v, eot, mk[e] != 0)) ? raw[e] / T : -INFINITY;
  }
}
__device__ __forceinline__ void ts_read_run(const float* __restrict__ xrow, int v0, float (&x)[TS_E]) {     // the thread's own stores
  const float4 q0 = *reinterpret_cast<const float4*>(xrow + v0), q1 = *reinterpret_cast<const float4*>(xrow + v0 + 4);
  x[0] = q0.x; x[1] = q0.y; x[2] = q0.z; x[3] = q0.w; x[4] = q1.x; x[5] = q1.y; x[6] = q1.z; x[7] = q1.w;
}
__global__ __launch_bounds__(TS_THREADS) void ts_sample_kernel(TsPickArgs a) {
  __shared__ float s_v[2][TS_WAVES];
  __shared__ int s_i[TS_WAVES];
  __shared__ float s_sum[2][TS_WAVES];
  __shared__ double s_wtot[TS_NB][TS_WAVES];
  __shared__ double s_own[TS_NB][TS_THREADS], s_pre[TS_NB][TS_THREADS];     // a run's sum / what its wave holds in front of it (2 x 56 KB)
  __shared__ int s_tok, s_last;
  __shared__ float s_px;
  __shared__ int s_ctok[TS_MAX_CAND];
  __shared__ float s_cpx[TS_MAX_CAND];
  __shared__ double s_cu[TS_MAX_CAND];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int step = a.fuse.x ? a.fuse.counters[1] : a.step_dev ? *a.step_dev : 0;
  const int pos = a.fuse.x ? a.fuse.counters[0] + 1 : 0;
  TsState st = a.st[b];
  const int n_cand = a.n_cand;
  if (st.done) {
    if (n_cand > 0) return;             // beam search: a finished decoder draws nothing
    if (tid == 0) {
      a.tokens_out[b] = a.eot;
      a.tokens_all[(long)step * gridDim.x + b] = a.eot;
      a.tids_all[(long)step * gridDim.x + b] = a.beg;
      if (a.plog_all) a.plog_all[(long)step * gridDim.x + b] = 0.f;
    }
    if (a.fuse.x) step_fuse_tail(a.fuse, a.eot, pos, step, b, tid);
    return;
  }
  const float* lg = a.logits + (long)b * a.ld;
  const TsRule rule(a, st);
  const float T = *a.temperature;
  const double u = n_cand > 0 ? 0.0 : a.u_all[(long)step * gridDim.x + b];
  if (tid == 0) { s_tok = -1; s_last = -1; }
  if (tid < n_cand) { s_ctok[tid] = -1; s_cu[tid] = a.u_all[((long)step * gridDim.x + b) * n_cand + tid]; }
  // ---- pass 1: maxima of the text / special ids and of the timestamps ----
  float tv = -INFINITY, xv = -INFINITY;
  int xi = 0x7fffffff;
  // The row as the passes see it (logit / T where the rules allow the id, -inf elsewhere) is evaluated ONCE and parked in
  // xrow (global, this row's TS_NB x TS_BLK floats): passes 2 and 3 read a thread's own eight-id runs back instead of
  // re-deriving them -- the rules and the IEEE division were 44 of the ~126 instructions per id of the three passes.
  float* __restrict__ xrow = a.x_scratch + (long)b * (TS_NB * TS_BLK);
#pragma unroll 1
  for (int jb = 0; jb < TS_NB; ++jb) {
    const int v0 = TS_BLK * jb + TS_E * tid;
    float x[TS_E];
    ts_load_run(rule, lg, a.V, a.eot, T, v0, x);
    *reinterpret_cast<float4*>(xrow + v0) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(xrow + v0 + 4) = make_float4(x[4], x[5], x[6], x[7]);
#pragma unroll
    for (int e = 0; e < TS_E; ++e) {
      if (v0 + e < a.beg) tv = fmaxf(tv, x[e]);
      else if (x[e] > xv) { xv = x[e]; xi = v0 + e; }          // a thread's ids ascend: its first maximum stays
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    tv = fmaxf(tv, __shfl_xor(tv, off, 64));
    const float ov = __shfl_xor(xv, off, 64); const int oi = __shfl_xor(xi, off, 64);
    if (ov > xv || (ov == xv && oi < xi)) { xv = ov; xi = oi; }
  }
  if (lane == 0) { s_v[0][wave] = tv; s_v[1][wave] = xv; s_i[wave] = xi; }
  __syncthreads();
  float max_text = s_v[0][0], max_ts = s_v[1][0];
  int arg_ts = s_i[0];
#pragma unroll
  for (int w = 1; w < TS_WAVES; ++w) {
    max_text = fmaxf(max_text, s_v[0][w]);
    if (s_v[1][w] > max_ts || (s_v[1][w] == max_ts && s_i[w] < arg_ts)) { max_ts = s_v[1][w]; arg_ts = s_i[w]; }
  }
  const float max_all = fmaxf(max_text, max_ts);
  // ---- pass 2: sums of exponentials ----
  float sum_all = 0.f, sum_ts = 0.f;
#pragma unroll 1
  for (int jb = 0; jb < TS_NB; ++jb) {
    const int v0 = TS_BLK * jb + TS_E * tid;
    float x[TS_E];
    ts_read_run(xrow, v0, x);
#pragma unroll
    for (int e = 0; e < TS_E; ++e) {
      if (x[e] == -INFINITY) continue;                         // not allowed, or past the row
      sum_all += expf(x[e] - max_all);
      if (v0 + e >= a.beg) sum_ts += expf(x[e] - max_ts);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { sum_all += __shfl_xor(sum_all, off, 64); sum_ts += __shfl_xor(sum_ts, off, 64); }
  if (lane == 0) { s_sum[0][wave] = sum_all; s_sum[1][wave] = sum_ts; }
  __syncthreads();
  float tot_all = 0.f, tot_ts = 0.f;
#pragma unroll
  for (int w = 0; w < TS_WAVES; ++w) { tot_all += s_sum[0][w]; tot_ts += s_sum[1][w]; }
  const float lse_all = max_all + logf(tot_all);
  const float lse_ts = max_ts > -INFINITY ? max_ts + logf(tot_ts) : -INFINITY;
  const bool ts_only = lse_ts > max_text;                      // the probability-mass rule
  // ---- pass 3: probabilities, eight-id sums per block, and per block an inclusive scan over the wave ----
  int last_pos = -1;
#pragma unroll 1
  for (int jb = 0; jb < TS_NB; ++jb) {
    const int v0 = TS_BLK * jb + TS_E * tid;
    float x[TS_E];
    ts_read_run(xrow, v0, x);
    double sj = 0.0;
#pragma unroll
    for (int e = 0; e < TS_E; ++e) {
      float p = 0.f;
      if (x[e] != -INFINITY && !(ts_only && v0 + e < a.beg)) p = expf(x[e] - lse_all);
      if (p > 0.f) { sj += (double)p; last_pos = v0 + e; }
    }
    double in = sj;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double o = __shfl_up(in, off, 64);
      if (lane >= off) in += o;
    }
    s_own[jb][tid] = sj;
    s_pre[jb][tid] = in - sj;
    if (lane == 63) s_wtot[jb][wave] = in;
  }
  if (last_pos >= 0) atomicMax(&s_last, last_pos);
  __syncthreads();
  double total = 0.0;
#pragma unroll
  for (int jb = 0; jb < TS_NB; ++jb)
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) total += s_wtot[jb][w];
  // the run whose interval (cum before, cum after] / total contains u is walked by its thread; the last id with any
  // probability closes at 1.0.  id order = (block, wave, lane, element).
  const int glast = s_last;
  double run = 0.0;                  // everything of the blocks before jb
#pragma unroll 1
  for (int jb = 0; jb < TS_NB; ++jb) {
    double front = run;              // + the waves of this block before mine
#pragma unroll
    for (int w = 0; w < TS_WAVES; ++w) {
      if (w < wave) front += s_wtot[jb][w];
      run += s_wtot[jb][w];
    }
    const double own = s_own[jb][tid];
    if (!(own > 0.0)) continue;
    const double before = front + s_pre[jb][tid], after = before + own;
    const int v0 = TS_BLK * jb + TS_E * tid;
    const bool owns_last = glast >= v0 && glast < v0 + TS_E;
    const double lo = before / total, hi = owns_last ? 1.0 : after / total;
    // the walk of this run for one variate
    auto walk = [&](double uu, int* tok_out, float* px_out) {
      double c = before;
      int pick = -1;
      float px = 0.f;
      for (int e = 0; e < TS_E; ++e) {
        const int v = v0 + e;
        if (pick >= 0 || v >= a.V || (ts_only && v < a.beg) || !rule.allowed(v, a.eot)) continue;
        const float x = lg[v] / T;
        const float p = expf(x - lse_all);
        if (!(p > 0.f)) continue;
        c += (double)p;
        if (c / total >= uu || v == glast) { pick = v; px = x; }
      }
      if (pick < 0) { pick = glast; px = lg[glast] / T; }      // (rounding: the run's last id)
      *tok_out = pick;
      *px_out = px;
    };
    if (n_cand > 0) {
      for (int k = 0; k < n_cand; ++k) {
        const double uk = s_cu[k];
        if (lo < uk && uk <= hi) walk(uk, &s_ctok[k], &s_cpx[k]);
      }
    } else if (lo < u && u <= hi) {
      walk(u, &s_tok, &s_px);
    }
  }
  __syncthreads();
  if (n_cand > 0) {
    if (tid < n_cand) {
      int pick = s_ctok[tid];
      float px = s_cpx[tid];
      if (pick < 0) {                   // the variate fell between two runs' rounded interval ends: the last id with any probability
        pick = s_last >= 0 ? s_last : a.eot;
        px = lg[pick] / T;
      }
      a.cand_tok[(long)b * n_cand + tid] = pick;
      a.cand_plog[(long)b * n_cand + tid] = px - lse_all;
      a.cand_tid[(long)b * n_cand + tid] = pick >= a.beg ? pick : (max_ts > -INFINITY ? arg_ts : a.beg);
    }
    return;
  }
  if (tid == 0) {
    int pick = s_tok;
    float px = s_px;
    if (pick < 0) {                     // u fell between two runs' rounded interval ends: the last id with any probability
      pick = s_last >= 0 ? s_last : a.eot;
      px = lg[pick] / T;
    }
    const int tsid = pick >= a.beg ? pick : (max_ts > -INFINITY ? arg_ts : a.beg);
    ts_commit(a, st, b, step, pick, tsid, px - lse_all);
    s_tok = pick;
  }
  if (a.fuse.x) {
    __syncthreads();
    step_fuse_tail(a.fuse, s_tok, pos, step, b, tid);
  }
}

// beam_kv_reorder: phase 0 gathers the parents' bytes into scratch, phase 1 scatters them into the rows.  The bytes are the
// cache rows of the positions generated so far, [counters[4], counters[0]) -- read on the device: the launch is part of a
// captured step; counters[5] = max_new of the pass, the scratch rows' pitch in positions.
__global__ __launch_bounds__(256) void beam_kv_copy_kernel(char* __restrict__ kv, char* __restrict__ scratch, const int* __restrict__ parent,
                                                           int rows, long row_bytes, long pos_bytes, const int* __restrict__ counters,
                                                           int phase) {
  const int r = blockIdx.x, l = blockIdx.y;
  const int p = parent[r];
  if (p == r) return;
  const int pos0 = counters[4];
  const long len = (long)(counters[0] - pos0) * pos_bytes, scratch_stride = (long)counters[5] * pos_bytes;
  char* row = kv + ((long)l * rows + (phase == 0 ? p : r)) * row_bytes + (long)pos0 * pos_bytes;
  char* tmp = scratch + ((long)l * rows + r) * scratch_stride;
  for (long x = 16L * (blockIdx.z * 256 + threadIdx.x); x < len; x += 16L * 256 * gridDim.z) {
    if (phase == 0) *reinterpret_cast<uint4*>(tmp + x) = *reinterpret_cast<const uint4*>(row + x);
    else *reinterpret_cast<uint4*>(row + x) = *reinterpret_cast<const uint4*>(tmp + x);
  }
}

// One step of whisper_full's beam search for one clip (BeamArgs, asr_common.h): one wave, lane = candidate (decoder j, draw k).
__global__ __launch_bounds__(64) void beam_advance_kernel(BeamArgs a) {
  __shared__ BeamRow s_row[TS_MAX_CAND];
  __shared__ TsState s_st[TS_MAX_CAND];
  __shared__ double s_sum[64];
  __shared__ int s_tok[64], s_tid[64], s_sorted[64], s_deal[TS_MAX_CAND], s_feed[TS_MAX_CAND];
  __shared__ float s_plog[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int n_dec = a.n_dec, n_cand = a.n_cand, r0 = c * n_dec;
  const int step = a.counters[1], pos = a.counters[0] + 1;
  if (lane < n_dec) { s_row[lane] = a.row[r0 + lane]; s_st[lane] = a.st[r0 + lane]; }
  __syncthreads();
  // the candidates of the clip's live decoders and the sum of ALL log-probabilities each would have
  const int j = lane / n_cand, k = lane - j * n_cand;
  const bool valid = j < n_dec && !(s_row[j < n_dec ? j : 0].completed || s_row[j < n_dec ? j : 0].failed);
  int tok = -1, tid = 0;
  float plog = 0.f;
  double sum = 0.0;
  if (valid) {
    const long x = (long)(r0 + j) * n_cand + k;
    tok = a.cand_tok[x]; tid = a.cand_tid[x]; plog = a.cand_plog[x];
    sum = s_row[j].sum_all + (double)plog;
  }
  s_tok[lane] = tok; s_tid[lane] = tid; s_plog[lane] = plog; s_sum[lane] = sum;
  const unsigned long long vmask = __ballot(valid);
  const int n_valid = __popcll(vmask);
  // std::stable_sort by (sum descending, decoder ascending) over candidates pushed decoder-major: position = the number of
  // candidates that come first = those with a larger sum, or an equal one and a smaller lane
  int rank = 0;
  for (int l = 0; l < 64; ++l) {
    const double sl = __shfl(sum, l, 64);
    if (((vmask >> l) & 1ull) && (sl > sum || (sl == sum && l < lane))) ++rank;
  }
  if (valid) s_sorted[rank] = lane;
  __syncthreads();
  // deal the sorted candidates to the live decoders, skipping repeats of the sequence just dealt (not at the first step):
  // two candidates are the same sequence when their ids are equal and their decoders' sequences are (BeamRow::eqid)
  if (lane == 0) {
    int cur_c = 0;
    for (int d = 0; d < n_dec; ++d) {
      s_deal[d] = -1;
      if (s_row[d].completed || s_row[d].failed || n_valid == 0) continue;
      if (cur_c >= n_valid) cur_c = 0;
      const int cur = s_sorted[cur_c++];
      const int cj = cur / n_cand;
      while (cur_c < n_valid && step > 0) {
        const int nx = s_sorted[cur_c], nj = nx / n_cand;
        if (!(s_tok[nx] == s_tok[cur] && (nj == cj || s_row[nj].eqid == s_row[cj].eqid))) break;
        ++cur_c;
      }
      s_deal[d] = cur;
    }
  }
  __syncthreads();
  int died = 0;
  if (lane < n_dec) {
    const int r = r0 + lane, cur = s_deal[lane];
    int feed = a.eot;
    if (cur < 0) {                               // ended in an earlier step: keeps its sequence and its cache rows
      a.parent[r] = r;
    } else {
      const int pj = cur / n_cand, t = s_tok[cur];
      BeamRow q = s_row[pj];
      TsState st = s_st[pj];
      q.sum_all = s_sum[cur];
      q.n += 1;
      st.prev = st.last; st.last = t; st.n += 1;                   // the rules' view of the sequence (the pick kernel's ts_commit)
      if (a.rules == TS_RULES_OPENAI ? t >= a.beg : t > a.beg) st.last_ts = t;
      // the sequence's class among the decoders dealt this step: the first decoder dealt the same parent class and id
      int eq = lane;
      for (int d = 0; d < lane; ++d) {
        const int od = s_deal[d];
        if (od >= 0 && s_tok[od] == t && s_row[od / n_cand].eqid == s_row[pj].eqid) { eq = d; break; }
      }
      q.eqid = eq;
      const long x = (long)step * a.rows + r;
      a.rec_tok[x] = t; a.rec_tid[x] = s_tid[cur]; a.rec_plog[x] = s_plog[cur]; a.rec_parent[x] = r0 + pj;
      a.parent[r] = r0 + pj;
      // completion / failure on the new last token (whisper_full's bookkeeping of a decoder)
      bool live = true;
      if (t > a.beg) {
        const int sd = 2 * (t - a.beg);
        if (q.has_ts && q.seek_delta > sd && q.result_len < step) { q.failed = 1; live = false; }      // "do not allow to go back in time"
        else { q.seek_delta = sd; q.result_len = step + 1; q.has_ts = 1; }
      }
      if (live && (t == a.eot || (q.has_ts && st.seek + q.seek_delta + a.delta_min >= st.seek_end))) {
        if (q.result_len == 0) {
          if (st.seek + q.seek_delta + a.delta_min >= st.seek_end) q.result_len = step + 1;
          else { q.failed = 1; live = false; }
        }
        if (live) { q.completed = 1; live = false; }
      }
      if (live && step == a.counters[5] - 1 && (q.result_len == 0 || q.seek_delta < 1500)) { q.failed = 1; live = false; }
      st.done = live ? 0 : 1;
      if (live) feed = t; else died = 1;
      a.row[r] = q;
      a.st[r] = st;
    }
    a.feed[r] = feed;
    s_feed[lane] = feed;
  }
  const int n_died = __popcll(__ballot(died != 0));
  if (lane == 0 && n_died) atomicAdd(a.done_count, n_died);
  if (!a.fuse.x) return;
  __syncthreads();
  for (int d = 0; d < n_dec; ++d) step_fuse_embed(a.fuse, s_feed[d], pos, r0 + d, lane);
  step_fuse_ticket(a.fuse, pos, step, lane);
}

// p_out[b] = softmax(row b)[token]: one 1024-thread block per row, two passes (maximum, sum of exponentials)
__global__ __launch_bounds__(1024) void softmax_prob_kernel(const float* __restrict__ logits, int V, long ld, int token, float* __restrict__ p_out) {
  __shared__ float s_r[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (long)b * ld;
  float m = -INFINITY;
  for (int v = tid; v < V; v += 1024) m = fmaxf(m, lg[v]);
  m = shfl_max(m);
  if ((tid & 63) == 0) s_r[tid >> 6] = m;
  __syncthreads();
  m = s_r[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) m = fmaxf(m, s_r[w]);
  __syncthreads();
  float sum = 0.f;
  for (int v = tid; v < V; v += 1024) sum += expf(lg[v] - m);
  sum = shfl_sum(sum);
  if ((tid & 63) == 0) s_r[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += s_r[w];
    p_out[b] = expf(lg[token] - m - logf(tot));
  }
}

}  // namespace

hipError_t embed_tokens_f32(const int* tokens, const float* tok_emb, const float* pos_emb, int pos, const int* pos_dev,
                            float* x, int B, int D, hipStream_t s, int rows_per_clip, const int* row_off) {
  hipLaunchKernelGGL(embed_kernel, dim3(B), dim3(256), 0, s, tokens, tok_emb, pos_emb, pos, pos_dev, x, D, rows_per_clip < 1 ? 1 : rows_per_clip, row_off);
  return hipGetLastError();
}
hipError_t argmax_f32(const float* logits, const unsigned char* mask, const unsigned char* mask_first,
                      const int* step_dev, int V, long ld, int* tokens_out, int* tokens_all, float* best, int B, hipStream_t s,
                      int eot, int* finished, int* done_count, const StepFuse* fuse) {
  hipLaunchKernelGGL(argmax_kernel, dim3(B), dim3(1024), 0, s, logits, mask, mask_first, step_dev, V, ld, tokens_out,
                     tokens_all, best, eot, finished, done_count, fuse ? *fuse : StepFuse{});
  return hipGetLastError();
}
hipError_t softmax_prob_f32(const float* logits, int V, long ld, int token, float* p_out, int B, hipStream_t s) {
  if (token < 0 || token >= V) return hipErrorInvalidValue;
  hipLaunchKernelGGL(softmax_prob_kernel, dim3(B), dim3(1024), 0, s, logits, V, ld, token, p_out);
  return hipGetLastError();
}

hipError_t beam_kv_reorder(void* kv, void* scratch, const int* parent_dev, int layers, int rows, long row_bytes, long pos_bytes,
                           const int* counters, hipStream_t s) {
  if (pos_bytes % 16 != 0 || row_bytes % 16 != 0) return hipErrorInvalidValue;
  for (int phase = 0; phase < 2; ++phase)
    hipLaunchKernelGGL(beam_kv_copy_kernel, dim3(rows, layers, 8), dim3(256), 0, s, reinterpret_cast<char*>(kv),
                       reinterpret_cast<char*>(scratch), parent_dev, rows, row_bytes, pos_bytes, counters, phase);
  return hipGetLastError();
}

hipError_t beam_advance(const BeamArgs& a, int n_clips, hipStream_t s) {
  if (a.n_dec < 1 || a.n_dec > TS_MAX_CAND || a.n_cand < 1 || a.n_cand > TS_MAX_CAND || a.n_dec * a.n_cand > 64 || n_clips < 1 ||
      a.rows != n_clips * a.n_dec)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_advance_kernel, dim3(n_clips), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t ts_pick(const TsPickArgs& a, int B, hipStream_t s) {
  if (a.n_cand < 0 || a.n_cand > TS_MAX_CAND || (a.n_cand > 0 && !(a.u_all && a.cand_tok && a.cand_plog && a.cand_tid))) return hipErrorInvalidValue;
  if (a.u_all) {
    if (!a.temperature || !a.x_scratch || a.V > TS_BLK * TS_NB) return hipErrorInvalidValue;      // a thread's ids: TS_NB runs of TS_E
    hipLaunchKernelGGL(ts_sample_kernel, dim3(B), dim3(TS_THREADS), 0, s, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(ts_pick_kernel, dim3(B), dim3(1024), 0, s, a);
  return hipGetLastError();
}

}  // namespace crispy

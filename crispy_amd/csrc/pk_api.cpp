// pk_api.cpp -- host side of the Parakeet FastConformer encoder (include/crispy_hip.h, "Parakeet encoder"; kernels in pk_sub.hip,
// pk_gemm.hip, pk_gemm_f16.hip, pk_attn.hip and pk_attn_f16.hip): the tensor table of crispy_pk_tensor_spec and crispy_pk_load, the folds and the layout of the
// handle's device copy, precision mode 1's f16 copies of the GEMM weights, the workspace and the launches of a call; and crispy_pk_transcribe ("Parakeet front end"), which joins the
// front end (pk_mel_api.cpp), the encoder and the decoder (pk_tdt_api.cpp) in one call.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "api_util.h"
#include "pk_internal.h"

using crispy::fail;
using namespace crispy::pk;

namespace {

const crispy_pk_config* as_cfg(const void* p) { return static_cast<const crispy_pk_config*>(p); }

// the supported set; a field outside it is named
int check_config(const char* who, const crispy_pk_config* c) {
  if (!c) return fail(CRISPY_ERR_INVALID_ARG, "%s: cfg is NULL", who);
  if (c->heads < 1 || c->heads > 16) return fail(CRISPY_ERR_INVALID_ARG, "%s: heads %d outside 1 ... 16", who, c->heads);
  if (c->hidden != kHeadDim * c->heads) return fail(CRISPY_ERR_INVALID_ARG, "%s: hidden %d is not 128 x heads (%d)", who, c->hidden, c->heads);
  if (c->layers < 1 || c->layers > 64) return fail(CRISPY_ERR_INVALID_ARG, "%s: layers %d outside 1 ... 64", who, c->layers);
  if (c->ffn < 128 || c->ffn > 16384 || c->ffn % 128 != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: ffn %d is not a multiple of 128 in 128 ... 16384", who, c->ffn);
  if (c->conv_kernel < 3 || c->conv_kernel > kMaxTaps || c->conv_kernel % 2 == 0)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: conv_kernel %d is not odd in 3 ... %d", who, c->conv_kernel, kMaxTaps);
  if (c->mel_bins < 8 || c->mel_bins > 256 || c->mel_bins % 8 != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: mel_bins %d is not a multiple of 8 in 8 ... 256", who, c->mel_bins);
  if (c->sub_channels < 32 || c->sub_channels > kMaxSubCh || c->sub_channels % 32 != 0)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: sub_channels %d is not a multiple of 32 in 32 ... %d", who, c->sub_channels, kMaxSubCh);
  if ((c->attention_bias | 1) != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: attention_bias %d is neither 0 nor 1", who, c->attention_bias);
  if ((c->convolution_bias | 1) != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: convolution_bias %d is neither 0 nor 1", who, c->convolution_bias);
  if ((c->scale_input | 1) != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: scale_input %d is neither 0 nor 1", who, c->scale_input);
  return CRISPY_OK;
}

// ---- the tensors crispy_pk_load takes, in the order of ParakeetEncoder's state dict -------------------------------------
struct Spec {
  std::string name;
  size_t count;
};

void push_linear(std::vector<Spec>& s, const std::string& p, size_t out, size_t in, bool bias) {
  s.push_back({p + ".weight", out * in});
  if (bias) s.push_back({p + ".bias", out});
}

std::vector<Spec> make_specs(const crispy_pk_config& c) {
  std::vector<Spec> s;
  const size_t H = (size_t)c.hidden, C = (size_t)c.sub_channels, F = (size_t)c.ffn, K = (size_t)c.conv_kernel;
  const bool ab = c.attention_bias != 0, cb = c.convolution_bias != 0;
  push_linear(s, "subsampling.layers.0", C, 9, true);
  for (int i = 0; i < 2; ++i) {
    push_linear(s, "subsampling.layers." + std::to_string(2 + 3 * i), C, 9, true);
    push_linear(s, "subsampling.layers." + std::to_string(3 + 3 * i), C, C, true);
  }
  push_linear(s, "subsampling.linear", H, C * (size_t)(c.mel_bins / 8), true);
  for (int l = 0; l < c.layers; ++l) {
    const std::string p = "layers." + std::to_string(l) + ".";
    auto ff = [&](const std::string& q) {
      push_linear(s, q + ".linear1", F, H, ab);
      push_linear(s, q + ".linear2", H, F, ab);
    };
    ff(p + "feed_forward1");
    s.push_back({p + "self_attn.bias_u", H});
    s.push_back({p + "self_attn.bias_v", H});
    for (const char* q : {"q_proj", "k_proj", "v_proj", "o_proj"}) push_linear(s, p + "self_attn." + q, H, H, ab);
    push_linear(s, p + "self_attn.relative_k_proj", H, H, false);
    push_linear(s, p + "conv.pointwise_conv1", 2 * H, H, cb);
    push_linear(s, p + "conv.depthwise_conv", H, K, cb);
    for (const char* q : {"weight", "bias", "running_mean", "running_var"}) s.push_back({p + "conv.norm." + q, H});
    push_linear(s, p + "conv.pointwise_conv2", H, H, cb);
    ff(p + "feed_forward2");
    for (const char* q : {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"}) push_linear(s, p + q, H, 1, true);
  }
  return s;
}

// ---- the device copy ------------------------------------------------------------------------------------------------
// Visits every field of the model in a fixed order with its element count: once to add up the size, once to place the fields.
template <class V>
void walk(PkModel& m, const crispy_pk_config& c, V&& v) {
  const size_t H = (size_t)c.hidden, C = (size_t)c.sub_channels, F = (size_t)c.ffn, K = (size_t)c.conv_kernel;
  v(m.conv0_w, 9 * C);
  v(m.conv0_b, C);
  for (int i = 0; i < 2; ++i) {
    v(m.dw_w[i], 9 * C);
    v(m.dw_b[i], C);
    v(m.pw_w[i], C * C);
    v(m.pw_b[i], C);
  }
  v(m.lin_w, C * (size_t)(c.mel_bins / 8) * H);
  v(m.lin_b, H);
  v(m.inv_freq, H / 2);
  m.layer.resize((size_t)c.layers);
  for (PkLayer& l : m.layer) {
    for (int i = 0; i < 5; ++i) {
      v(l.ln_g[i], H);
      v(l.ln_b[i], H);
    }
    for (int i = 0; i < 2; ++i) {
      v(l.ff_w1[i], H * F);
      v(l.ff_b1[i], F);
      v(l.ff_w2[i], F * H);
      v(l.ff_b2[i], H);
    }
    v(l.qkv_w, H * 3 * H);
    v(l.qkv_b, 3 * H);
    v(l.o_w, H * H);
    v(l.o_b, H);
    v(l.r_w, H * H);
    v(l.bias_u, H);
    v(l.bias_v, H);
    v(l.pw1_w, H * 2 * H);
    v(l.pw1_b, 2 * H);
    v(l.dw_w, K * H);
    v(l.dw_scale, H);
    v(l.dw_shift, H);
    v(l.pw2_w, H * H);
    v(l.pw2_b, H);
  }
}

size_t model_floats(const crispy_pk_config& c) {
  PkModel m{};
  size_t at = 0;
  walk(m, c, [&at](const float*&, size_t n) { at += (n + 63) & ~(size_t)63; });      // every tensor starts on a 256-byte boundary
  return at;
}

PkModel model_of(const float* base, const crispy_pk_config& c) {
  PkModel m{};
  size_t at = 0;
  walk(m, c, [&at, base](const float*& f, size_t n) {
    f = base + at;
    at += (n + 63) & ~(size_t)63;
  });
  return m;
}

float* wr(const float* p) { return const_cast<float*>(p); }      // the host copy is written through the model's pointers

// torch's [out][in][taps] -> [(tap * in_n + in)][ld] at column col0 + out
void put_transposed(const float* src, size_t out_n, size_t in_n, size_t taps, const float* dst, size_t ld, size_t col0) {
  for (size_t o = 0; o < out_n; ++o)
    for (size_t i = 0; i < in_n; ++i)
      for (size_t k = 0; k < taps; ++k) wr(dst)[(k * in_n + i) * ld + col0 + o] = src[(o * in_n + i) * taps + k];
}

// ---- mode 1's f16 copies of the GEMM weights ------------------------------------------------------------------------------
// Visits every matrix that launch_gemm multiplies by in a call, in a fixed order, with its f16 slot and its [K][cols] shape.
template <class V>
void walk_half(const PkModel& m, PkHalfModel& hm, const crispy_pk_config& c, V&& v) {
  const size_t H = (size_t)c.hidden, F = (size_t)c.ffn;
  v(m.lin_w, hm.lin_w, (size_t)c.sub_channels * (size_t)(c.mel_bins / 8), H);
  hm.layer.resize((size_t)c.layers);
  for (size_t li = 0; li < hm.layer.size(); ++li) {
    const PkLayer& l = m.layer[li];
    PkHalfLayer& h = hm.layer[li];
    for (int i = 0; i < 2; ++i) {
      v(l.ff_w1[i], h.ff_w1[i], H, F);
      v(l.ff_w2[i], h.ff_w2[i], F, H);
    }
    v(l.qkv_w, h.qkv_w, H, 3 * H);
    v(l.o_w, h.o_w, H, H);
    v(l.r_w, h.r_w, H, H);
    v(l.pw1_w, h.pw1_w, H, 2 * H);
    v(l.pw2_w, h.pw2_w, H, H);
  }
}

size_t half_bytes(const crispy_pk_config& c) {
  PkModel m{};      // only the shapes are visited
  m.layer.resize((size_t)c.layers);
  PkHalfModel hm;
  size_t at = 0;
  walk_half(m, hm, c, [&at](const float*, const void*&, size_t K, size_t N) { at += (K * N * 2 + 255) & ~(size_t)255; });
  return at;
}

PkHalfModel half_of(const char* base, const PkModel& m, const crispy_pk_config& c) {      // base == NULL (mode 0): every slot NULL
  PkHalfModel hm;
  size_t at = 0;
  walk_half(m, hm, c, [&at, base](const float*, const void*& p, size_t K, size_t N) {
    p = base ? base + at : nullptr;
    at += (K * N * 2 + 255) & ~(size_t)255;
  });
  return hm;
}

// Packs the f16 copies of the model at `weights` into a fresh allocation, on the device, and waits.  The size is checked against
// the device's free memory first: CRISPY_ERR_OOM leaves `out` as it was with nothing enqueued.
int pack_half(const char* who, const float* weights, const crispy_pk_config& cfg, hipStream_t st, crispy::DevBuf<char>& out) {
  const size_t need = half_bytes(cfg);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b) return fail(CRISPY_ERR_OOM, "%s: the f16 copies of the weights need %zu bytes, the device has %zu free", who, need, free_b);
  crispy::DevBuf<char> fresh;
  HIP_TRY(fresh.alloc(need));
  const PkModel m = model_of(weights, cfg);
  PkHalfModel hm = half_of(fresh.p, m, cfg);
  hipError_t err = hipSuccess;
  walk_half(m, hm, cfg, [&](const float* src, const void*& dst, size_t K, size_t N) {
    if (err == hipSuccess) err = launch_pack_f16(src, (int)K, (int)N, const_cast<void*>(dst), st);
  });
  HIP_TRY(err);
  HIP_TRY(hipStreamSynchronize(st));
  out = std::move(fresh);
  return CRISPY_OK;
}

// ---- a call's workspace ---------------------------------------------------------------------------------------------
struct Carve {      // pieces on 256-byte boundaries; with p == NULL it only adds up the size
  char* p = nullptr;
  size_t used = 0;
  template <class T> T* take(size_t n) {
    T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};

struct Work {
  int* tab;                                  // off[4][n_clips + 1]
  float *img1, *img2, *flat;                 // [T1][M/2][C], [T2][M/4][C], [T'][C * M/8]
  float *x, *ln, *big, *mid, *pos, *r;       // [T'][H], [T'][H], [T'][max(ffn, 3H)], [T'][H], [2 tmax - 1][H] twice
};

void carve(Carve& c, Work& w, const crispy_pk_config& cfg, const size_t len[4], size_t n_clips, size_t tmax) {
  const size_t H = (size_t)cfg.hidden, C = (size_t)cfg.sub_channels, M = (size_t)cfg.mel_bins;
  w.tab = c.take<int>(4 * (n_clips + 1));
  w.img1 = c.take<float>(len[1] * (M / 2) * C);
  w.img2 = c.take<float>(len[2] * (M / 4) * C);
  w.flat = c.take<float>(len[3] * (M / 8) * C);
  w.x = c.take<float>(len[3] * H);
  w.ln = c.take<float>(len[3] * H);
  w.big = c.take<float>(len[3] * std::max((size_t)cfg.ffn, 3 * H));
  w.mid = c.take<float>(len[3] * H);
  w.pos = c.take<float>((2 * tmax - 1) * H);
  w.r = c.take<float>((2 * tmax - 1) * H);
}

// Developer aid (CRISPY_PK_TIMELINE in the dev build): device time of a call by stage, to stderr.
enum Stage { kStSub, kStGemm, kStAttn, kStConv, kStNorm, kStCount };
struct Timeline {
  bool on = false;
  crispy::EventList ev;
  std::vector<int> stage;      // stage[i]: what ran between event i - 1 and event i
  hipError_t mark(int s, hipStream_t st) {
    if (!on) return hipSuccess;
    hipError_t e = ev.ensure(ev.v.size() + 1, 0);
    if (e != hipSuccess) return e;
    stage.push_back(s);
    return hipEventRecord(ev.v.back(), st);
  }
  void report() const {
    if (!on) return;
    double ms[kStCount] = {};
    for (size_t i = 1; i < ev.v.size(); ++i) {
      float t = 0.0f;
      if (stage[i] >= 0 && hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[stage[i]] += t;
    }
    std::fprintf(stderr, "crispy_pk timeline: subsampling %.3f ms, gemms %.3f ms, attention %.3f ms, convolution %.3f ms, layernorm %.3f ms\n",
                 ms[kStSub], ms[kStGemm], ms[kStAttn], ms[kStConv], ms[kStNorm]);
  }
};

int check_call(const char* who, const crispy_pk* h, const long* frame_offset, int n_clips, int tap_layer, const void* d_tap) {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (n_clips < 1 || n_clips > kMaxClips) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_clips %d outside 1 ... %d", who, n_clips, kMaxClips);
  if (!frame_offset) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset is NULL", who);
  if (frame_offset[0] != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset[0] is %ld, not 0", who, frame_offset[0]);
  for (int c = 0; c < n_clips; ++c) {
    const long n = frame_offset[c + 1] - frame_offset[c];
    if (n < 1 || n > kMaxRows) return fail(CRISPY_ERR_INVALID_ARG, "%s: clip %d has %ld rows, outside 1 ... %d", who, c, n, kMaxRows);
  }
  if (!h->weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no encoder is loaded (crispy_pk_load comes first)", who);
  if (d_tap && (tap_layer < 0 || tap_layer >= h->cfg.layers))
    return fail(CRISPY_ERR_INVALID_ARG, "%s: tap_layer %d outside 0 ... %d", who, tap_layer, h->cfg.layers - 1);
  return CRISPY_OK;
}

// The encoder on n_clips clips of feature rows; the arguments have been checked.  With `wait` the call is complete on return;
// without, it is enqueued (crispy_pk_transcribe: the decoder's stream waits for an event instead).
int pk_run(crispy_pk* h, const float* d_feats, const long* frame_offset, int n_clips, float* d_out, float* d_sub, int tap_layer, float* d_tap,
           float* d_pos, hipStream_t st, bool wait = true) {
  const crispy_pk_config& cfg = h->cfg;
  const int H = cfg.hidden, C = cfg.sub_channels, M = cfg.mel_bins;
  std::vector<int> tab((size_t)4 * (n_clips + 1), 0);
  size_t len[4] = {0, 0, 0, 0};
  PkTables tb{};
  tb.n_clips = n_clips;
  for (int c = 0; c < n_clips; ++c) {
    long n = frame_offset[c + 1] - frame_offset[c];
    for (int s = 0; s < 4; ++s) {
      len[s] += (size_t)n;
      tb.max_len[s] = std::max(tb.max_len[s], (int)n);
      tab[(size_t)s * (n_clips + 1) + c + 1] = (int)len[s];
      n = sub_len(n);
    }
  }
  const int tmax = tb.max_len[3];
  Carve size;
  Work w{};
  carve(size, w, cfg, len, (size_t)n_clips, (size_t)tmax);
  if (size.used > h->scratch.bytes) {      // before any launch: what does not fit is refused with nothing enqueued
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (size.used > free_b + h->scratch.bytes)
      return fail(CRISPY_ERR_OOM, "crispy_pk_encode: the call needs a workspace of %zu bytes, the device has %zu free", size.used, free_b + h->scratch.bytes);
    HIP_TRY(h->scratch.grow(size.used));
  }
  Carve place;
  place.p = h->scratch.p;
  carve(place, w, cfg, len, (size_t)n_clips, (size_t)tmax);
  for (int s = 0; s < 4; ++s) tb.off[s] = w.tab + (size_t)s * (n_clips + 1);
  const PkModel m = model_of(h->weights.p, cfg);
  const int mode = h->precision;      // 1: crispy_pk_set_precision or crispy_pk_load packed the f16 copies
  const PkHalfModel hm = half_of(mode == 1 ? h->weights16.p : nullptr, m, cfg);
  const long T = (long)len[3];
  Timeline tl;
  tl.on = crispy::dev_env("CRISPY_PK_TIMELINE") != nullptr;
  HIP_TRY(hipMemcpyAsync(w.tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(tl.mark(-1, st));
  HIP_TRY(launch_sub_conv0(m, tb, d_feats, M, C, w.img1, st));
  HIP_TRY(launch_sub_dwpw(1, m, tb, w.img1, M / 2, C, w.img2, false, st));
  HIP_TRY(launch_sub_dwpw(2, m, tb, w.img2, M / 4, C, w.flat, true, st));
  HIP_TRY(tl.mark(kStSub, st));
  HIP_TRY(launch_gemm(mode, kGemmScale, w.flat, C * (M / 8), m.lin_w, hm.lin_w, m.lin_b, H, cfg.scale_input ? std::sqrt((float)H) : 1.0f, nullptr, w.x, T, st));
  float* pos = d_pos ? d_pos : w.pos;
  HIP_TRY(launch_pos_table(m.inv_freq, tmax, H, pos, st));
  HIP_TRY(tl.mark(kStGemm, st));
  if (d_sub) HIP_TRY(hipMemcpyAsync(d_sub, w.x, (size_t)T * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  for (int li = 0; li < cfg.layers; ++li) {
    const PkLayer& l = m.layer[(size_t)li];
    const PkHalfLayer& lh = hm.layer[(size_t)li];
    auto ff = [&](int i) -> int {
      HIP_TRY(launch_layernorm(w.x, l.ln_g[i ? 3 : 0], l.ln_b[i ? 3 : 0], w.ln, T, H, st));
      HIP_TRY(tl.mark(kStNorm, st));
      HIP_TRY(launch_gemm(mode, kGemmSilu, w.ln, H, l.ff_w1[i], lh.ff_w1[i], l.ff_b1[i], cfg.ffn, 1.0f, nullptr, w.big, T, st));
      HIP_TRY(launch_gemm(mode, kGemmResidual, w.big, cfg.ffn, l.ff_w2[i], lh.ff_w2[i], l.ff_b2[i], H, 0.5f, w.x, w.x, T, st));
      HIP_TRY(tl.mark(kStGemm, st));
      return CRISPY_OK;
    };
    int rc = ff(0);
    if (rc != CRISPY_OK) return rc;
    HIP_TRY(launch_layernorm(w.x, l.ln_g[1], l.ln_b[1], w.ln, T, H, st));
    HIP_TRY(tl.mark(kStNorm, st));
    HIP_TRY(launch_gemm(mode, kGemmScale, w.ln, H, l.qkv_w, lh.qkv_w, l.qkv_b, 3 * H, 1.0f, nullptr, w.big, T, st));
    HIP_TRY(launch_gemm(mode, kGemmScale, pos, H, l.r_w, lh.r_w, nullptr, H, 1.0f, nullptr, w.r, 2L * tmax - 1, st));
    HIP_TRY(tl.mark(kStGemm, st));
    HIP_TRY(launch_attention(h->attn_precision, l, tb, w.big, w.r, tmax, cfg.heads, w.mid, st));
    HIP_TRY(tl.mark(kStAttn, st));
    HIP_TRY(launch_gemm(mode, kGemmResidual, w.mid, H, l.o_w, lh.o_w, l.o_b, H, 1.0f, w.x, w.x, T, st));
    HIP_TRY(tl.mark(kStGemm, st));
    HIP_TRY(launch_layernorm(w.x, l.ln_g[2], l.ln_b[2], w.ln, T, H, st));
    HIP_TRY(tl.mark(kStNorm, st));
    HIP_TRY(launch_gemm(mode, kGemmGlu, w.ln, H, l.pw1_w, lh.pw1_w, l.pw1_b, H, 1.0f, nullptr, w.mid, T, st));
    HIP_TRY(tl.mark(kStGemm, st));
    HIP_TRY(launch_dwconv(l, tb, w.mid, H, cfg.conv_kernel, w.ln, st));
    HIP_TRY(tl.mark(kStConv, st));
    HIP_TRY(launch_gemm(mode, kGemmResidual, w.ln, H, l.pw2_w, lh.pw2_w, l.pw2_b, H, 1.0f, w.x, w.x, T, st));
    HIP_TRY(tl.mark(kStGemm, st));
    rc = ff(1);
    if (rc != CRISPY_OK) return rc;
    const bool last = li == cfg.layers - 1;
    HIP_TRY(launch_layernorm(w.x, l.ln_g[4], l.ln_b[4], last ? d_out : w.x, T, H, st));
    HIP_TRY(tl.mark(kStNorm, st));
    if (d_tap && li == tap_layer)
      HIP_TRY(hipMemcpyAsync(d_tap, last ? d_out : w.x, (size_t)T * H * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (wait || tl.on) HIP_TRY(hipStreamSynchronize(st));
  tl.report();
  return CRISPY_OK;
}

// ---- crispy_pk_transcribe: features, encoder and decoder in one call ------------------------------------------------------
struct Chain {
  std::vector<long> row_off, frame_off;      // [n_clips + 1] each
  long budget = 0;                           // rows of the step log
};

// Everything that refuses a call, before anything is enqueued.
int check_transcribe(const char* who, const crispy_pk* e, const crispy_pk_tdt* d, const long* sample_offset, int n_clips, Chain& ch) {
  if (!e || !d) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!e->weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no encoder is loaded (crispy_pk_load comes first)", who);
  if (!d->weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no decoder is loaded (crispy_pk_tdt_load comes first)", who);
  if (e->cfg.hidden != d->cfg.hidden)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: the encoder's hidden %d is not the decoder's (%d)", who, e->cfg.hidden, d->cfg.hidden);
  if (e->device != d->device) return fail(CRISPY_ERR_INVALID_ARG, "%s: the encoder is on device %d, the decoder on device %d", who, e->device, d->device);
  if (e->cfg.mel_bins > kMelMaxBins) return fail(CRISPY_ERR_INVALID_ARG, "%s: the front end has at most %d mel bins, the encoder %d", who, kMelMaxBins, e->cfg.mel_bins);
  if (!e->mel_fb.empty() && e->mel_fb_bins != e->cfg.mel_bins)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: the filters set with crispy_pk_set_mel_filters have %d bins, the encoder %d", who, e->mel_fb_bins, e->cfg.mel_bins);
  const int rc = mel_check_offsets(who, sample_offset, n_clips);
  if (rc != CRISPY_OK) return rc;
  ch.row_off.assign((size_t)n_clips + 1, 0);
  ch.frame_off.assign((size_t)n_clips + 1, 0);
  for (int c = 0; c < n_clips; ++c) {
    const long rows = mel_rows(sample_offset[c + 1] - sample_offset[c]), t = frames(rows);
    ch.row_off[(size_t)c + 1] = ch.row_off[(size_t)c] + rows;
    ch.frame_off[(size_t)c + 1] = ch.frame_off[(size_t)c] + t;
    ch.budget += tdt_max_steps(d->cfg.max_symbols_per_step, t);
  }
  return CRISPY_OK;
}

// The three stages; the arguments have been checked.  st == NULL: each handle's own stream, ordered by an event.
int transcribe_run(crispy_pk* e, crispy_pk_tdt* d, const char* who, const float* d_pcm, const long* sample_offset, int n_clips, const Chain& ch,
                   int* d_steps, int* d_n_steps, hipStream_t st) {
  const size_t M = (size_t)e->cfg.mel_bins, H = (size_t)e->cfg.hidden;
  auto round = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t rows_b = round((size_t)ch.row_off[(size_t)n_clips] * M * sizeof(float)), frames_b = round((size_t)ch.frame_off[(size_t)n_clips] * H * sizeof(float));
  if (rows_b + frames_b > e->chain.bytes) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (rows_b + frames_b > free_b + e->chain.bytes)
      return fail(CRISPY_ERR_OOM, "%s: the rows and frames need %zu bytes, the device has %zu free", who, rows_b + frames_b, free_b + e->chain.bytes);
    HIP_TRY(e->chain.grow(rows_b + frames_b));
  }
  float* d_rows = reinterpret_cast<float*>(e->chain.p);
  float* d_frames = reinterpret_cast<float*>(e->chain.p + rows_b);
  hipStream_t se = st ? st : e->stream, sd = st ? st : d->stream;
  int rc = mel_enqueue(e, who, (int)M, d_pcm, sample_offset, n_clips, d_rows, nullptr, nullptr, se);
  if (rc != CRISPY_OK) return rc;
  rc = pk_run(e, d_rows, ch.row_off.data(), n_clips, d_frames, nullptr, 0, nullptr, nullptr, se, false);
  if (rc != CRISPY_OK) return rc;
  if (se != sd) {
    HIP_TRY(e->chain_ev.ensure(1, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e->chain_ev[0], se));
    HIP_TRY(hipStreamWaitEvent(sd, e->chain_ev[0], 0));
  }
  return crispy_pk_tdt_decode_device(d, d_frames, ch.frame_off.data(), n_clips, d_steps, d_n_steps, nullptr, nullptr, sd);      // complete on return
}

}  // namespace

extern "C" {

int crispy_pk_create(int device, void** out) try {
  if (!out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_pk_create: out is NULL");
  *out = nullptr;
  const int rc = crispy::check_device(device, "crispy_pk_create");
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  crispy_pk* h = new crispy_pk;
  h->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    h->stream = nullptr;
    delete h;
    return fail(CRISPY_ERR_HIP, "crispy_pk_create: hipStreamCreate: %s", hipGetErrorString(e));
  }
  *out = h;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_create")

void crispy_pk_destroy(void* hv) try {
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}
CRISPY_CATCH_VOID("crispy_pk_destroy")

long crispy_pk_frames(long rows) try {
  return frames(rows);
}
CRISPY_CATCH_RET("crispy_pk_frames")

int crispy_pk_tensor_spec(const void* cfg, int i, const char** name, long* count) try {
  const char* who = "crispy_pk_tensor_spec";
  const int rc = check_config(who, as_cfg(cfg));
  if (rc != CRISPY_OK) return rc;
  static thread_local std::vector<Spec> sp;      // *name stays valid until this thread's next call
  sp = make_specs(*as_cfg(cfg));
  if (i < 0 || i >= (int)sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: i %d outside 0 ... %zu", who, i, sp.size() - 1);
  if (name) *name = sp[(size_t)i].name.c_str();
  if (count) *count = (long)sp[(size_t)i].count;
  return (int)sp.size();
}
CRISPY_CATCH_RET("crispy_pk_tensor_spec")

int crispy_pk_load(void* hv, const void* cfgv, const char* const* names, const float* const* data, const long* count, int n_tensors) try {
  const char* who = "crispy_pk_load";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_config(who, as_cfg(cfgv));
  if (rc != CRISPY_OK) return rc;
  const crispy_pk_config cfg = *as_cfg(cfgv);
  if (!names || !data || !count) return fail(CRISPY_ERR_INVALID_ARG, "%s: names, data or count is NULL", who);
  const std::vector<Spec> sp = make_specs(cfg);
  if (n_tensors < 1 || n_tensors > 4 * (int)sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_tensors %d outside 1 ... %zu", who, n_tensors, 4 * sp.size());
  std::map<std::string, size_t> index;
  for (size_t k = 0; k < sp.size(); ++k) index[sp[k].name] = k;
  std::vector<const float*> src(sp.size(), nullptr);
  for (int i = 0; i < n_tensors; ++i) {
    if (!names[i]) return fail(CRISPY_ERR_INVALID_ARG, "%s: names[%d] is NULL", who, i);
    const auto it = index.find(names[i]);
    if (it == index.end()) return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown tensor '%.200s'", who, names[i]);
    const size_t k = it->second;
    if (src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' given twice", who, names[i]);
    if (!data[i]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a NULL pointer", who, names[i]);
    if (count[i] != (long)sp[k].count) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has %ld values, expected %zu", who, names[i], count[i], sp[k].count);
    const bool is_var = sp[k].name.size() > 12 && sp[k].name.compare(sp[k].name.size() - 12, 12, ".running_var") == 0;
    for (size_t j = 0; j < sp[k].count; ++j) {
      if (!std::isfinite(data[i][j])) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a non-finite value at %zu", who, names[i], j);
      if (is_var && data[i][j] < 0.0f) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a negative variance at %zu", who, names[i], j);
    }
    src[k] = data[i];
  }
  for (size_t k = 0; k < sp.size(); ++k)
    if (!src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' is missing", who, sp[k].name.c_str());
  auto get = [&](const std::string& name) -> const float* {      // NULL for a bias the flags leave out
    const auto it = index.find(name);
    return it == index.end() ? nullptr : src[it->second];
  };
  const size_t H = (size_t)cfg.hidden, C = (size_t)cfg.sub_channels, F = (size_t)cfg.ffn, K = (size_t)cfg.conv_kernel;
  const size_t total = model_floats(cfg);
  std::vector<float> blob(total, 0.0f);      // a bias that is absent stays zero
  const PkModel m = model_of(blob.data(), cfg);
  auto copy = [&](const std::string& name, const float* dst, size_t n) {
    if (const float* s = get(name)) std::memcpy(wr(dst), s, n * sizeof(float));
  };
  auto linear = [&](const std::string& p, size_t out, size_t in, const float* w, const float* b, size_t ld, size_t col0) {
    put_transposed(get(p + ".weight"), out, in, 1, w, ld, col0);
    if (const float* s = get(p + ".bias")) std::memcpy(wr(b) + col0, s, out * sizeof(float));
  };
  put_transposed(get("subsampling.layers.0.weight"), C, 1, 9, m.conv0_w, C, 0);
  copy("subsampling.layers.0.bias", m.conv0_b, C);
  for (int i = 0; i < 2; ++i) {
    const std::string dw = "subsampling.layers." + std::to_string(2 + 3 * i), pw = "subsampling.layers." + std::to_string(3 + 3 * i);
    put_transposed(get(dw + ".weight"), C, 1, 9, m.dw_w[i], C, 0);
    copy(dw + ".bias", m.dw_b[i], C);
    linear(pw, C, C, m.pw_w[i], m.pw_b[i], C, 0);
  }
  linear("subsampling.linear", H, C * (size_t)(cfg.mel_bins / 8), m.lin_w, m.lin_b, H, 0);
  for (size_t k = 0; k < H / 2; ++k) wr(m.inv_freq)[k] = (float)(1.0 / std::pow(10000.0, (double)(2 * k) / (double)H));
  const char* const kNorm[5] = {"norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"};
  for (int li = 0; li < cfg.layers; ++li) {
    const PkLayer& l = m.layer[(size_t)li];
    const std::string p = "layers." + std::to_string(li) + ".";
    for (int i = 0; i < 5; ++i) {
      copy(p + kNorm[i] + ".weight", l.ln_g[i], H);
      copy(p + kNorm[i] + ".bias", l.ln_b[i], H);
    }
    for (int i = 0; i < 2; ++i) {
      const std::string q = p + (i ? "feed_forward2" : "feed_forward1");
      linear(q + ".linear1", F, H, l.ff_w1[i], l.ff_b1[i], F, 0);
      linear(q + ".linear2", H, F, l.ff_w2[i], l.ff_b2[i], H, 0);
    }
    linear(p + "self_attn.q_proj", H, H, l.qkv_w, l.qkv_b, 3 * H, 0);
    linear(p + "self_attn.k_proj", H, H, l.qkv_w, l.qkv_b, 3 * H, H);
    linear(p + "self_attn.v_proj", H, H, l.qkv_w, l.qkv_b, 3 * H, 2 * H);
    linear(p + "self_attn.o_proj", H, H, l.o_w, l.o_b, H, 0);
    linear(p + "self_attn.relative_k_proj", H, H, l.r_w, nullptr, H, 0);
    copy(p + "self_attn.bias_u", l.bias_u, H);
    copy(p + "self_attn.bias_v", l.bias_v, H);
    {
      const float* w1 = get(p + "conv.pointwise_conv1.weight");      // [2H][H][1]
      const float* b1 = get(p + "conv.pointwise_conv1.bias");
      for (size_t o = 0; o < 2 * H; ++o) {
        const size_t col = glu_column(o, H);
        for (size_t i = 0; i < H; ++i) wr(l.pw1_w)[i * 2 * H + col] = w1[o * H + i];
        if (b1) wr(l.pw1_b)[col] = b1[o];
      }
    }
    put_transposed(get(p + "conv.depthwise_conv.weight"), H, 1, K, l.dw_w, H, 0);
    {
      // BatchNorm at inference behind the depthwise bias: scale = w / sqrt(var + eps), shift = b + (bias - mean) * scale, in double
      const float *g = get(p + "conv.norm.weight"), *b = get(p + "conv.norm.bias"), *mean = get(p + "conv.norm.running_mean"),
                  *var = get(p + "conv.norm.running_var"), *db = get(p + "conv.depthwise_conv.bias");
      for (size_t c = 0; c < H; ++c) {
        const double s = (double)g[c] / std::sqrt((double)var[c] + kEps);
        wr(l.dw_scale)[c] = (float)s;
        wr(l.dw_shift)[c] = (float)((double)b[c] + ((db ? (double)db[c] : 0.0) - (double)mean[c]) * s);
      }
    }
    linear(p + "conv.pointwise_conv2", H, H, l.pw2_w, l.pw2_b, H, 0);
  }
  for (size_t i = 0; i < total; ++i)
    if (!std::isfinite(blob[i])) return fail(CRISPY_ERR_INVALID_ARG, "%s: a folded BatchNorm (weight / sqrt(running_var + 1e-5)) is not finite", who);
  HIP_TRY(hipSetDevice(h->device));
  crispy::DevBuf<float> fresh;
  HIP_TRY(fresh.alloc(total * sizeof(float)));
  HIP_TRY(hipMemcpy(fresh.p, blob.data(), total * sizeof(float), hipMemcpyHostToDevice));
  crispy::DevBuf<char> fresh16;      // the f16 copies of an earlier load go with it, in either mode
  if (h->precision == 1) {           // the mode survives the load: what does not fit refuses it, and the handle keeps what it had
    const int rc16 = pack_half(who, fresh.p, cfg, h->stream, fresh16);
    if (rc16 != CRISPY_OK) return rc16;
  }
  h->weights = std::move(fresh);      // the copy of an earlier load goes with `fresh`
  h->weights16 = std::move(fresh16);
  h->cfg = cfg;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_load")

int crispy_pk_loaded(void* hv) try {
  const crispy_pk* h = static_cast<const crispy_pk*>(hv);
  return h && h->weights.p ? 1 : 0;
}
CRISPY_CATCH_RET("crispy_pk_loaded")

int crispy_pk_config_of(void* hv, void* cfg) try {
  const char* who = "crispy_pk_config_of";
  const crispy_pk* h = static_cast<const crispy_pk*>(hv);
  if (!h || !cfg) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle or cfg", who);
  if (!h->weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no encoder is loaded (crispy_pk_load comes first)", who);
  *static_cast<crispy_pk_config*>(cfg) = h->cfg;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_config_of")

int crispy_pk_set_precision(void* hv, int mode) try {
  const char* who = "crispy_pk_set_precision";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (mode != 0 && mode != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: mode %d is neither 0 nor 1", who, mode);
  if (mode == 1 && h->weights.p && !h->weights16.p) {      // the first time a loaded handle is in mode 1
    HIP_TRY(hipSetDevice(h->device));
    const int rc = pack_half(who, h->weights.p, h->cfg, h->stream, h->weights16);
    if (rc != CRISPY_OK) return rc;      // the handle stays in the mode it had
  }
  h->precision = mode;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_set_precision")

int crispy_pk_precision(void* hv) try {
  const crispy_pk* h = static_cast<const crispy_pk*>(hv);
  return h ? h->precision : 0;
}
CRISPY_CATCH_RET("crispy_pk_precision")

int crispy_pk_stage_gemm_device(void* hv, int mode, int epilogue, const float* d_a, long M, int K, const float* d_w, const float* d_bias, int N,
                                float alpha, const float* d_res, float* d_c) try {
  const char* who = "crispy_pk_stage_gemm_device";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (mode != 0 && mode != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: mode %d is neither 0 nor 1", who, mode);
  if (epilogue < kGemmScale || epilogue > kGemmGlu) return fail(CRISPY_ERR_INVALID_ARG, "%s: epilogue %d outside 0 ... 3", who, epilogue);
  const GemmEpilogue e = static_cast<GemmEpilogue>(epilogue);
  if (!d_a || !d_w || !d_c) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_a, d_w or d_c is NULL", who);
  if (M < 1 || M > 0x7fffffffL) return fail(CRISPY_ERR_INVALID_ARG, "%s: M %ld outside 1 ... 2^31 - 1", who, M);
  if (K < 32 || K > 65536 || K % 32 != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: K %d is not a multiple of 32 in 32 ... 65536", who, K);
  if (N < 64 || N > 32768) return fail(CRISPY_ERR_INVALID_ARG, "%s: N %d outside 64 ... 32768", who, N);
  const int cols = e == kGemmGlu ? 2 * N : N;
  if (cols % 128 != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: N %d gives %d columns, not a multiple of 128", who, N, cols);
  if (e == kGemmResidual && !d_res) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_res is NULL with the residual epilogue", who);
  HIP_TRY(hipSetDevice(h->device));
  const size_t bt_b = (size_t)K * cols * sizeof(float), bp_b = mode == 1 ? (size_t)K * cols * 2 : 0;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bt_b + bp_b > free_b) return fail(CRISPY_ERR_OOM, "%s: the weight images need %zu bytes, the device has %zu free", who, bt_b + bp_b, free_b);
  crispy::DevBuf<float> bt;      // [K][cols], as crispy_pk_load lays a weight out
  crispy::DevBuf<char> bp;       // mode 1: its packed f16 image, as pack_half makes it
  crispy::DevBuf<float> bias;    // the GLU: the bias in the weight's column order, as crispy_pk_load puts it
  HIP_TRY(bt.alloc(bt_b));
  HIP_TRY(launch_weight_transpose(d_w, K, cols, e == kGemmGlu, bt.p, h->stream));
  if (e == kGemmGlu && d_bias) {
    HIP_TRY(bias.alloc((size_t)cols * sizeof(float)));
    HIP_TRY(launch_weight_transpose(d_bias, 1, cols, true, bias.p, h->stream));      // a [cols][1] matrix
    d_bias = bias.p;
  }
  if (mode == 1) {
    HIP_TRY(bp.alloc(bp_b));
    HIP_TRY(launch_pack_f16(bt.p, K, cols, bp.p, h->stream));
  }
  const hipError_t err = launch_gemm(mode, e, d_a, K, bt.p, bp.p, d_bias, N, alpha, d_res, d_c, M, h->stream);
  if (err == hipErrorInvalidValue) return fail(CRISPY_ERR_INVALID_ARG, "%s: launch_gemm refuses M %ld, K %d, N %d", who, M, K, N);
  HIP_TRY(err);
  HIP_TRY(hipStreamSynchronize(h->stream));      // bt and bp go with the call
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_stage_gemm_device")

int crispy_pk_set_attention_precision(void* hv, int mode) try {
  const char* who = "crispy_pk_set_attention_precision";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (mode != 0 && mode != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: mode %d is neither 0 nor 1", who, mode);
  h->attn_precision = mode;      // the operands are activations: nothing to pack
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_set_attention_precision")

int crispy_pk_attention_precision(void* hv) try {
  const crispy_pk* h = static_cast<const crispy_pk*>(hv);
  return h ? h->attn_precision : 0;
}
CRISPY_CATCH_RET("crispy_pk_attention_precision")

int crispy_pk_stage_attention_device(void* hv, int mode, const float* d_qkv, const float* d_r, const float* d_bias_u, const float* d_bias_v,
                                     const long* frame_offset, int n_clips, int heads, int tmax, float* d_out) try {
  const char* who = "crispy_pk_stage_attention_device";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (mode != 0 && mode != 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: mode %d is neither 0 nor 1", who, mode);
  const struct { const char* name; const void* p; } ptrs[] = {{"d_qkv", d_qkv}, {"d_r", d_r}, {"d_bias_u", d_bias_u}, {"d_bias_v", d_bias_v}, {"d_out", d_out}};
  for (const auto& a : ptrs) {
    if (!a.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: %s is NULL", who, a.name);
    if (reinterpret_cast<size_t>(a.p) % 16 != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: %s is not 16-byte aligned", who, a.name);
  }
  if (!frame_offset) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset is NULL", who);
  if (n_clips < 1 || n_clips > kMaxClips) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_clips %d outside 1 ... %d", who, n_clips, kMaxClips);
  if (heads < 1 || heads > 16) return fail(CRISPY_ERR_INVALID_ARG, "%s: heads %d outside 1 ... 16", who, heads);
  if (tmax < 1 || tmax > kMaxFrames) return fail(CRISPY_ERR_INVALID_ARG, "%s: tmax %d outside 1 ... %d", who, tmax, kMaxFrames);
  if (frame_offset[0] != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset[0] is %ld, not 0", who, frame_offset[0]);
  std::vector<int> off((size_t)n_clips + 1, 0);
  PkTables tb{};
  tb.n_clips = n_clips;
  for (int c = 0; c < n_clips; ++c) {
    const long n = frame_offset[c + 1] - frame_offset[c];
    if (n < 1 || n > tmax) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset: clip %d has %ld frames, outside 1 ... tmax (%d)", who, c, n, tmax);
    off[(size_t)c + 1] = (int)frame_offset[c + 1];
    tb.max_len[3] = std::max(tb.max_len[3], (int)n);
  }
  HIP_TRY(hipSetDevice(h->device));
  crispy::DevBuf<int> d_off;
  HIP_TRY(d_off.alloc(off.size() * sizeof(int)));
  HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  tb.off[3] = d_off.p;
  PkLayer l{};
  l.bias_u = d_bias_u;
  l.bias_v = d_bias_v;
  const hipError_t err = launch_attention(mode, l, tb, d_qkv, d_r, tmax, heads, d_out, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));      // off and d_off go with the call
  HIP_TRY(err);
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_stage_attention_device")

int crispy_pk_encode_device(void* hv, const float* d_feats, const long* frame_offset, int n_clips, float* d_out, float* d_sub, int tap_layer,
                            float* d_tap, float* d_pos, void* hip_stream) try {
  const char* who = "crispy_pk_encode_device";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  const int rc = check_call(who, h, frame_offset, n_clips, tap_layer, d_tap);
  if (rc != CRISPY_OK) return rc;
  if (!d_feats || !d_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_feats or d_out is NULL", who);
  HIP_TRY(hipSetDevice(h->device));
  return pk_run(h, d_feats, frame_offset, n_clips, d_out, d_sub, tap_layer, d_tap, d_pos, hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_pk_encode_device")

int crispy_pk_encode(void* hv, const float* feats, const long* frame_offset, int n_clips, float* out, float* sub, int tap_layer, float* tap,
                     float* pos) try {
  const char* who = "crispy_pk_encode";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  const int rc0 = check_call(who, h, frame_offset, n_clips, tap_layer, tap);
  if (rc0 != CRISPY_OK) return rc0;
  if (!feats || !out) return fail(CRISPY_ERR_INVALID_ARG, "%s: feats or out is NULL", who);
  const size_t H = (size_t)h->cfg.hidden, M = (size_t)h->cfg.mel_bins;
  size_t T = 0, tmax = 0;
  for (int c = 0; c < n_clips; ++c) {
    const size_t t = (size_t)frames(frame_offset[c + 1] - frame_offset[c]);
    T += t;
    tmax = std::max(tmax, t);
  }
  auto round = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t feat_b = round((size_t)frame_offset[n_clips] * M * sizeof(float)), out_b = round(T * H * sizeof(float)),
               pos_b = round((2 * tmax - 1) * H * sizeof(float));
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(h->io.grow(feat_b + out_b * (1 + (sub ? 1 : 0) + (tap ? 1 : 0)) + (pos ? pos_b : 0)));
  char* at = h->io.p;
  float* d_feats = reinterpret_cast<float*>(at); at += feat_b;
  float* d_out = reinterpret_cast<float*>(at); at += out_b;
  float* d_sub = nullptr; if (sub) { d_sub = reinterpret_cast<float*>(at); at += out_b; }
  float* d_tap = nullptr; if (tap) { d_tap = reinterpret_cast<float*>(at); at += out_b; }
  float* d_pos = pos ? reinterpret_cast<float*>(at) : nullptr;
  HIP_TRY(hipMemcpyAsync(d_feats, feats, (size_t)frame_offset[n_clips] * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const int rc = pk_run(h, d_feats, frame_offset, n_clips, d_out, d_sub, tap_layer, d_tap, d_pos, h->stream);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out, d_out, T * H * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (sub) HIP_TRY(hipMemcpyAsync(sub, d_sub, T * H * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (tap) HIP_TRY(hipMemcpyAsync(tap, d_tap, T * H * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (pos) HIP_TRY(hipMemcpyAsync(pos, d_pos, (2 * tmax - 1) * H * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_encode")

int crispy_pk_transcribe_device(void* h_enc, void* h_tdt, const float* d_pcm, const long* sample_offset, int n_clips, int* d_steps, int* d_n_steps,
                                void* hip_stream) try {
  const char* who = "crispy_pk_transcribe_device";
  crispy_pk* e = static_cast<crispy_pk*>(h_enc);
  crispy_pk_tdt* d = static_cast<crispy_pk_tdt*>(h_tdt);
  Chain ch;
  const int rc = check_transcribe(who, e, d, sample_offset, n_clips, ch);
  if (rc != CRISPY_OK) return rc;
  if (!d_pcm || !d_n_steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_pcm or d_n_steps is NULL", who);
  if (ch.budget > 0 && !d_steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_steps is NULL", who);
  HIP_TRY(hipSetDevice(e->device));
  return transcribe_run(e, d, who, d_pcm, sample_offset, n_clips, ch, d_steps, d_n_steps, static_cast<hipStream_t>(hip_stream));
}
CRISPY_CATCH_RET("crispy_pk_transcribe_device")

int crispy_pk_transcribe(void* h_enc, void* h_tdt, const float* pcm, const long* sample_offset, int n_clips, int* steps, int* n_steps) try {
  const char* who = "crispy_pk_transcribe";
  crispy_pk* e = static_cast<crispy_pk*>(h_enc);
  crispy_pk_tdt* d = static_cast<crispy_pk_tdt*>(h_tdt);
  Chain ch;
  const int rc0 = check_transcribe(who, e, d, sample_offset, n_clips, ch);
  if (rc0 != CRISPY_OK) return rc0;
  if (!pcm || !n_steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: pcm or n_steps is NULL", who);
  const size_t B = (size_t)ch.budget, n = (size_t)sample_offset[n_clips];
  if (B > 0 && !steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: steps is NULL", who);
  auto round = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t pcm_b = round(n * sizeof(float)), steps_b = round(B * 3 * sizeof(int)), n_b = round((size_t)n_clips * sizeof(int));
  const size_t need = pcm_b + steps_b + n_b;
  HIP_TRY(hipSetDevice(e->device));
  if (need > e->io.bytes) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b + e->io.bytes) return fail(CRISPY_ERR_OOM, "%s: the call's buffers need %zu bytes, the device has %zu free", who, need, free_b + e->io.bytes);
    HIP_TRY(e->io.grow(need));
  }
  float* d_pcm = reinterpret_cast<float*>(e->io.p);
  int* d_steps = reinterpret_cast<int*>(e->io.p + pcm_b);
  int* d_n = reinterpret_cast<int*>(e->io.p + pcm_b + steps_b);
  HIP_TRY(hipMemcpyAsync(d_pcm, pcm, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
  if (B > 0) HIP_TRY(hipMemsetAsync(d_steps, 0, B * 3 * sizeof(int), e->stream));      // rows behind a clip's n_steps read as zeros
  const int rc = transcribe_run(e, d, who, d_pcm, sample_offset, n_clips, ch, d_steps, d_n, nullptr);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(n_steps, d_n, (size_t)n_clips * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (B > 0) HIP_TRY(hipMemcpyAsync(steps, d_steps, B * 3 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_transcribe")

}  // extern "C"

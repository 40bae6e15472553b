// diar_seg_api.cpp -- host side of the segmentation network (include/crispy_hip.h, "Segmentation network"; kernels in
// diar_seg.hip): the tensor table and the checks of crispy_diar_seg_load, the layout of the handle's device copy, and the
// turns and launches of the forward and the recording entry points (pyannote_get_segments_fixed,
// src-tauri/src/managers/diarization.rs:103-145).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_util.h"
#include "diar_internal.h"

using crispy::fail;
using namespace crispy::diar;

namespace {

constexpr long kMaxSamples = 115200000;                 // 2 h at 16 kHz, as the ASR path
constexpr int kMaxWindows = 4096;
constexpr int kHead = kSegHidden;                       // width of the two hidden linear layers

int lstm_in(int layer) { return layer == 0 ? kSegC1 : 2 * kSegHidden; }

// ---- the tensors crispy_diar_seg_load takes -------------------------------------------------------------------------
struct Spec {
  std::string name;
  size_t count;
};

std::vector<Spec> specs() {
  std::vector<Spec> s = {
      {"sincnet.wav_norm1d.weight", 1},
      {"sincnet.wav_norm1d.bias", 1},
      {"sincnet.conv1d.0.filters", (size_t)kSegC0 * kSegTaps0},
      {"sincnet.conv1d.1.weight", (size_t)kSegC1 * kSegC0 * kSegTaps},
      {"sincnet.conv1d.1.bias", (size_t)kSegC1},
      {"sincnet.conv1d.2.weight", (size_t)kSegC1 * kSegC1 * kSegTaps},
      {"sincnet.conv1d.2.bias", (size_t)kSegC1},
  };
  const int norm_c[3] = {kSegC0, kSegC1, kSegC1};
  for (int i = 0; i < 3; ++i) {
    s.push_back({"sincnet.norm1d." + std::to_string(i) + ".weight", (size_t)norm_c[i]});
    s.push_back({"sincnet.norm1d." + std::to_string(i) + ".bias", (size_t)norm_c[i]});
  }
  for (int l = 0; l < kSegLayers; ++l)
    for (int d = 0; d < 2; ++d) {
      const std::string tail = "_l" + std::to_string(l) + (d ? "_reverse" : "");
      s.push_back({"lstm.weight_ih" + tail, (size_t)kSegGates * lstm_in(l)});
      s.push_back({"lstm.weight_hh" + tail, (size_t)kSegGates * kSegHidden});
      s.push_back({"lstm.bias_ih" + tail, (size_t)kSegGates});
      s.push_back({"lstm.bias_hh" + tail, (size_t)kSegGates});
    }
  s.push_back({"linear.0.weight", (size_t)kHead * 2 * kSegHidden});
  s.push_back({"linear.0.bias", (size_t)kHead});
  s.push_back({"linear.1.weight", (size_t)kHead * kHead});
  s.push_back({"linear.1.bias", (size_t)kHead});
  s.push_back({"classifier.weight", (size_t)kSegClasses * kHead});
  s.push_back({"classifier.bias", (size_t)kSegClasses});
  return s;
}

// ---- the device copy ------------------------------------------------------------------------------------------------
struct Layout {
  size_t wav_g, wav_b, f0, w1, b1, w2, b2, n_g[3], n_b[3], w_ih[kSegLayers], b[kSegLayers], w_hh[kSegLayers], l0, l0_b, l1, l1_b, cls, cls_b;
  size_t total;
};

Layout layout() {
  Layout y{};
  size_t at = 0;
  auto take = [&at](size_t n) {
    const size_t r = at;
    at += (n + 63) & ~(size_t)63;      // every tensor starts on a 256-byte boundary
    return r;
  };
  y.wav_g = take(1);
  y.wav_b = take(1);
  y.f0 = take((size_t)kSegTaps0 * kSegC0);
  y.w1 = take((size_t)kSegC0 * kSegTaps * kSegC1);
  y.b1 = take(kSegC1);
  y.w2 = take((size_t)kSegC1 * kSegTaps * kSegC1);
  y.b2 = take(kSegC1);
  const int norm_c[3] = {kSegC0, kSegC1, kSegC1};
  for (int i = 0; i < 3; ++i) {
    y.n_g[i] = take(norm_c[i]);
    y.n_b[i] = take(norm_c[i]);
  }
  for (int l = 0; l < kSegLayers; ++l) {
    y.w_ih[l] = take((size_t)2 * kSegGates * lstm_in(l));
    y.b[l] = take((size_t)2 * kSegGates);
    y.w_hh[l] = take((size_t)2 * kSegGates * kSegHidden);
  }
  y.l0 = take((size_t)2 * kSegHidden * kHead);
  y.l0_b = take(kHead);
  y.l1 = take((size_t)kHead * kHead);
  y.l1_b = take(kHead);
  y.cls = take((size_t)kSegClasses * kHead);
  y.cls_b = take(kSegClasses);
  y.total = at;
  return y;
}

SegModel model_of(const float* p) {
  const Layout y = layout();
  SegModel m{};
  m.wav_g = p + y.wav_g; m.wav_b = p + y.wav_b;
  m.f0 = p + y.f0; m.w1 = p + y.w1; m.b1 = p + y.b1; m.w2 = p + y.w2; m.b2 = p + y.b2;
  for (int i = 0; i < 3; ++i) { m.n_g[i] = p + y.n_g[i]; m.n_b[i] = p + y.n_b[i]; }
  for (int l = 0; l < kSegLayers; ++l) { m.w_ih[l] = p + y.w_ih[l]; m.b[l] = p + y.b[l]; m.w_hh[l] = p + y.w_hh[l]; }
  m.l0 = p + y.l0; m.l0_b = p + y.l0_b; m.l1 = p + y.l1; m.l1_b = p + y.l1_b; m.cls = p + y.cls; m.cls_b = p + y.cls_b;
  return m;
}

// torch's [co][ci][k] -> [(ci * taps + k)][co]
void conv_transposed(const float* src, int co_n, int ci_n, int taps, float* dst) {
  for (int co = 0; co < co_n; ++co)
    for (int ci = 0; ci < ci_n; ++ci)
      for (int k = 0; k < taps; ++k) dst[((size_t)ci * taps + k) * co_n + co] = src[((size_t)co * ci_n + ci) * taps + k];
}

// torch's [out][in] -> [in][out]
void linear_transposed(const float* src, int out_n, int in_n, float* dst) {
  for (int o = 0; o < out_n; ++o)
    for (int i = 0; i < in_n; ++i) dst[(size_t)i * out_n + o] = src[(size_t)o * in_n + i];
}

// ---- a call's scratch -----------------------------------------------------------------------------------------------
struct Turn {
  float *x, *pool0, *pool1, *pool2, *sinc, *xproj, *ya, *yb;
  float2 *st_w, *st0, *st1, *st2;
};

void carve_turn(Carve& c, Turn& t, const SegShape& s, size_t nw, bool from_pcm) {
  t.x = from_pcm ? c.take<float>(nw * kSegWindow) : nullptr;
  t.st_w = c.take<float2>(nw);
  t.pool0 = c.take<float>(nw * s.p0 * kSegC0);
  t.st0 = c.take<float2>(nw * kSegC0);
  t.pool1 = c.take<float>(nw * s.p1 * kSegC1);
  t.st1 = c.take<float2>(nw * kSegC1);
  t.pool2 = c.take<float>(nw * s.frames * kSegC1);
  t.st2 = c.take<float2>(nw * kSegC1);
  t.sinc = c.take<float>(nw * s.frames * kSegC1);
  t.xproj = c.take<float>(nw * s.frames * 2 * kSegGates);
  t.ya = c.take<float>(nw * s.frames * 2 * kSegHidden);
  t.yb = c.take<float>(nw * s.frames * 2 * kSegHidden);
}

// Developer aid (CRISPY_DIAR_SEG_TIMELINE in the dev build): device time of a call by kernel family, to stderr.
struct Timeline {
  bool on = false;
  crispy::EventList ev;
  std::vector<int> family;      // family[i]: what ran between event i and event i + 1
  hipError_t mark(int fam, hipStream_t st) {      // fam < 0: the start of a turn
    if (!on) return hipSuccess;
    hipError_t e = ev.ensure(ev.v.size() + 1, 0);
    if (e != hipSuccess) return e;
    family.push_back(fam);
    return hipEventRecord(ev.v.back(), st);
  }
  void report() const {
    if (!on) return;
    double ms[4] = {0, 0, 0, 0};
    for (size_t i = 1; i < ev.v.size(); ++i) {
      float t = 0.0f;
      if (family[i] >= 0 && hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[family[i]] += t;
    }
    std::fprintf(stderr, "crispy_diar_seg timeline: front %.3f ms, projections %.3f ms, recurrence %.3f ms, head %.3f ms\n", ms[0], ms[1],
                 ms[2], ms[3]);
  }
};

// The network on n_win windows of `len` samples: d_x [n_win][len], or (d_x NULL) the windows of the recording d_pcm.
int seg_run(crispy_diar* h, const float* d_x, const void* d_pcm, int pcm_format, long n_samples, int n_win, long len, float* d_scores,
            float* d_sinc, float* d_lstm, hipStream_t st) {
  const SegShape s = seg_shape(len);
  const SegModel m = model_of(h->seg_weights.p);
  const bool from_pcm = d_x == nullptr;
  Carve one;
  Turn t{};
  carve_turn(one, t, s, 1, from_pcm);
  size_t turn = std::max<size_t>(1, std::min<size_t>((size_t)n_win, kScratchCap / one.used));
  if (const char* e = crispy::dev_env("CRISPY_DIAR_SEG_TURN")) {      // developer knob: small turns, for the test of their bytes
    const int v = std::atoi(e);
    if (v > 0) turn = std::min<size_t>(turn, (size_t)v);
  }
  Carve size;
  carve_turn(size, t, s, turn, from_pcm);
  HIP_TRY(h->scratch.grow(size.used));
  Timeline tl;
  tl.on = crispy::dev_env("CRISPY_DIAR_SEG_TIMELINE") != nullptr;
  const size_t fr = (size_t)s.frames;
  for (size_t w0 = 0; w0 < (size_t)n_win; w0 += turn) {
    const int nw = (int)std::min(turn, (size_t)n_win - w0);
    Carve c;
    c.p = h->scratch.p;
    carve_turn(c, t, s, (size_t)nw, from_pcm);
    const long rows = (long)nw * s.frames;
    HIP_TRY(tl.mark(-1, st));
    const float* x = d_x ? d_x + w0 * (size_t)len : t.x;
    if (from_pcm) HIP_TRY(launch_seg_windows(d_pcm, pcm_format, n_samples, (long)w0, nw, t.x, st));
    HIP_TRY(launch_seg_stats(x, nw, (int)len, 1, t.st_w, st));
    HIP_TRY(launch_seg_conv(0, m, x, nw, (int)len, t.st_w, t.pool0, s.p0, st));
    HIP_TRY(launch_seg_stats(t.pool0, nw, s.p0, kSegC0, t.st0, st));
    HIP_TRY(launch_seg_conv(1, m, t.pool0, nw, s.p0, t.st0, t.pool1, s.p1, st));
    HIP_TRY(launch_seg_stats(t.pool1, nw, s.p1, kSegC1, t.st1, st));
    HIP_TRY(launch_seg_conv(2, m, t.pool1, nw, s.p1, t.st1, t.pool2, s.frames, st));
    HIP_TRY(launch_seg_stats(t.pool2, nw, s.frames, kSegC1, t.st2, st));
    float* sinc = d_sinc ? d_sinc + w0 * fr * kSegC1 : t.sinc;
    HIP_TRY(launch_seg_norm(m, t.pool2, nw, s.frames, t.st2, sinc, st));
    HIP_TRY(tl.mark(0, st));
    const float* in = sinc;
    for (int l = 0; l < kSegLayers; ++l) {
      float* out = (l == kSegLayers - 1 && d_lstm) ? d_lstm + w0 * fr * 2 * kSegHidden : (l % 2 ? t.yb : t.ya);
      HIP_TRY(launch_seg_proj(in, rows, lstm_in(l), m.w_ih[l], m.b[l], t.xproj, st));
      HIP_TRY(tl.mark(1, st));
      HIP_TRY(launch_seg_lstm(t.xproj, m.w_hh[l], nw, s.frames, out, st));
      HIP_TRY(tl.mark(2, st));
      in = out;
    }
    HIP_TRY(launch_seg_head(m, in, rows, d_scores + w0 * fr * kSegClasses, st));
    HIP_TRY(tl.mark(3, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  tl.report();
  return CRISPY_OK;
}

long windows_of(long n) { return n <= 0 ? 0 : (n + kSegWindow - 1) / kSegWindow + 1; }

// What the two recording entry points check before a device is touched.
int check_scores_args(const char* who, crispy_diar* h, const void* pcm, int pcm_format, long n_samples, const float* scores) {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (pcm_format != CRISPY_PCM_I16 && pcm_format != CRISPY_PCM_F32)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: pcm_format %d is neither CRISPY_PCM_I16 nor CRISPY_PCM_F32", who, pcm_format);
  if (n_samples < 1 || n_samples > kMaxSamples)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: n_samples %ld outside 1 ... %ld", who, n_samples, kMaxSamples);
  if (!pcm || !scores) return fail(CRISPY_ERR_INVALID_ARG, "%s: pcm or scores is NULL", who);
  return CRISPY_OK;
}

int check_loaded(const char* who, const crispy_diar* h) {
  if (!h->seg_weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no segmentation network is loaded (crispy_diar_seg_load comes first)", who);
  return CRISPY_OK;
}

}  // namespace

extern "C" {

long crispy_diar_seg_frames(long len) try {
  if (len < kSegMinLen) return 0;
  return ((((len - kSegTaps0) / kSegStride0 + 1) / 3 - (kSegTaps - 1)) / 3 - (kSegTaps - 1)) / 3;
}
CRISPY_CATCH_RET("crispy_diar_seg_frames")

long crispy_diar_seg_windows(long n_samples) try {
  return windows_of(n_samples);
}
CRISPY_CATCH_RET("crispy_diar_seg_windows")

int crispy_diar_seg_load(void* hv, const char* const* names, const float* const* data, const long* count, int n_tensors) try {
  const char* who = "crispy_diar_seg_load";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!names || !data || !count) return fail(CRISPY_ERR_INVALID_ARG, "%s: names, data or count is NULL", who);
  const std::vector<Spec> sp = specs();
  if (n_tensors < 1 || n_tensors > 4 * (int)sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_tensors %d outside 1 ... %zu", who, n_tensors, 4 * sp.size());
  std::vector<const float*> src(sp.size(), nullptr);
  for (int i = 0; i < n_tensors; ++i) {
    if (!names[i]) return fail(CRISPY_ERR_INVALID_ARG, "%s: names[%d] is NULL", who, i);
    size_t k = 0;
    while (k < sp.size() && sp[k].name != names[i]) ++k;
    if (k == sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown tensor '%.200s'", who, names[i]);
    if (src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' given twice", who, names[i]);
    if (!data[i]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a NULL pointer", who, names[i]);
    if (count[i] != (long)sp[k].count)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has %ld values, expected %zu", who, names[i], count[i], sp[k].count);
    for (size_t j = 0; j < sp[k].count; ++j)
      if (!std::isfinite(data[i][j])) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a non-finite value at %zu", who, names[i], j);
    src[k] = data[i];
  }
  for (size_t k = 0; k < sp.size(); ++k)
    if (!src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' is missing", who, sp[k].name.c_str());
  auto get = [&](const std::string& name) {
    size_t k = 0;
    while (sp[k].name != name) ++k;      // every name below is in the table
    return src[k];
  };
  const Layout y = layout();
  std::vector<float> blob(y.total, 0.0f);
  float* b = blob.data();
  b[y.wav_g] = get("sincnet.wav_norm1d.weight")[0];
  b[y.wav_b] = get("sincnet.wav_norm1d.bias")[0];
  conv_transposed(get("sincnet.conv1d.0.filters"), kSegC0, 1, kSegTaps0, b + y.f0);
  conv_transposed(get("sincnet.conv1d.1.weight"), kSegC1, kSegC0, kSegTaps, b + y.w1);
  conv_transposed(get("sincnet.conv1d.2.weight"), kSegC1, kSegC1, kSegTaps, b + y.w2);
  std::memcpy(b + y.b1, get("sincnet.conv1d.1.bias"), kSegC1 * sizeof(float));
  std::memcpy(b + y.b2, get("sincnet.conv1d.2.bias"), kSegC1 * sizeof(float));
  const int norm_c[3] = {kSegC0, kSegC1, kSegC1};
  for (int i = 0; i < 3; ++i) {
    std::memcpy(b + y.n_g[i], get("sincnet.norm1d." + std::to_string(i) + ".weight"), norm_c[i] * sizeof(float));
    std::memcpy(b + y.n_b[i], get("sincnet.norm1d." + std::to_string(i) + ".bias"), norm_c[i] * sizeof(float));
  }
  for (int l = 0; l < kSegLayers; ++l)
    for (int d = 0; d < 2; ++d) {
      const std::string tail = "_l" + std::to_string(l) + (d ? "_reverse" : "");
      const size_t in = (size_t)lstm_in(l);
      std::memcpy(b + y.w_ih[l] + d * kSegGates * in, get("lstm.weight_ih" + tail), kSegGates * in * sizeof(float));
      std::memcpy(b + y.w_hh[l] + (size_t)d * kSegGates * kSegHidden, get("lstm.weight_hh" + tail), (size_t)kSegGates * kSegHidden * sizeof(float));
      const float *bi = get("lstm.bias_ih" + tail), *bh = get("lstm.bias_hh" + tail);
      for (int g = 0; g < kSegGates; ++g) b[y.b[l] + d * kSegGates + g] = bi[g] + bh[g];
    }
  linear_transposed(get("linear.0.weight"), kHead, 2 * kSegHidden, b + y.l0);
  linear_transposed(get("linear.1.weight"), kHead, kHead, b + y.l1);
  std::memcpy(b + y.l0_b, get("linear.0.bias"), kHead * sizeof(float));
  std::memcpy(b + y.l1_b, get("linear.1.bias"), kHead * sizeof(float));
  std::memcpy(b + y.cls, get("classifier.weight"), (size_t)kSegClasses * kHead * sizeof(float));
  std::memcpy(b + y.cls_b, get("classifier.bias"), kSegClasses * sizeof(float));
  for (size_t i = 0; i < y.total; ++i)
    if (!std::isfinite(b[i])) return fail(CRISPY_ERR_INVALID_ARG, "%s: bias_ih + bias_hh of an lstm layer is not finite", who);
  HIP_TRY(hipSetDevice(h->device));
  crispy::DevBuf<float> fresh;
  HIP_TRY(fresh.alloc(y.total * sizeof(float)));
  HIP_TRY(hipMemcpy(fresh.p, b, y.total * sizeof(float), hipMemcpyHostToDevice));
  h->seg_weights = std::move(fresh);      // the copy of an earlier load goes with `fresh`
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_seg_load")

int crispy_diar_seg_loaded(void* hv) try {
  const crispy_diar* h = static_cast<const crispy_diar*>(hv);
  return h && h->seg_weights.p ? 1 : 0;
}
CRISPY_CATCH_RET("crispy_diar_seg_loaded")

int crispy_diar_seg_forward_device(void* hv, const float* d_x, int n_win, long len, float* d_scores, float* d_sincnet, float* d_lstm,
                                   void* hip_stream) try {
  const char* who = "crispy_diar_seg_forward_device";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (len < kSegMinLen || len > kSegWindow) return fail(CRISPY_ERR_INVALID_ARG, "%s: len %ld outside %d ... %d", who, len, kSegMinLen, kSegWindow);
  if (n_win < 1 || n_win > kMaxWindows) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_win %d outside 1 ... %d", who, n_win, kMaxWindows);
  if (!d_x || !d_scores) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_x or d_scores is NULL", who);
  const int rc = check_loaded(who, h);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return seg_run(h, d_x, nullptr, CRISPY_PCM_F32, 0, n_win, len, d_scores, d_sincnet, d_lstm,
                 hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_diar_seg_forward_device")

int crispy_diar_seg_scores_device(void* hv, const void* d_pcm, int pcm_format, long n_samples, float* d_scores, void* hip_stream) try {
  const char* who = "crispy_diar_seg_scores_device";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  int rc = check_scores_args(who, h, d_pcm, pcm_format, n_samples, d_scores);
  if (rc != CRISPY_OK) return rc;
  rc = check_loaded(who, h);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return seg_run(h, nullptr, d_pcm, pcm_format, n_samples, (int)windows_of(n_samples), kSegWindow, d_scores, nullptr, nullptr,
                 hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_diar_seg_scores_device")

int crispy_diar_seg_scores(void* hv, const void* pcm, int pcm_format, long n_samples, float* scores) try {
  const char* who = "crispy_diar_seg_scores";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  int rc = check_scores_args(who, h, pcm, pcm_format, n_samples, scores);
  if (rc != CRISPY_OK) return rc;
  rc = check_loaded(who, h);
  if (rc != CRISPY_OK) return rc;
  const size_t elem = pcm_format == CRISPY_PCM_F32 ? sizeof(float) : sizeof(short);
  const size_t pcm_bytes = ((size_t)n_samples * elem + 255) & ~(size_t)255;
  const size_t score_bytes = (size_t)windows_of(n_samples) * seg_shape(kSegWindow).frames * kSegClasses * sizeof(float);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(h->io.grow(pcm_bytes + score_bytes));
  float* d_scores = reinterpret_cast<float*>(h->io.p + pcm_bytes);
  HIP_TRY(hipMemcpyAsync(h->io.p, pcm, (size_t)n_samples * elem, hipMemcpyHostToDevice, h->stream));
  rc = seg_run(h, nullptr, h->io.p, pcm_format, n_samples, (int)windows_of(n_samples), kSegWindow, d_scores, nullptr, nullptr, h->stream);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(scores, d_scores, score_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_seg_scores")

}  // extern "C"

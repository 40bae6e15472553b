// diar_emb_api.cpp -- host side of the speaker-embedding network (include/crispy_hip.h, "Embedding network"; kernels in
// diar_emb.hip): the tensor table of crispy_diar_emb_tensor_spec and crispy_diar_emb_load, the BatchNorm folds and the layout
// of the handle's device copy, the turns and launches of the forward, and the recording entry points
// (EmbeddingExtractor::compute, src-tauri/src/managers/diarization.rs:53-75, for all chunks of a recording).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "api_util.h"
#include "diar_internal.h"

using crispy::fail;
using namespace crispy::diar;

namespace {

constexpr int kMaxChunks = 16384;      // as crispy_diar_fbank

// ---- the tensors crispy_diar_emb_load takes, in the order of wespeaker's state dict ----------------------------------
struct Spec {
  std::string name;
  size_t count;      // fixed part
  size_t per_dim;    // + per_dim * dim
};

const char* const kHeadConv[kEmbHeadConvs] = {"head.conv1",           "head.layer1.0.conv1", "head.layer1.0.conv2", "head.layer1.0.shortcut.0",
                                              "head.layer1.1.conv1",  "head.layer1.1.conv2", "head.layer2.0.conv1", "head.layer2.0.conv2",
                                              "head.layer2.0.shortcut.0", "head.layer2.1.conv1", "head.layer2.1.conv2", "head.conv2"};
const char* const kHeadBn[kEmbHeadConvs] = {"head.bn1",           "head.layer1.0.bn1", "head.layer1.0.bn2", "head.layer1.0.shortcut.1",
                                            "head.layer1.1.bn1",  "head.layer1.1.bn2", "head.layer2.0.bn1", "head.layer2.0.bn2",
                                            "head.layer2.0.shortcut.1", "head.layer2.1.bn1", "head.layer2.1.bn2", "head.bn2"};
int head_cin(int i) { return i == 0 ? 1 : kEmbHeadCh; }
int head_ks(int i) { return (i == 3 || i == 8) ? 1 : 3; }

std::string layer_name(int b, int i) { return "xvector.block" + std::to_string(b + 1) + ".tdnnd" + std::to_string(i + 1); }
std::string transit_name(int b) { return "xvector.transit" + std::to_string(b + 1); }
int block_cin(int b) { return b == 0 ? kEmbInit : kEmbBlockWidth[b - 1] / 2; }

void push_bn(std::vector<Spec>& s, const std::string& p, size_t c, bool affine = true) {
  if (affine) {
    s.push_back({p + ".weight", c, 0});
    s.push_back({p + ".bias", c, 0});
  }
  s.push_back({p + ".running_mean", c, 0});
  s.push_back({p + ".running_var", c, 0});
}

std::vector<Spec> make_specs() {
  std::vector<Spec> s;
  // state-dict order inside the head: conv1, bn1, the layers, conv2, bn2; inside a block: conv1, bn1, conv2, bn2, shortcut
  for (int i = 0; i < kEmbHeadConvs; ++i) {
    s.push_back({std::string(kHeadConv[i]) + ".weight", (size_t)kEmbHeadCh * head_cin(i) * head_ks(i) * head_ks(i), 0});
    push_bn(s, kHeadBn[i], kEmbHeadCh);
  }
  s.push_back({"xvector.tdnn.linear.weight", (size_t)kEmbInit * kEmbHeadOut * kEmbTdnnTaps, 0});
  push_bn(s, "xvector.tdnn.nonlinear.batchnorm", kEmbInit);
  for (int b = 0; b < kEmbBlocks; ++b) {
    for (int i = 0; i < kEmbBlockLayers[b]; ++i) {
      const std::string p = layer_name(b, i);
      const size_t cin = (size_t)block_cin(b) + (size_t)i * kEmbGrowth;
      push_bn(s, p + ".nonlinear1.batchnorm", cin);
      s.push_back({p + ".linear1.weight", (size_t)kEmbBn * cin, 0});
      push_bn(s, p + ".nonlinear2.batchnorm", kEmbBn);
      s.push_back({p + ".cam_layer.linear_local.weight", (size_t)kEmbGrowth * kEmbBn * 3, 0});
      s.push_back({p + ".cam_layer.linear1.weight", (size_t)kEmbGate * kEmbBn, 0});
      s.push_back({p + ".cam_layer.linear1.bias", (size_t)kEmbGate, 0});
      s.push_back({p + ".cam_layer.linear2.weight", (size_t)kEmbGrowth * kEmbGate, 0});
      s.push_back({p + ".cam_layer.linear2.bias", (size_t)kEmbGrowth, 0});
    }
    const size_t c = (size_t)kEmbBlockWidth[b];
    push_bn(s, transit_name(b) + ".nonlinear.batchnorm", c);
    s.push_back({transit_name(b) + ".linear.weight", c * (c / 2), 0});
  }
  push_bn(s, "xvector.out_nonlinear.batchnorm", kEmbXvec);
  s.push_back({"xvector.dense.linear.weight", 0, (size_t)kEmbStats});
  s.push_back({"xvector.dense.nonlinear.batchnorm.running_mean", 0, 1});
  s.push_back({"xvector.dense.nonlinear.batchnorm.running_var", 0, 1});
  return s;
}

const std::vector<Spec>& specs() {
  static const std::vector<Spec> s = make_specs();
  return s;
}

// ---- the device copy ------------------------------------------------------------------------------------------------
// Visits every field of the model in a fixed order with its element count: once to add up the size, once to place the fields.
template <class V>
void walk(EmbModel& m, int dim, V&& v) {
  m.dim = dim;
  for (int i = 0; i < kEmbHeadConvs; ++i) {
    v(m.head[i].w, (size_t)head_ks(i) * head_ks(i) * head_cin(i) * kEmbHeadCh);
    v(m.head[i].scale, kEmbHeadCh);
    v(m.head[i].shift, kEmbHeadCh);
  }
  v(m.tdnn.w, (size_t)kEmbTdnnTaps * kEmbHeadOut * kEmbInit);
  v(m.tdnn.scale, kEmbInit);
  v(m.tdnn.shift, kEmbInit);
  int l = 0;
  for (int b = 0; b < kEmbBlocks; ++b) {
    for (int i = 0; i < kEmbBlockLayers[b]; ++i, ++l) {
      EmbDense& d = m.layer[l];
      d.c_in = block_cin(b) + i * kEmbGrowth;
      d.dilation = kEmbBlockDilation[b];
      v(d.s1, d.c_in);
      v(d.h1, d.c_in);
      v(d.w1, (size_t)d.c_in * kEmbBn);
      v(d.s2, kEmbBn);
      v(d.h2, kEmbBn);
      v(d.wl, (size_t)3 * kEmbBn * kEmbGrowth);
      v(d.g1, (size_t)kEmbBn * kEmbGate);
      v(d.b1, kEmbGate);
      v(d.g2, (size_t)kEmbGate * kEmbGrowth);
      v(d.b2, kEmbGrowth);
    }
    EmbTransit& t = m.transit[b];
    t.c_in = kEmbBlockWidth[b];
    v(t.s, t.c_in);
    v(t.h, t.c_in);
    v(t.w, (size_t)t.c_in * (t.c_in / 2));
  }
  v(m.out_s, kEmbXvec);
  v(m.out_h, kEmbXvec);
  v(m.dense.w, (size_t)kEmbStats * dim);
  v(m.dense.scale, dim);
  v(m.dense.shift, dim);
}

size_t model_floats(int dim) {
  EmbModel m{};
  size_t at = 0;
  walk(m, dim, [&at](const float*&, size_t n) { at += (n + 63) & ~(size_t)63; });      // every tensor starts on a 256-byte boundary
  return at;
}

EmbModel model_of(const float* base, int dim) {
  EmbModel m{};
  size_t at = 0;
  walk(m, dim, [&at, base](const float*& f, size_t n) {
    f = base + at;
    at += (n + 63) & ~(size_t)63;
  });
  return m;
}

float* wr(const float* p) { return const_cast<float*>(p); }      // the host copy is written through the model's pointers

// scale = w / sqrt(var + eps), shift = b - mean * scale, in double, rounded once; without affine terms w = 1, b = 0
void fold_bn(const float* w, const float* b, const float* mean, const float* var, size_t c, const float* scale, const float* shift) {
  for (size_t i = 0; i < c; ++i) {
    const double s = (w ? (double)w[i] : 1.0) / std::sqrt((double)var[i] + kEmbBnEps);
    wr(scale)[i] = (float)s;
    wr(shift)[i] = (float)((b ? (double)b[i] : 0.0) - (double)mean[i] * s);
  }
}

// torch's [co][ci][taps] -> [(tap * ci_n + ci)][co]
void conv_transposed(const float* src, int co_n, int ci_n, int taps, const float* dst) {
  for (int co = 0; co < co_n; ++co)
    for (int ci = 0; ci < ci_n; ++ci)
      for (int k = 0; k < taps; ++k) wr(dst)[((size_t)k * ci_n + ci) * co_n + co] = src[((size_t)co * ci_n + ci) * taps + k];
}

// ---- a call's scratch -----------------------------------------------------------------------------------------------
struct Turn {
  float *a, *b[3], *head, *blk[kEmbBlocks], *h, *xvec, *segsum, *gates, *stats;
};

void carve_turn(Carve& c, Turn& t, size_t rows, size_t t2, size_t segs, size_t n_chunks) {
  t.a = c.take<float>(rows * kEmbFeat * kEmbHeadCh);
  for (int i = 0; i < 3; ++i) t.b[i] = c.take<float>(rows * (kEmbFeat / 2) * kEmbHeadCh);
  t.head = c.take<float>(rows * kEmbHeadOut);
  for (int b = 0; b < kEmbBlocks; ++b) t.blk[b] = c.take<float>(t2 * kEmbBlockWidth[b]);
  t.h = c.take<float>(t2 * kEmbBn);
  t.xvec = c.take<float>(t2 * kEmbXvec);
  t.segsum = c.take<float>(segs * kEmbBn);
  t.gates = c.take<float>(segs * kEmbGrowth);
  t.stats = c.take<float>(n_chunks * kEmbStats);
}

size_t turn_bytes(size_t rows, size_t t2, size_t segs, size_t n_chunks) {
  Carve c;
  Turn t{};
  carve_turn(c, t, rows, t2, segs, n_chunks);
  return c.used;
}

// Developer aid (CRISPY_DIAR_EMB_TIMELINE in the dev build): device time of a call by kernel family, to stderr.
enum Family { kFamHead, kFamTdnn, kFamGemm, kFamCam, kFamTransit, kFamPool, kFamCount };
struct Timeline {
  bool on = false;
  crispy::EventList ev;
  std::vector<int> family;      // family[i]: what ran between event i - 1 and event i
  hipError_t mark(int fam, hipStream_t st) {      // fam < 0: the start of a turn
    if (!on) return hipSuccess;
    hipError_t e = ev.ensure(ev.v.size() + 1, 0);
    if (e != hipSuccess) return e;
    family.push_back(fam);
    return hipEventRecord(ev.v.back(), st);
  }
  void report() const {
    if (!on) return;
    double ms[kFamCount] = {};
    for (size_t i = 1; i < ev.v.size(); ++i) {
      float t = 0.0f;
      if (family[i] >= 0 && hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[family[i]] += t;
    }
    std::fprintf(stderr, "crispy_diar_emb timeline: head %.3f ms, tdnn %.3f ms, dense gemms %.3f ms, cam %.3f ms, transits %.3f ms, pooling %.3f ms\n",
                 ms[kFamHead], ms[kFamTdnn], ms[kFamGemm], ms[kFamCam], ms[kFamTransit], ms[kFamPool]);
  }
};

// The network on n_chunks chunks of feature rows; frame_offset has been checked.
int emb_run(crispy_diar* h, const float* d_feats, const long* frame_offset, int n_chunks, float* d_emb, float* d_head, float* d_xvec,
            float* d_stats, hipStream_t st) {
  const int dim = h->emb_dim;
  const EmbModel m = model_of(h->emb_weights.p, dim);
  size_t max_chunks = (size_t)n_chunks;
  if (const char* e = crispy::dev_env("CRISPY_DIAR_EMB_TURN")) {      // developer knob: small turns, for the test of their bytes
    const int v = std::atoi(e);
    if (v > 0) max_chunks = std::min<size_t>(max_chunks, (size_t)v);
  }
  // turns: as many consecutive chunks as fit kScratchCap (one chunk of kEmbMaxRows rows does)
  struct Span { int c0, c1; size_t rows, t2, segs, tab; };
  std::vector<Span> turns;
  std::vector<int> tab;      // per turn: row_off, t2_off, seg_off, each [chunks + 1], relative to the turn
  size_t biggest = 0;
  for (int c0 = 0; c0 < n_chunks;) {
    Span s{c0, c0, 0, 0, 0, tab.size()};
    while (s.c1 < n_chunks && (size_t)(s.c1 - s.c0) < max_chunks) {
      const size_t r = (size_t)(frame_offset[s.c1 + 1] - frame_offset[s.c1]), q = (size_t)emb_frames((long)r), g = (size_t)emb_segments((long)q);
      if (s.c1 > s.c0 && turn_bytes(s.rows + r, s.t2 + q, s.segs + g, (size_t)(s.c1 - s.c0 + 1)) > kScratchCap) break;
      s.rows += r; s.t2 += q; s.segs += g; ++s.c1;
    }
    const int nc = s.c1 - s.c0;
    int r = 0, q = 0, g = 0;
    std::vector<int> ro(1, 0), qo(1, 0), go(1, 0);
    for (int c = s.c0; c < s.c1; ++c) {
      const long n = frame_offset[c + 1] - frame_offset[c];
      r += (int)n; q += (int)emb_frames(n); g += (int)emb_segments(emb_frames(n));
      ro.push_back(r); qo.push_back(q); go.push_back(g);
    }
    tab.insert(tab.end(), ro.begin(), ro.end());
    tab.insert(tab.end(), qo.begin(), qo.end());
    tab.insert(tab.end(), go.begin(), go.end());
    biggest = std::max(biggest, turn_bytes(s.rows, s.t2, s.segs, (size_t)nc));
    turns.push_back(s);
    c0 = s.c1;
  }
  HIP_TRY(h->scratch.grow(biggest));
  HIP_TRY(h->emb_tab.grow(tab.size() * sizeof(int)));
  HIP_TRY(hipMemcpyAsync(h->emb_tab.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
  Timeline tl;
  tl.on = crispy::dev_env("CRISPY_DIAR_EMB_TIMELINE") != nullptr;
  for (const Span& s : turns) {
    const int nc = s.c1 - s.c0;
    Carve c;
    c.p = h->scratch.p;
    Turn t{};
    carve_turn(c, t, s.rows, s.t2, s.segs, (size_t)nc);
    EmbTables tb{};
    tb.row_off = h->emb_tab.as<int>() + s.tab;
    tb.t2_off = tb.row_off + (nc + 1);
    tb.seg_off = tb.t2_off + (nc + 1);
    tb.n_chunks = nc;
    for (int k = 0; k < nc; ++k) {
      tb.max_rows = std::max(tb.max_rows, tab[s.tab + k + 1] - tab[s.tab + k]);
      tb.max_t2 = std::max(tb.max_t2, tab[s.tab + nc + 1 + k + 1] - tab[s.tab + nc + 1 + k]);
    }
    const size_t row0 = (size_t)frame_offset[s.c0];
    size_t q0 = 0;      // positions after the tdnn in front of this turn
    for (int k = 0; k < s.c0; ++k) q0 += (size_t)emb_frames(frame_offset[k + 1] - frame_offset[k]);
    const float* x = d_feats + row0 * kEmbFeat;
    float* head = d_head ? d_head + row0 * kEmbHeadOut : t.head;
    float* xvec = d_xvec ? d_xvec + q0 * kEmbXvec : t.xvec;
    float* stats = d_stats ? d_stats + (size_t)s.c0 * kEmbStats : t.stats;
    HIP_TRY(tl.mark(-1, st));
    // head: conv1 -> a; layer1: (a) -> b1; layer2: (b1) -> b1; conv2 -> head
    HIP_TRY(launch_emb_head_conv(0, m, tb, x, nullptr, t.a, st));
    HIP_TRY(launch_emb_head_conv(1, m, tb, t.a, nullptr, t.b[0], st));
    HIP_TRY(launch_emb_head_conv(3, m, tb, t.a, nullptr, t.b[1], st));
    HIP_TRY(launch_emb_head_conv(2, m, tb, t.b[0], t.b[1], t.b[2], st));
    HIP_TRY(launch_emb_head_conv(4, m, tb, t.b[2], nullptr, t.b[0], st));
    HIP_TRY(launch_emb_head_conv(5, m, tb, t.b[0], t.b[2], t.b[1], st));
    HIP_TRY(launch_emb_head_conv(6, m, tb, t.b[1], nullptr, t.b[0], st));
    HIP_TRY(launch_emb_head_conv(8, m, tb, t.b[1], nullptr, t.b[2], st));
    HIP_TRY(launch_emb_head_conv(7, m, tb, t.b[0], t.b[2], t.a, st));
    HIP_TRY(launch_emb_head_conv(9, m, tb, t.a, nullptr, t.b[0], st));
    HIP_TRY(launch_emb_head_conv(10, m, tb, t.b[0], t.a, t.b[1], st));
    HIP_TRY(launch_emb_head_conv(11, m, tb, t.b[1], nullptr, head, st));
    HIP_TRY(tl.mark(kFamHead, st));
    HIP_TRY(launch_emb_tdnn(m, tb, head, t.blk[0], st));
    HIP_TRY(tl.mark(kFamTdnn, st));
    int l = 0;
    for (int b = 0; b < kEmbBlocks; ++b) {
      const int width = kEmbBlockWidth[b];
      for (int i = 0; i < kEmbBlockLayers[b]; ++i, ++l) {
        const EmbDense& d = m.layer[l];
        HIP_TRY(launch_emb_gemm(t.blk[b], width, d.c_in, d.s1, d.h1, d.w1, kEmbBn, d.s2, d.h2, t.h, kEmbBn, (long)s.t2, st));
        HIP_TRY(tl.mark(kFamGemm, st));
        HIP_TRY(launch_emb_gates(d, tb, t.h, t.segsum, t.gates, st));
        HIP_TRY(launch_emb_local(d, tb, t.h, t.gates, t.blk[b], width, st));
        HIP_TRY(tl.mark(kFamCam, st));
      }
      const EmbTransit& tr = m.transit[b];
      const bool last = b == kEmbBlocks - 1;
      HIP_TRY(launch_emb_gemm(t.blk[b], width, width, tr.s, tr.h, tr.w, width / 2, last ? m.out_s : nullptr, last ? m.out_h : nullptr,
                              last ? xvec : t.blk[b + 1], last ? kEmbXvec : kEmbBlockWidth[b + 1], (long)s.t2, st));
      HIP_TRY(tl.mark(kFamTransit, st));
    }
    HIP_TRY(launch_emb_pool(tb, xvec, stats, st));
    HIP_TRY(launch_emb_dense(m, tb, stats, d_emb + (size_t)s.c0 * dim, st));
    HIP_TRY(tl.mark(kFamPool, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  tl.report();
  return CRISPY_OK;
}

int check_loaded(const char* who, const crispy_diar* h) {
  if (!h->emb_weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no embedding network is loaded (crispy_diar_emb_load comes first)", who);
  return CRISPY_OK;
}

int check_rows(const char* who, const long* frame_offset, int n_chunks) {
  for (int c = 0; c < n_chunks; ++c) {
    const long n = frame_offset[c + 1] - frame_offset[c];
    if (n < kEmbMinRows || n > kEmbMaxRows)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: chunk %d has %ld rows, outside %d ... %d", who, c, n, kEmbMinRows, kEmbMaxRows);
  }
  return CRISPY_OK;
}

}  // namespace

extern "C" {

long crispy_diar_emb_frames(long rows) try {
  return emb_frames(rows);
}
CRISPY_CATCH_RET("crispy_diar_emb_frames")

int crispy_diar_emb_tensor_spec(int i, int dim, const char** name, long* count) try {
  const char* who = "crispy_diar_emb_tensor_spec";
  const std::vector<Spec>& sp = specs();
  if (i < 0 || i >= (int)sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: i %d outside 0 ... %zu", who, i, sp.size() - 1);
  if (dim < 1 || dim > kEmbMaxDim) return fail(CRISPY_ERR_INVALID_ARG, "%s: dim %d outside 1 ... %d", who, dim, kEmbMaxDim);
  if (name) *name = sp[i].name.c_str();
  if (count) *count = (long)(sp[i].count + sp[i].per_dim * (size_t)dim);
  return (int)sp.size();
}
CRISPY_CATCH_RET("crispy_diar_emb_tensor_spec")

int crispy_diar_emb_load(void* hv, const char* const* names, const float* const* data, const long* count, int n_tensors) try {
  const char* who = "crispy_diar_emb_load";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!names || !data || !count) return fail(CRISPY_ERR_INVALID_ARG, "%s: names, data or count is NULL", who);
  const std::vector<Spec>& sp = specs();
  if (n_tensors < 1 || n_tensors > 4 * (int)sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_tensors %d outside 1 ... %zu", who, n_tensors, 4 * sp.size());
  std::map<std::string, size_t> index;
  for (size_t k = 0; k < sp.size(); ++k) index[sp[k].name] = k;
  // the width first: every other count is checked against it
  int dim = 0;
  for (int i = 0; i < n_tensors; ++i)
    if (names[i] && std::strcmp(names[i], "xvector.dense.linear.weight") == 0) {
      if (count[i] < kEmbStats || count[i] % kEmbStats != 0 || count[i] / kEmbStats > kEmbMaxDim)
        return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has %ld values, expected %d x (1 ... %d)", who, names[i], count[i], kEmbStats, kEmbMaxDim);
      dim = (int)(count[i] / kEmbStats);
      break;
    }
  std::vector<const float*> src(sp.size(), nullptr);
  for (int i = 0; i < n_tensors; ++i) {
    if (!names[i]) return fail(CRISPY_ERR_INVALID_ARG, "%s: names[%d] is NULL", who, i);
    const auto it = index.find(names[i]);
    if (it == index.end()) return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown tensor '%.200s'", who, names[i]);
    const size_t k = it->second;
    if (src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' given twice", who, names[i]);
    if (!data[i]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a NULL pointer", who, names[i]);
    if (dim == 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor 'xvector.dense.linear.weight' is missing", who);
    const size_t want = sp[k].count + sp[k].per_dim * (size_t)dim;
    if (count[i] != (long)want) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has %ld values, expected %zu", who, names[i], count[i], want);
    const bool is_var = sp[k].name.size() > 12 && sp[k].name.compare(sp[k].name.size() - 12, 12, ".running_var") == 0;
    for (size_t j = 0; j < want; ++j) {
      if (!std::isfinite(data[i][j])) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a non-finite value at %zu", who, names[i], j);
      if (is_var && data[i][j] < 0.0f) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a negative variance at %zu", who, names[i], j);
    }
    src[k] = data[i];
  }
  for (size_t k = 0; k < sp.size(); ++k)
    if (!src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' is missing", who, sp[k].name.c_str());
  auto get = [&](const std::string& name) { return src[index.at(name)]; };
  auto bn = [&](const std::string& p, size_t c, const float* scale, const float* shift, bool affine = true) {
    fold_bn(affine ? get(p + ".weight") : nullptr, affine ? get(p + ".bias") : nullptr, get(p + ".running_mean"), get(p + ".running_var"), c, scale,
            shift);
  };
  const size_t total = model_floats(dim);
  std::vector<float> blob(total, 0.0f);
  const EmbModel m = model_of(blob.data(), dim);
  for (int i = 0; i < kEmbHeadConvs; ++i) {
    // [co][ci][kf][kt] -> [(kf * ks + kt) * ci_n + ci][co]
    conv_transposed(get(std::string(kHeadConv[i]) + ".weight"), kEmbHeadCh, head_cin(i), head_ks(i) * head_ks(i), m.head[i].w);
    bn(kHeadBn[i], kEmbHeadCh, m.head[i].scale, m.head[i].shift);
  }
  conv_transposed(get("xvector.tdnn.linear.weight"), kEmbInit, kEmbHeadOut, kEmbTdnnTaps, m.tdnn.w);
  bn("xvector.tdnn.nonlinear.batchnorm", kEmbInit, m.tdnn.scale, m.tdnn.shift);
  int l = 0;
  for (int b = 0; b < kEmbBlocks; ++b) {
    for (int i = 0; i < kEmbBlockLayers[b]; ++i, ++l) {
      const EmbDense& d = m.layer[l];
      const std::string p = layer_name(b, i);
      bn(p + ".nonlinear1.batchnorm", (size_t)d.c_in, d.s1, d.h1);
      conv_transposed(get(p + ".linear1.weight"), kEmbBn, d.c_in, 1, d.w1);
      bn(p + ".nonlinear2.batchnorm", kEmbBn, d.s2, d.h2);
      conv_transposed(get(p + ".cam_layer.linear_local.weight"), kEmbGrowth, kEmbBn, 3, d.wl);
      conv_transposed(get(p + ".cam_layer.linear1.weight"), kEmbGate, kEmbBn, 1, d.g1);
      conv_transposed(get(p + ".cam_layer.linear2.weight"), kEmbGrowth, kEmbGate, 1, d.g2);
      std::memcpy(wr(d.b1), get(p + ".cam_layer.linear1.bias"), kEmbGate * sizeof(float));
      std::memcpy(wr(d.b2), get(p + ".cam_layer.linear2.bias"), kEmbGrowth * sizeof(float));
    }
    const EmbTransit& t = m.transit[b];
    bn(transit_name(b) + ".nonlinear.batchnorm", (size_t)t.c_in, t.s, t.h);
    conv_transposed(get(transit_name(b) + ".linear.weight"), t.c_in / 2, t.c_in, 1, t.w);
  }
  bn("xvector.out_nonlinear.batchnorm", kEmbXvec, m.out_s, m.out_h);
  conv_transposed(get("xvector.dense.linear.weight"), dim, kEmbStats, 1, m.dense.w);
  bn("xvector.dense.nonlinear.batchnorm", (size_t)dim, m.dense.scale, m.dense.shift, false);
  for (size_t i = 0; i < total; ++i)
    if (!std::isfinite(blob[i])) return fail(CRISPY_ERR_INVALID_ARG, "%s: a folded BatchNorm (weight / sqrt(running_var + 1e-5)) is not finite", who);
  HIP_TRY(hipSetDevice(h->device));
  crispy::DevBuf<float> fresh;
  HIP_TRY(fresh.alloc(total * sizeof(float)));
  HIP_TRY(hipMemcpy(fresh.p, blob.data(), total * sizeof(float), hipMemcpyHostToDevice));
  h->emb_weights = std::move(fresh);      // the copy of an earlier load goes with `fresh`
  h->emb_dim = dim;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_emb_load")

int crispy_diar_emb_loaded(void* hv) try {
  const crispy_diar* h = static_cast<const crispy_diar*>(hv);
  return h && h->emb_weights.p ? 1 : 0;
}
CRISPY_CATCH_RET("crispy_diar_emb_loaded")

int crispy_diar_emb_dim(void* hv) try {
  const crispy_diar* h = static_cast<const crispy_diar*>(hv);
  return h && h->emb_weights.p ? h->emb_dim : 0;
}
CRISPY_CATCH_RET("crispy_diar_emb_dim")

int crispy_diar_emb_forward_device(void* hv, const float* d_feats, const long* frame_offset, int n_chunks, float* d_emb, float* d_head,
                                   float* d_xvec, float* d_stats, void* hip_stream) try {
  const char* who = "crispy_diar_emb_forward_device";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (n_chunks < 1 || n_chunks > kMaxChunks) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_chunks %d outside 1 ... %d", who, n_chunks, kMaxChunks);
  if (!frame_offset) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset is NULL", who);
  if (frame_offset[0] != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset[0] is %ld, not 0", who, frame_offset[0]);
  int rc = check_rows(who, frame_offset, n_chunks);
  if (rc != CRISPY_OK) return rc;
  rc = check_loaded(who, h);      // in front of the pointers: without a network the width is 0 and d_emb has no bytes
  if (rc != CRISPY_OK) return rc;
  if (!d_feats || !d_emb) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_feats or d_emb is NULL", who);
  HIP_TRY(hipSetDevice(h->device));
  return emb_run(h, d_feats, frame_offset, n_chunks, d_emb, d_head, d_xvec, d_stats, hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_diar_emb_forward_device")

int crispy_diar_embed_device(void* hv, const void* d_pcm, int pcm_format, const long* first, const long* len, int n_chunks, float scale,
                             float* d_emb, void* hip_stream) try {
  const char* who = "crispy_diar_embed_device";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (n_chunks < 1 || n_chunks > kMaxChunks) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_chunks %d outside 1 ... %d", who, n_chunks, kMaxChunks);
  std::vector<long> off((size_t)n_chunks + 1, 0);
  int rc = crispy_diar_fbank_device(hv, nullptr, pcm_format, first, len, n_chunks, scale, nullptr, nullptr, off.data(), nullptr);      // checks and sizes
  if (rc != CRISPY_OK) return rc;
  rc = check_rows(who, off.data(), n_chunks);
  if (rc != CRISPY_OK) return rc;
  rc = check_loaded(who, h);      // in front of the pointers: without a network the width is 0 and the embeddings have no bytes
  if (rc != CRISPY_OK) return rc;
  if (!d_pcm || !d_emb) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_pcm or d_emb is NULL", who);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(h->io.grow((size_t)off[n_chunks] * kEmbFeat * sizeof(float)));
  float* d_feats = h->io.as<float>();      // the feature rows stay on the device
  rc = crispy_diar_fbank_device(hv, d_pcm, pcm_format, first, len, n_chunks, scale, d_feats, nullptr, off.data(), hip_stream);
  if (rc != CRISPY_OK) return rc;
  return emb_run(h, d_feats, off.data(), n_chunks, d_emb, nullptr, nullptr, nullptr, hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_diar_embed_device")

int crispy_diar_embed(void* hv, const void* pcm, int pcm_format, const long* first, const long* len, int n_chunks, float scale, float* emb) try {
  const char* who = "crispy_diar_embed";
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (n_chunks < 1 || n_chunks > kMaxChunks) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_chunks %d outside 1 ... %d", who, n_chunks, kMaxChunks);
  std::vector<long> off((size_t)n_chunks + 1, 0);
  int rc = crispy_diar_fbank_device(hv, nullptr, pcm_format, first, len, n_chunks, scale, nullptr, nullptr, off.data(), nullptr);      // checks and sizes
  if (rc != CRISPY_OK) return rc;
  rc = check_rows(who, off.data(), n_chunks);
  if (rc != CRISPY_OK) return rc;
  rc = check_loaded(who, h);      // in front of the pointers: without a network the width is 0 and the embeddings have no bytes
  if (rc != CRISPY_OK) return rc;
  if (!pcm || !emb) return fail(CRISPY_ERR_INVALID_ARG, "%s: pcm or emb is NULL", who);
  long lo = first[0], hi = 0;      // the samples the chunks read (every chunk has rows)
  for (int c = 0; c < n_chunks; ++c) {
    lo = std::min(lo, first[c]);
    hi = std::max(hi, first[c] + len[c]);
  }
  std::vector<long> shifted(first, first + n_chunks);
  for (long& f : shifted) f -= lo;
  const size_t elem = pcm_format == CRISPY_PCM_F32 ? sizeof(float) : sizeof(short);
  const size_t pcm_bytes = ((size_t)(hi - lo) * elem + 255) & ~(size_t)255;
  const size_t feat_bytes = ((size_t)off[n_chunks] * kEmbFeat * sizeof(float) + 255) & ~(size_t)255;
  const size_t emb_bytes = (size_t)n_chunks * h->emb_dim * sizeof(float);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(h->io.grow(pcm_bytes + feat_bytes + emb_bytes));
  float* d_feats = reinterpret_cast<float*>(h->io.p + pcm_bytes);
  float* d_emb = reinterpret_cast<float*>(h->io.p + pcm_bytes + feat_bytes);
  HIP_TRY(hipMemcpyAsync(h->io.p, static_cast<const char*>(pcm) + (size_t)lo * elem, (size_t)(hi - lo) * elem, hipMemcpyHostToDevice, h->stream));
  rc = crispy_diar_fbank_device(hv, h->io.p, pcm_format, shifted.data(), len, n_chunks, scale, d_feats, nullptr, off.data(), nullptr);
  if (rc != CRISPY_OK) return rc;
  rc = emb_run(h, d_feats, off.data(), n_chunks, d_emb, nullptr, nullptr, nullptr, h->stream);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(emb, d_emb, emb_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_embed")

}  // extern "C"

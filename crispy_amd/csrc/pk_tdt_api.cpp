// pk_tdt_api.cpp -- host side of Parakeet's TDT decoder (include/crispy_hip.h, "Parakeet TDT decoder"; kernels in pk_tdt.hip, the
// encoder projector on pk_gemm.hip): the tensor table, the layout of the handle's device copy, the limits, the workspace, the
// loop that enqueues steps in groups, and the word grouping, which needs no device.
#include <algorithm>
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

const crispy_pk_tdt_config* as_cfg(const void* p) { return static_cast<const crispy_pk_tdt_config*>(p); }

// the supported set; a field outside it is named
int check_config(const char* who, const crispy_pk_tdt_config* c) {
  if (!c) return fail(CRISPY_ERR_INVALID_ARG, "%s: cfg is NULL", who);
  if (c->hidden < 32 || c->hidden > 4096 || c->hidden % 32 != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: hidden %d is not a multiple of 32 in 32 ... 4096", who, c->hidden);
  if (c->decoder_hidden < 128 || c->decoder_hidden > kTdtMaxWidth || c->decoder_hidden % 128 != 0)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: decoder_hidden %d is not a multiple of 128 in 128 ... %d", who, c->decoder_hidden, kTdtMaxWidth);
  if (c->decoder_layers < 1 || c->decoder_layers > kTdtMaxLayers)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: decoder_layers %d outside 1 ... %d", who, c->decoder_layers, kTdtMaxLayers);
  if (c->vocab < 2 || c->vocab > kTdtMaxVocab) return fail(CRISPY_ERR_INVALID_ARG, "%s: vocab %d outside 2 ... %d", who, c->vocab, kTdtMaxVocab);
  if (c->blank < 0 || c->blank >= c->vocab) return fail(CRISPY_ERR_INVALID_ARG, "%s: blank %d outside 0 ... vocab - 1 (%d)", who, c->blank, c->vocab - 1);
  if (c->n_durations < 1 || c->n_durations > kTdtMaxDurations)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: n_durations %d outside 1 ... %d", who, c->n_durations, kTdtMaxDurations);
  for (int i = 0; i < c->n_durations; ++i) {
    if (c->durations[i] < 0 || c->durations[i] > kTdtMaxFrames)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: durations[%d] %d outside 0 ... %d", who, i, c->durations[i], kTdtMaxFrames);
    if (i > 0 && c->durations[i] <= c->durations[i - 1])
      return fail(CRISPY_ERR_INVALID_ARG, "%s: durations[%d] %d does not ascend from %d", who, i, c->durations[i], c->durations[i - 1]);
  }
  if (c->max_symbols_per_step < 1 || c->max_symbols_per_step > kTdtMaxSymbols)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: max_symbols_per_step %d outside 1 ... %d", who, c->max_symbols_per_step, kTdtMaxSymbols);
  return CRISPY_OK;
}

// ---- the tensors crispy_pk_tdt_load takes, in the order of ParakeetForTDT's state dict behind the encoder --------------------
struct Spec {
  std::string name;
  size_t count;
};

std::vector<Spec> make_specs(const crispy_pk_tdt_config& c) {
  std::vector<Spec> s;
  const size_t H = (size_t)c.hidden, D = (size_t)c.decoder_hidden, W = (size_t)c.vocab + (size_t)c.n_durations;
  s.push_back({"encoder_projector.weight", D * H});
  s.push_back({"encoder_projector.bias", D});
  s.push_back({"decoder.embedding.weight", (size_t)c.vocab * D});
  for (int l = 0; l < c.decoder_layers; ++l) {
    const std::string n = std::to_string(l);
    s.push_back({"decoder.lstm.weight_ih_l" + n, 4 * D * D});
    s.push_back({"decoder.lstm.weight_hh_l" + n, 4 * D * D});
    s.push_back({"decoder.lstm.bias_ih_l" + n, 4 * D});
    s.push_back({"decoder.lstm.bias_hh_l" + n, 4 * D});
  }
  s.push_back({"decoder.decoder_projector.weight", D * D});
  s.push_back({"decoder.decoder_projector.bias", D});
  s.push_back({"joint.head.weight", W * D});
  s.push_back({"joint.head.bias", W});
  return s;
}

// ---- the device copy ------------------------------------------------------------------------------------------------
size_t pad_cols(const crispy_pk_tdt_config& c) { return ((size_t)c.vocab + (size_t)c.n_durations + kTdtCols - 1) / kTdtCols * kTdtCols; }

// Visits every field of the model in a fixed order with its element count: once to add up the size, once to place the fields.
template <class V>
void walk(TdtModel& m, const crispy_pk_tdt_config& c, V&& v) {
  const size_t H = (size_t)c.hidden, D = (size_t)c.decoder_hidden, P = pad_cols(c);
  v(m.proj_w, H * D);
  v(m.proj_b, D);
  v(m.emb, (size_t)c.vocab * D);
  for (int l = 0; l < c.decoder_layers; ++l) {
    v(m.lstm_w[l], 2 * D * 4 * D);
    v(m.lstm_b[l], 4 * D);
  }
  v(m.dp_w, D * D);
  v(m.dp_b, D);
  v(m.head_w, D * P);
  v(m.head_b, P);
}

void fill_scalars(TdtModel& m, const crispy_pk_tdt_config& c) {
  m.D = c.decoder_hidden;
  m.L = c.decoder_layers;
  m.V = c.vocab;
  m.n_dur = c.n_durations;
  m.blank = c.blank;
  m.n_pad = (int)pad_cols(c);
  for (int i = 0; i < kTdtMaxDurations; ++i) m.dur[i] = i < c.n_durations ? c.durations[i] : 0;
}

size_t model_floats(const crispy_pk_tdt_config& c) {
  TdtModel m{};
  size_t at = 0;
  walk(m, c, [&at](const float*&, size_t n) { at += (n + 63) & ~(size_t)63; });      // every tensor starts on a 256-byte boundary
  return at;
}

TdtModel model_of(const float* base, const crispy_pk_tdt_config& c) {
  TdtModel m{};
  size_t at = 0;
  walk(m, c, [&at, base](const float*& f, size_t n) {
    f = base + at;
    at += (n + 63) & ~(size_t)63;
  });
  fill_scalars(m, c);
  return m;
}

float* wr(const float* p) { return const_cast<float*>(p); }      // the host copy is written through the model's pointers

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
  int* off;
  long* step_off;
  int *t, *tok, *run, *budget, *done, *finished, *part_idx;
  float *h, *c, *hn, *g, *p, *part_val, *dur_logit;
};

void carve(Carve& c, Work& w, const crispy_pk_tdt_config& cfg, size_t n, size_t total_frames) {
  const size_t D = (size_t)cfg.decoder_hidden, L = (size_t)cfg.decoder_layers, tiles = pad_cols(cfg) / kTdtCols;
  w.off = c.take<int>(n + 1);
  w.step_off = c.take<long>(n + 1);
  w.t = c.take<int>(n);
  w.tok = c.take<int>(n);
  w.run = c.take<int>(n);
  w.budget = c.take<int>(n);
  w.done = c.take<int>(n);
  w.finished = c.take<int>(1);
  w.part_idx = c.take<int>(n * tiles);
  w.h = c.take<float>(L * n * D);
  w.c = c.take<float>(L * n * D);
  w.hn = c.take<float>(L * n * D);
  w.g = c.take<float>(n * D);
  w.p = c.take<float>(total_frames * D);
  w.part_val = c.take<float>(n * tiles);
  w.dur_logit = c.take<float>(n * kTdtMaxDurations);
}

int check_call(const char* who, const crispy_pk_tdt* h, const long* frame_offset, int n_clips) {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (n_clips < 1 || n_clips > kMaxClips) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_clips %d outside 1 ... %d", who, n_clips, kMaxClips);
  if (!frame_offset) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset is NULL", who);
  if (frame_offset[0] != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: frame_offset[0] is %ld, not 0", who, frame_offset[0]);
  for (int c = 0; c < n_clips; ++c) {
    const long n = frame_offset[c + 1] - frame_offset[c];
    if (n < 0 || n > kTdtMaxFrames) return fail(CRISPY_ERR_INVALID_ARG, "%s: clip %d has %ld frames, outside 0 ... %d", who, c, n, kTdtMaxFrames);
  }
  if (!h->weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no decoder is loaded (crispy_pk_tdt_load comes first)", who);
  return CRISPY_OK;
}

long total_budget(const crispy_pk_tdt_config& cfg, const long* frame_offset, int n_clips) {
  long sum = 0;
  for (int c = 0; c < n_clips; ++c) sum += tdt_max_steps(cfg.max_symbols_per_step, frame_offset[c + 1] - frame_offset[c]);
  return sum;
}

// Developer aid (CRISPY_PK_TDT_TIMELINE in the dev build): device time of a call by stage, to stderr.  Events around every launch
// serialise nothing here -- the launches are on one stream -- but cost host time; the call's own time is measured without it.
enum Stage { kStProj, kStPredict, kStJoint, kStAdvance, kStCount };
struct Timeline {
  bool on = false;
  crispy::EventList ev;
  std::vector<int> stage;
  hipError_t mark(int s, hipStream_t st) {
    if (!on) return hipSuccess;
    hipError_t e = ev.ensure(ev.v.size() + 1, 0);
    if (e != hipSuccess) return e;
    stage.push_back(s);
    return hipEventRecord(ev.v.back(), st);
  }
  void report(long steps) const {
    if (!on) return;
    double ms[kStCount] = {};
    for (size_t i = 1; i < ev.v.size(); ++i) {
      float t = 0.0f;
      if (stage[i] >= 0 && hipEventElapsedTime(&t, ev[i - 1], ev[i]) == hipSuccess) ms[stage[i]] += t;
    }
    std::fprintf(stderr, "crispy_pk_tdt timeline: %ld steps enqueued, projector %.3f ms, prediction %.3f ms, joint %.3f ms, advance %.3f ms\n", steps,
                 ms[kStProj], ms[kStPredict], ms[kStJoint], ms[kStAdvance]);
  }
};

// The loop on n_clips clips of frames; the arguments have been checked.
int tdt_run(crispy_pk_tdt* h, const float* d_frames, const long* frame_offset, int n_clips, int* d_steps, int* d_n_steps, float* d_proj_tap,
            float* d_logits_tap, hipStream_t st) {
  const crispy_pk_tdt_config& cfg = h->cfg;
  const size_t D = (size_t)cfg.decoder_hidden;
  std::vector<int> off((size_t)n_clips + 1, 0);
  std::vector<long> step_off((size_t)n_clips + 1, 0);
  long max_budget = 0;
  for (int c = 0; c < n_clips; ++c) {
    const long b = tdt_max_steps(cfg.max_symbols_per_step, frame_offset[c + 1] - frame_offset[c]);
    off[(size_t)c + 1] = (int)frame_offset[c + 1];
    step_off[(size_t)c + 1] = step_off[(size_t)c] + b;
    max_budget = std::max(max_budget, b);
  }
  const size_t total_frames = (size_t)frame_offset[n_clips];
  Carve size;
  Work w{};
  carve(size, w, cfg, (size_t)n_clips, total_frames);
  if (size.used > h->scratch.bytes) {      // before any launch: what does not fit is refused with nothing enqueued
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (size.used > free_b + h->scratch.bytes)
      return fail(CRISPY_ERR_OOM, "crispy_pk_tdt_decode: the call needs a workspace of %zu bytes, the device has %zu free", size.used, free_b + h->scratch.bytes);
    HIP_TRY(h->scratch.grow(size.used));
  }
  Carve place;
  place.p = h->scratch.p;
  carve(place, w, cfg, (size_t)n_clips, total_frames);
  const TdtModel m = model_of(h->weights.p, cfg);
  TdtState s{};
  s.n_clips = n_clips;
  s.tiles = m.n_pad / kTdtCols;
  s.off = w.off;
  s.step_off = w.step_off;
  s.t = w.t; s.tok = w.tok; s.run = w.run; s.budget = w.budget; s.done = w.done; s.finished = w.finished;
  s.h = w.h; s.c = w.c; s.hn = w.hn; s.g = w.g; s.p = w.p;
  s.part_val = w.part_val; s.part_idx = w.part_idx; s.dur_logit = w.dur_logit;
  s.steps = d_steps; s.n_steps = d_n_steps; s.logits_tap = d_logits_tap;
  Timeline tl;
  tl.on = crispy::dev_env("CRISPY_PK_TDT_TIMELINE") != nullptr;
  int group = kTdtGroup;
  if (const char* e = crispy::dev_env("CRISPY_PK_TDT_GROUP")) group = std::max(1, std::atoi(e));
  HIP_TRY(hipMemcpyAsync(w.off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.step_off, step_off.data(), step_off.size() * sizeof(long), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_tdt_init(m, s, st));
  long enqueued = 0;
  if (total_frames > 0) {
    HIP_TRY(tl.mark(-1, st));
    HIP_TRY(launch_gemm(kGemmScale, d_frames, cfg.hidden, m.proj_w, m.proj_b, cfg.decoder_hidden, 1.0f, nullptr, w.p, (long)total_frames, st));
    HIP_TRY(tl.mark(kStProj, st));
    if (d_proj_tap) HIP_TRY(hipMemcpyAsync(d_proj_tap, w.p, total_frames * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(tl.mark(-1, st));
    HIP_TRY(launch_tdt_predict(m, s, st));      // the start: embedding[blank] on the zero state
    HIP_TRY(tl.mark(kStPredict, st));
    // At most max_budget steps: by then every clip has used its budget, whatever the network says.
    while (enqueued < max_budget) {
      const long n = std::min<long>(group, max_budget - enqueued);
      for (long i = 0; i < n; ++i) {
        HIP_TRY(launch_tdt_joint(m, s, st));
        HIP_TRY(tl.mark(kStJoint, st));
        HIP_TRY(launch_tdt_advance(m, s, st));
        HIP_TRY(tl.mark(kStAdvance, st));
        HIP_TRY(launch_tdt_predict(m, s, st));
        HIP_TRY(tl.mark(kStPredict, st));
      }
      enqueued += n;
      int finished = 0;
      HIP_TRY(hipMemcpyAsync(&finished, w.finished, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (finished >= n_clips) break;
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  tl.report(enqueued);
  return CRISPY_OK;
}

// one UTF-8 piece: does it begin with U+2581 (E2 96 81)?
bool has_marker(const char* s) { return (unsigned char)s[0] == 0xE2 && (unsigned char)s[1] == 0x96 && (unsigned char)s[2] == 0x81; }

}  // namespace

extern "C" {

int crispy_pk_tdt_create(int device, void** out) try {
  if (!out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_pk_tdt_create: out is NULL");
  *out = nullptr;
  const int rc = crispy::check_device(device, "crispy_pk_tdt_create");
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  crispy_pk_tdt* h = new crispy_pk_tdt;
  h->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    h->stream = nullptr;
    delete h;
    return fail(CRISPY_ERR_HIP, "crispy_pk_tdt_create: hipStreamCreate: %s", hipGetErrorString(e));
  }
  *out = h;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_tdt_create")

void crispy_pk_tdt_destroy(void* hv) try {
  crispy_pk_tdt* h = static_cast<crispy_pk_tdt*>(hv);
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}
CRISPY_CATCH_VOID("crispy_pk_tdt_destroy")

long crispy_pk_tdt_max_steps(const void* cfg, long frames) try {
  const int rc = check_config("crispy_pk_tdt_max_steps", as_cfg(cfg));
  if (rc != CRISPY_OK) return rc;
  if (frames > kTdtMaxFrames) return fail(CRISPY_ERR_INVALID_ARG, "crispy_pk_tdt_max_steps: frames %ld outside 0 ... %d", frames, kTdtMaxFrames);
  return tdt_max_steps(as_cfg(cfg)->max_symbols_per_step, frames);
}
CRISPY_CATCH_RET("crispy_pk_tdt_max_steps")

int crispy_pk_tdt_tensor_spec(const void* cfg, int i, const char** name, long* count) try {
  const char* who = "crispy_pk_tdt_tensor_spec";
  const int rc = check_config(who, as_cfg(cfg));
  if (rc != CRISPY_OK) return rc;
  static thread_local std::vector<Spec> sp;      // *name stays valid until this thread's next call
  sp = make_specs(*as_cfg(cfg));
  if (i < 0 || i >= (int)sp.size()) return fail(CRISPY_ERR_INVALID_ARG, "%s: i %d outside 0 ... %zu", who, i, sp.size() - 1);
  if (name) *name = sp[(size_t)i].name.c_str();
  if (count) *count = (long)sp[(size_t)i].count;
  return (int)sp.size();
}
CRISPY_CATCH_RET("crispy_pk_tdt_tensor_spec")

int crispy_pk_tdt_load(void* hv, const void* cfgv, const char* const* names, const float* const* data, const long* count, int n_tensors) try {
  const char* who = "crispy_pk_tdt_load";
  crispy_pk_tdt* h = static_cast<crispy_pk_tdt*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_config(who, as_cfg(cfgv));
  if (rc != CRISPY_OK) return rc;
  const crispy_pk_tdt_config cfg = *as_cfg(cfgv);
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
    for (size_t j = 0; j < sp[k].count; ++j)
      if (!std::isfinite(data[i][j])) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' has a non-finite value at %zu", who, names[i], j);
    src[k] = data[i];
  }
  for (size_t k = 0; k < sp.size(); ++k)
    if (!src[k]) return fail(CRISPY_ERR_INVALID_ARG, "%s: tensor '%s' is missing", who, sp[k].name.c_str());
  auto get = [&](const std::string& name) { return src[index.at(name)]; };
  const size_t H = (size_t)cfg.hidden, D = (size_t)cfg.decoder_hidden, V = (size_t)cfg.vocab, W = V + (size_t)cfg.n_durations, P = pad_cols(cfg);
  const size_t total = model_floats(cfg);
  std::vector<float> blob(total, 0.0f);      // the head's padding columns stay zero
  const TdtModel m = model_of(blob.data(), cfg);
  // torch's [out][in] -> [in][ld] at column o
  auto transposed = [](const float* w, size_t out_n, size_t in_n, const float* dst, size_t ld) {
    for (size_t o = 0; o < out_n; ++o)
      for (size_t i = 0; i < in_n; ++i) wr(dst)[i * ld + o] = w[o * in_n + i];
  };
  transposed(get("encoder_projector.weight"), D, H, m.proj_w, D);
  std::memcpy(wr(m.proj_b), get("encoder_projector.bias"), D * sizeof(float));
  std::memcpy(wr(m.emb), get("decoder.embedding.weight"), V * D * sizeof(float));
  for (int l = 0; l < cfg.decoder_layers; ++l) {
    const std::string n = std::to_string(l);
    const float *ih = get("decoder.lstm.weight_ih_l" + n), *hh = get("decoder.lstm.weight_hh_l" + n), *bi = get("decoder.lstm.bias_ih_l" + n),
                *bh = get("decoder.lstm.bias_hh_l" + n);
    for (size_t q = 0; q < 4; ++q)
      for (size_t j = 0; j < D; ++j) {
        const size_t row = q * D + j, col = 4 * j + q;      // torch stacks the gates i, f, g, o along the rows
        for (size_t k = 0; k < D; ++k) {
          wr(m.lstm_w[l])[k * 4 * D + col] = ih[row * D + k];
          wr(m.lstm_w[l])[(D + k) * 4 * D + col] = hh[row * D + k];
        }
        wr(m.lstm_b[l])[col] = bi[row] + bh[row];
      }
  }
  transposed(get("decoder.decoder_projector.weight"), D, D, m.dp_w, D);
  std::memcpy(wr(m.dp_b), get("decoder.decoder_projector.bias"), D * sizeof(float));
  transposed(get("joint.head.weight"), W, D, m.head_w, P);
  std::memcpy(wr(m.head_b), get("joint.head.bias"), W * sizeof(float));
  HIP_TRY(hipSetDevice(h->device));
  crispy::DevBuf<float> fresh;
  HIP_TRY(fresh.alloc(total * sizeof(float)));
  HIP_TRY(hipMemcpy(fresh.p, blob.data(), total * sizeof(float), hipMemcpyHostToDevice));
  h->weights = std::move(fresh);      // the copy of an earlier load goes with `fresh`
  h->cfg = cfg;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_tdt_load")

int crispy_pk_tdt_loaded(void* hv) try {
  const crispy_pk_tdt* h = static_cast<const crispy_pk_tdt*>(hv);
  return h && h->weights.p ? 1 : 0;
}
CRISPY_CATCH_RET("crispy_pk_tdt_loaded")

int crispy_pk_tdt_config_of(void* hv, void* cfg) try {
  const char* who = "crispy_pk_tdt_config_of";
  const crispy_pk_tdt* h = static_cast<const crispy_pk_tdt*>(hv);
  if (!h || !cfg) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle or cfg", who);
  if (!h->weights.p) return fail(CRISPY_ERR_INVALID_ARG, "%s: no decoder is loaded (crispy_pk_tdt_load comes first)", who);
  *static_cast<crispy_pk_tdt_config*>(cfg) = h->cfg;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_tdt_config_of")

int crispy_pk_tdt_decode_device(void* hv, const float* d_frames, const long* frame_offset, int n_clips, int* d_steps, int* d_n_steps,
                                float* d_proj_tap, float* d_logits_tap, void* hip_stream) try {
  const char* who = "crispy_pk_tdt_decode_device";
  crispy_pk_tdt* h = static_cast<crispy_pk_tdt*>(hv);
  const int rc = check_call(who, h, frame_offset, n_clips);
  if (rc != CRISPY_OK) return rc;
  if (!d_n_steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_n_steps is NULL", who);
  if (frame_offset[n_clips] > 0 && !d_frames) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_frames is NULL", who);
  if (total_budget(h->cfg, frame_offset, n_clips) > 0 && !d_steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_steps is NULL", who);
  HIP_TRY(hipSetDevice(h->device));
  return tdt_run(h, d_frames, frame_offset, n_clips, d_steps, d_n_steps, d_proj_tap, d_logits_tap, hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_pk_tdt_decode_device")

int crispy_pk_tdt_decode(void* hv, const float* frames, const long* frame_offset, int n_clips, int* steps, int* n_steps, float* proj_tap,
                         float* logits_tap) try {
  const char* who = "crispy_pk_tdt_decode";
  crispy_pk_tdt* h = static_cast<crispy_pk_tdt*>(hv);
  const int rc0 = check_call(who, h, frame_offset, n_clips);
  if (rc0 != CRISPY_OK) return rc0;
  if (!n_steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_steps is NULL", who);
  const size_t T = (size_t)frame_offset[n_clips], B = (size_t)total_budget(h->cfg, frame_offset, n_clips);
  if (T > 0 && !frames) return fail(CRISPY_ERR_INVALID_ARG, "%s: frames is NULL", who);
  if (B > 0 && !steps) return fail(CRISPY_ERR_INVALID_ARG, "%s: steps is NULL", who);
  const size_t H = (size_t)h->cfg.hidden, D = (size_t)h->cfg.decoder_hidden, W = (size_t)h->cfg.vocab + (size_t)h->cfg.n_durations;
  auto round = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t frames_b = round(T * H * sizeof(float)), steps_b = round(B * 3 * sizeof(int)), n_b = round((size_t)n_clips * sizeof(int)),
               proj_b = proj_tap ? round(T * D * sizeof(float)) : 0, tap_b = logits_tap ? round(B * W * sizeof(float)) : 0;
  const size_t need = frames_b + steps_b + n_b + proj_b + tap_b;
  HIP_TRY(hipSetDevice(h->device));
  if (need > h->io.bytes) {      // the logits tap is what makes this large: refused before anything is enqueued
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b + h->io.bytes)
      return fail(CRISPY_ERR_OOM, "%s: the call's buffers need %zu bytes, the device has %zu free", who, need, free_b + h->io.bytes);
    HIP_TRY(h->io.grow(need));
  }
  char* at = h->io.p;
  float* d_frames = reinterpret_cast<float*>(at); at += frames_b;
  int* d_steps = reinterpret_cast<int*>(at); at += steps_b;
  int* d_n = reinterpret_cast<int*>(at); at += n_b;
  float* d_proj = nullptr; if (proj_tap) { d_proj = reinterpret_cast<float*>(at); at += proj_b; }
  float* d_tap = logits_tap ? reinterpret_cast<float*>(at) : nullptr;
  if (T > 0) HIP_TRY(hipMemcpyAsync(d_frames, frames, T * H * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if (B > 0) HIP_TRY(hipMemsetAsync(d_steps, 0, B * 3 * sizeof(int), h->stream));      // rows behind a clip's n_steps read as zeros
  if (d_tap && B > 0) HIP_TRY(hipMemsetAsync(d_tap, 0, B * W * sizeof(float), h->stream));
  const int rc = tdt_run(h, d_frames, frame_offset, n_clips, d_steps, d_n, d_proj, d_tap, h->stream);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(n_steps, d_n, (size_t)n_clips * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (B > 0) HIP_TRY(hipMemcpyAsync(steps, d_steps, B * 3 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (proj_tap && T > 0) HIP_TRY(hipMemcpyAsync(proj_tap, d_proj, T * D * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (logits_tap && B > 0) HIP_TRY(hipMemcpyAsync(logits_tap, d_tap, B * W * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_tdt_decode")

long crispy_pk_tdt_words(const int* steps, int n_steps, int frames, int blank, const char* const* pieces, int vocab, double seconds_per_frame,
                         float* start_s, float* end_s, long* text_off, int max_words, char* text, long text_cap, long* text_needed) try {
  const char* who = "crispy_pk_tdt_words";
  if (n_steps < 0 || (n_steps > 0 && !steps)) return fail(CRISPY_ERR_INVALID_ARG, "%s: steps is NULL or n_steps %d is negative", who, n_steps);
  if (!pieces || vocab < 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: pieces is NULL or vocab %d is below 1", who, vocab);
  if (frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: frames %d is negative", who, frames);
  if (!(seconds_per_frame > 0.0) || !std::isfinite(seconds_per_frame)) return fail(CRISPY_ERR_INVALID_ARG, "%s: seconds_per_frame is not a positive number", who);
  if (max_words < 0 || text_cap < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: max_words %d or text_cap %ld is negative", who, max_words, text_cap);
  struct Word {
    int start, end;
    std::string text;
  };
  std::vector<Word> words;
  for (int i = 0; i < n_steps; ++i) {
    const int k = steps[3 * i], t = steps[3 * i + 1], d = steps[3 * i + 2];
    if (k == blank) continue;
    if (k < 0 || k >= vocab) return fail(CRISPY_ERR_INVALID_ARG, "%s: step %d has token %d, outside 0 ... %d", who, i, k, vocab - 1);
    if (t < 0 || d < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: step %d has frame %d and duration %d", who, i, t, d);
    const char* piece = pieces[k];
    if (!piece) return fail(CRISPY_ERR_INVALID_ARG, "%s: pieces[%d] is NULL", who, k);
    const bool fresh = has_marker(piece);
    if (fresh) piece += 3;
    const int end = (int)std::min<long>((long)t + d, frames);
    if (fresh || words.empty()) {
      words.push_back({t, end, piece});
    } else {
      words.back().end = end;
      words.back().text += piece;
    }
  }
  long need = 0;
  for (const Word& w : words) need += (long)w.text.size() + 1;
  if (text_needed) *text_needed = need;
  const long n = (long)words.size();
  if (n > max_words || need > text_cap || (n > 0 && (!start_s || !end_s || !text_off || !text))) return n;      // sizes only: nothing is written
  long at = 0;
  for (long i = 0; i < n; ++i) {
    start_s[i] = (float)((double)words[(size_t)i].start * seconds_per_frame);
    end_s[i] = (float)((double)words[(size_t)i].end * seconds_per_frame);
    text_off[i] = at;
    std::memcpy(text + at, words[(size_t)i].text.c_str(), words[(size_t)i].text.size() + 1);
    at += (long)words[(size_t)i].text.size() + 1;
  }
  return n;
}
CRISPY_CATCH_RET("crispy_pk_tdt_words")

}  // extern "C"

// rn_legacy_io.cpp -- the host side of NsState's Legacy arm and of the model switch, for every stream of a handle at once:
//   crispy_rn_model_configure   set_monitoring_model (src-tauri/src/audio.rs:942-967): a fresh processor of the named kind
//   crispy_rn_model             which variant of NsState the handle is
//   crispy_ns_noise_state       SharedAudio's LCG and its noise values, pure
//   (push / pull)               SharedAudio::push_sample / next_sample (audio.rs:151-199) and, behind the push, the rest of
//                               push_mono_to_buffers (audio.rs:701-726): what crispy_rn_push*, crispy_rn_pull* and
//                               crispy_rn_capture* run on a Legacy handle, reached through RnLegacy's pointers (rn_handle.h)
// The kernels are rn_legacy.hip, and for the recording side rn_capture_resample_kernel and the ring append, driven through
// the launchers of rn_common.h.  Rates and volume are the adapter's, the deque is the playback ring (raw samples at the raw
// rate), the callback's recording resampler is RnCaptureState's; the model kind and the LCG state are RnLegacy's.  All of it
// lives on the host: the streams of a handle are pushed and pulled in lock step.
// Every entry point allocates before it changes anything: a failure returns with the handle's state as it was.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "api_util.h"
#include "rn_common.h"
#include "rn_handle.h"

using namespace crispy;

namespace {

constexpr long kLegacyMaxIn = 1L << 24;      // samples per stream and push, as in the RNNoise arm

// SharedAudio::push_sample over the n_in samples of every stream, then push_mono_to_buffers' resampler and ring.
int legacy_push_impl(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_out, long out_stride, long* n_out, hipStream_t s,
                     const char* who) {
  RnLegacy* lg = h->lg.get();
  const RnAdapter* a = adapter_of(h);
  const long B = h->B;
  if (n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in < 0", who);
  if (n_in > kLegacyMaxIn) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in %ld above the limit of %ld samples per push", who, n_in, kLegacyMaxIn);
  if (in_stride < n_in) return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than n_in %ld", who, in_stride, n_in);
  if (out_stride < n_in) return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld samples of this push", who, out_stride, n_in);
  {
    const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)((B - 1) * in_stride + n_in) * sizeof(float);
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)((B - 1) * out_stride + n_in) * sizeof(float);
    if (i0 < o1 && o0 < i1) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_out overlaps d_in", who);
  }
  // The callback's resampler (audio.rs:701-714): reconfigured -- and so reset -- when what the processor produces is 1 Hz or
  // more off its input rate; it runs on every sample returned, whether or not the handle records.
  RnCaptureState* c = h->cap.get();      // (crispy_rn_model_configure made it)
  const float produced = a->rate;        // NsState::produced_rate_hz: s.input_rate, the raw rate
  const bool reset = std::fabs(lg->rec_rate - produced) >= 1.f;
  const float rec_rate = reset ? produced : lg->rec_rate;
  const bool rec_resample = std::fabs(rec_rate - 48000.f) >= 1.f;
  const bool rec = recording(h);
  LinResState rs = reset ? LinResState() : c->rs;
  long n_rec = n_in;
  if (rec_resample) {
    if (rec) { c->idx.clear(); c->t.clear(); }
    n_rec = linres_advance(rs, (double)(rec_rate / 48000.f), n_in, kPushMaxNew, rec ? &c->idx : nullptr, rec ? &c->t : nullptr);
    if (n_rec < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: more than %ld resampled samples per push", who, kPushMaxNew);
  }
  // every allocation first: a failure from here on returns with the handle's state as it was
  const bool upload = rec && rec_resample && n_rec > 0;
  const long rec_stride = (n_rec + 3) & ~3L;       // rows stay 16-byte aligned
  if (upload) {
    const size_t bytes = (size_t)B * rec_stride * sizeof(float);
    if (lg->rec.grow(bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: recording workspace allocation of %zu bytes failed", who, bytes);
    }
    const int rc = c->pos.reserve((size_t)2 * n_rec, who);
    if (rc != CRISPY_OK) return rc;
  }

  // ---- enqueue ----
  const bool noisy = lg->model == CRISPY_NS_NOISY;
  RnPlayback* pb = h->pb.get();
  RnLegacyPush lp{};
  lp.in = d_in;
  lp.in_stride = in_stride;
  lp.n = (int)n_in;
  lp.out = d_out;
  lp.out_stride = out_stride;
  lp.volume = a->volume;
  lp.rng = lg->rng;
  lp.B = h->B;
  AppendPlan ap;
  if (pb) {      // `buffer`: the raw sample, with the deque's eviction (audio.rs:152-155)
    ap = plan_append(pb->buf, pb->cap, n_in);
    lp.ring = pb->ring.p;
    lp.cap = pb->cap;
    lp.tail = ap.tail;
    lp.skip = (int)ap.skip;
  }
  HIP_TRY(rn_launch_legacy_push(lp, noisy, s));
  int cur_next = c->cur;
  if (rec_resample) {
    RnCaptureResample cr{};
    cr.mono = d_out;
    cr.mono_stride = out_stride;
    cr.n_in = (int)n_in;
    if (upload) {
      const int rc = c->pos.send((size_t)2 * n_rec, s, [&](int* slot) {
        std::memcpy(slot, c->idx.data(), (size_t)n_rec * sizeof(int));
        std::memcpy(slot + n_rec, c->t.data(), (size_t)n_rec * sizeof(float));
      });
      if (rc != CRISPY_OK) return rc;
      cr.idx = c->pos.dev.p;
      cr.t = reinterpret_cast<const float*>(c->pos.dev.p + n_rec);
      cr.out = lg->rec.p;
      cr.out_stride = rec_stride;
      cr.n_out = n_rec;
    }      // else: nothing is emitted, or nobody records it -- the launch only keeps last_sample
    const int cur = c->cur, nxt = cur ^ 1;
    cr.last_old = c->last.p + (size_t)cur * B;
    cr.last_new = c->last.p + (size_t)nxt * B;
    cr.B = h->B;
    HIP_TRY(rn_launch_capture_resample(cr, s));
    cur_next = nxt;
  }
  if (rec && n_rec > 0) {      // audio.rs:716-725 (the append moves the mic ring's position itself, once it is enqueued)
    const int rc = rec_resample ? ring_append(h->rec->mic_ring.p, h->rec->mic, h->rec->cap, lg->rec.p, rec_stride, n_rec, h->B, s)
                                : ring_append(h->rec->mic_ring.p, h->rec->mic, h->rec->cap, d_out, out_stride, n_in, h->B, s);
    if (rc != CRISPY_OK) return rc;
  }
  // everything is enqueued: the host's state moves in one piece, so an enqueue that failed above left all of it as it was
  if (pb) pb->buf = ap.after;
  if (noisy) lg->rng = ns_lcg_jump(lg->rng, (uint32_t)n_in);
  lg->rec_rate = rec_rate;
  c->rs = rs;
  c->cur = cur_next;
  *n_out = n_in;
  return CRISPY_OK;
}

// SharedAudio::next_sample, n_frames times.  Arguments checked (rn_io.cpp: check_pull), n_frames > 0, the handle's device current.
int legacy_pull_impl(crispy_rn* h, long n_frames, int channels, int format, void* d_out, long out_stride, long* n_live, hipStream_t s,
                     const char* who) {
  RnLegacy* lg = h->lg.get();
  RnPlayback* p = h->pb.get();
  const PullPlan pl = plan_pull(p, n_frames);      // step = input_rate as f64 / output_rate as f64 with the raw rate
  // every allocation first: a failure from here on returns with the handle's state as it was
  const size_t words = (size_t)2 * n_frames;
  int rc = p->frames.reserve(words, who);
  if (rc != CRISPY_OK) return rc;

  // ---- enqueue ----
  rc = p->frames.send(words, s, [&](int* slot) {
    std::memcpy(slot, p->off.data(), (size_t)n_frames * sizeof(int));
    std::memcpy(slot + n_frames, p->frac.data(), (size_t)n_frames * sizeof(float));
  });
  if (rc != CRISPY_OK) return rc;
  const bool noisy = lg->model == CRISPY_NS_NOISY;
  RnLegacyPull a{};
  a.p.ring = p->ring.p;
  a.p.cap = p->cap;
  a.p.head = p->buf.head;
  a.p.off = p->frames.dev.p;
  a.p.frac = reinterpret_cast<const float*>(p->frames.dev.p + n_frames);
  a.p.out = d_out;
  a.p.out_stride = out_stride;
  a.p.n_frames = (unsigned)n_frames;
  a.p.n_elems = (unsigned)(n_frames * channels);
  a.p.channels = (unsigned)channels;
  a.p.B = h->B;
  a.volume = adapter_of(static_cast<const crispy_rn*>(h))->volume;
  a.rng = lg->rng;
  HIP_TRY(rn_launch_legacy_pull(a, format, noisy, s));
  p->buf.head = (int)((p->buf.head + pl.pops) % p->cap);
  p->buf.len = (int)pl.len;
  p->pos = pl.pos;
  if (noisy) lg->rng = ns_lcg_jump(lg->rng, (uint32_t)pl.live);      // a dry frame advances nothing
  if (n_live) *n_live = pl.live;
  return CRISPY_OK;
}

}  // namespace

extern "C" {

int crispy_rn_model_configure(crispy_rn* h, int model) try {
  const char* who = "crispy_rn_model_configure";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (model != CRISPY_NS_RNNOISE && model != CRISPY_NS_DUMMY && model != CRISPY_NS_NOISY)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown model %d", who, model);
  HIP_TRY(hipSetDevice(h->device));
  const float rate = adapter_of(static_cast<const crispy_rn*>(h))->rate, volume = adapter_of(static_cast<const crispy_rn*>(h))->volume;
  const bool made = !h->lg;
  if (made) {
    // (std::bad_alloc: the guard makes it CRISPY_ERR_OOM.)  crispy_rn_adapter_configure below reads the model from the handle,
    // so the object is installed here and taken off again if the call fails.
    h->lg.reset(new RnLegacy());
    h->lg->rec_rate = rate;        // LinearResampler::new(input_rate, 48000) of the capture stream (audio.rs:746)
    h->lg->push = legacy_push_impl;
    h->lg->pull = legacy_pull_impl;
  }
  if (model != CRISPY_NS_RNNOISE) {
    const int rc = ensure_capture_last(h, who);
    if (rc != CRISPY_OK) {
      if (made) h->lg.reset();
      return rc;
    }
  }
  // The fresh processor at the remembered rate and the current volume (audio.rs:949-965): crispy_rn_adapter_configure makes
  // the one of the handle's model -- RnnNoiseProcessor::new as ever, or SharedAudio::new: the ring emptied and sized from the
  // raw rate, resample_pos = 0, rng_state = 0x1234abcd.  It allocates before it changes anything.
  const int old = h->lg->model;
  h->lg->model = model;
  const int rc = crispy_rn_adapter_configure(h, rate, volume);
  if (rc != CRISPY_OK) {
    h->lg->model = old;
    if (made) h->lg.reset();
  }
  return rc;
} CRISPY_CATCH_RET("crispy_rn_model_configure")

int crispy_rn_model(const crispy_rn* h, int* model) try {
  if (!h || !model) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_model: NULL argument");
  *model = h->lg ? h->lg->model : CRISPY_NS_RNNOISE;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_model")

long crispy_ns_noise_state(long state, long n, float* noise) try {
  if (state < 0 || state > 0xffffffffL) return fail(CRISPY_ERR_INVALID_ARG, "crispy_ns_noise_state: state outside 0...2^32 - 1");
  if (n < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_ns_noise_state: n < 0");
  uint32_t s = (uint32_t)state;
  if (!noise) return (long)ns_lcg_jump(s, (uint32_t)n);      // the period is 2^32: n counts modulo it
  for (long k = 0; k < n; ++k) {
    s = ns_lcg_step(s);
    noise[k] = ns_noise(s);
  }
  return (long)s;
} CRISPY_CATCH_RET("crispy_ns_noise_state")

}  // extern "C"

// rn_capture_io.cpp -- the host side of the capture callbacks in front of push_sample, for every stream of a handle at once:
//   crispy_rn_capture*               build_input_stream_f32 / _i16 / _u16 and push_mono_to_buffers (src-tauri/src/audio.rs:682-921):
//                                    the device's frames to mono, the level meter, then the handle's arm -- the RNNoise arm is
//                                    crispy_rn_push_device on the mono, the bypass arm the callback's own LinearResampler
//   crispy_rn_bypass_configure       the `shared == None` arm (audio.rs:545, 697-699): noise suppression off, recording on
//   crispy_rn_record_app_push_at*    the app-audio handler of a stream at its own rate: resample_audio (recording.rs:13-39)
// The kernels are rn_capture.hip (and rn_level_kernel, the ring append), driven through the launchers of rn_common.h; the
// state is RnCaptureState (rn_handle.h); the push, the ring plans and the resampler recurrence are rn_io.cpp's.
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

constexpr long kCaptureMaxFrames = 1L << 24;    // frames per stream and capture: the push's and the level meter's limit
constexpr long kAppAtMaxOut = 1L << 24;         // 48 kHz samples per stream and app push: an output index is exact in f64 and f32
constexpr int kAppRateMin = 8000, kAppRateMax = 384000;

inline size_t pcm_bytes(int format) { return format == CRISPY_PCM_F32 ? 4 : 2; }

RnCaptureState* capture_of(crispy_rn* h) {
  if (!h->cap) h->cap.reset(new RnCaptureState());      // (std::bad_alloc: the entry point's guard makes it CRISPY_ERR_OOM)
  return h->cap.get();
}
inline bool bypassed(const crispy_rn* h) { return h->cap && h->cap->bypass_rate > 0.f; }

// What a capture of n_frames will return, worked out on the host without touching the handle.
struct CapturePlan {
  bool bypass = false;
  LinResState rs;      // the bypass resampler's state behind the capture
  long n_out = 0;      // samples per stream that go to d_out
};

// idx / t: where a bypassed capture records its positions; null: count only.
int plan_capture(const crispy_rn* h, long n_frames, std::vector<int>* idx, std::vector<float>* t, CapturePlan* p, const char* who) {
  if (n_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames < 0", who);
  if (n_frames > kCaptureMaxFrames)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames %ld above the limit of %ld frames per capture", who, n_frames, kCaptureMaxFrames);
  p->bypass = bypassed(h);
  if (!p->bypass) {
    PushPlan pp;
    const int rc = plan_push(adapter_of(h), n_frames, nullptr, nullptr, &pp, who);
    if (rc != CRISPY_OK) return rc;
    p->n_out = legacy_active(h) ? n_frames : pp.n_out;      // NsState::Legacy: one sample out per sample in
    return CRISPY_OK;
  }
  const RnCaptureState* c = h->cap.get();
  p->rs = c->rs;
  if (c->resample) {
    if (idx) { idx->clear(); t->clear(); }
    const double step = (double)(c->bypass_rate / 48000.f);
    p->n_out = linres_advance(p->rs, step, n_frames, kPushMaxNew, idx, t);
    if (p->n_out < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: more than %ld resampled samples per capture", who, kPushMaxNew);
  } else {
    p->n_out = n_frames;
  }
  return CRISPY_OK;
}

// The arguments every capture checks, before anything is touched; n_frames > 0.
int check_capture(const void* in, long in_stride, long n_frames, int channels, int format, const void* out, const char* who) {
  if (channels < 1 || channels > 8) return fail(CRISPY_ERR_INVALID_ARG, "%s: channels %d outside 1...8", who, channels);
  if (format != CRISPY_PCM_F32 && format != CRISPY_PCM_I16 && format != CRISPY_PCM_U16)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown format %d", who, format);
  if (!in || !out) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL audio pointer", who);
  if (in_stride < n_frames * channels)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than the %ld elements of this capture", who, in_stride, n_frames * channels);
  return CRISPY_OK;
}

inline bool rows_overlap(const float* a, long a_stride, long a_n, const float* b, long b_stride, long b_n, long B) {
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (size_t)((B - 1) * a_stride + a_n) * sizeof(float);
  const uintptr_t b0 = (uintptr_t)b, b1 = b0 + (size_t)((B - 1) * b_stride + b_n) * sizeof(float);
  return a0 == b0 || (a_n > 0 && b_n > 0 && a0 < b1 && b0 < a1);
}

// Arguments checked (check_capture), n_frames > 0, the handle's device current.
int capture_device_impl(crispy_rn* h, const void* d_in, long in_stride, long n_frames, int channels, int format, float* d_out,
                        long out_stride, float* d_mono, long mono_stride, float* d_rms, long* n_out, hipStream_t s, const char* who) {
  RnCaptureState* c = capture_of(h);
  CapturePlan p;
  int rc = plan_capture(h, n_frames, &c->idx, &c->t, &p, who);
  if (rc != CRISPY_OK) return rc;
  const long B = h->B;
  if (out_stride < p.n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld samples of this capture", who, out_stride, p.n_out);
  if (d_mono && mono_stride < n_frames)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: mono_stride %ld shorter than n_frames %ld", who, mono_stride, n_frames);
  if (d_mono && rows_overlap(d_mono, mono_stride, n_frames, d_out, out_stride, p.n_out, B))
    return fail(CRISPY_ERR_INVALID_ARG, "%s: d_out overlaps d_mono", who);
  // every allocation of this file's own first; the push makes its own before it changes anything
  if (!d_mono) {
    mono_stride = (n_frames + 3) & ~3L;        // rows stay 16-byte aligned
    const size_t bytes = (size_t)B * mono_stride * sizeof(float);
    if (c->mono.grow(bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: mono workspace allocation of %zu bytes failed", who, bytes);
    }
    d_mono = c->mono.p;
  }
  const bool upload = p.bypass && c->resample && p.n_out > 0;
  if (upload) {
    rc = c->pos.reserve((size_t)2 * p.n_out, who);
    if (rc != CRISPY_OK) return rc;
  }

  // ---- enqueue ----
  RnCapture ca{};
  ca.in = d_in;
  ca.in_stride = in_stride;
  ca.n = (int)n_frames;
  ca.channels = channels;
  ca.mono = d_mono;
  ca.mono_stride = mono_stride;
  ca.B = h->B;
  HIP_TRY(rn_launch_capture(ca, format, s));
  if (d_rms) {
    rc = level_device_impl(h, d_mono, mono_stride, n_frames, d_rms, s);
    if (rc != CRISPY_OK) return rc;
  }
  if (!p.bypass) {    // Some(shared): push_sample on every mono sample, its output to the playback and recording rings
    // (every argument the Legacy push checks -- the sample count, both strides against it, d_out against the mono rows -- was
    // checked above with p.n_out = n_frames, before anything was launched)
    if (legacy_active(h)) return h->lg->push(h, d_mono, mono_stride, n_frames, d_out, out_stride, n_out, s, who);
    return push_device_impl(h, d_mono, mono_stride, n_frames, d_out, out_stride, nullptr, 0, nullptr, n_out, s, who);
  }

  // shared == None: the callback's resampler on the raw mono (audio.rs:697-714)
  RnCaptureResample cr{};
  cr.mono = d_mono;
  cr.mono_stride = mono_stride;
  cr.n_in = (int)n_frames;
  if (upload) {
    rc = c->pos.send((size_t)2 * p.n_out, s, [&](int* slot) {
      std::memcpy(slot, c->idx.data(), (size_t)p.n_out * sizeof(int));
      std::memcpy(slot + p.n_out, c->t.data(), (size_t)p.n_out * sizeof(float));
    });
    if (rc != CRISPY_OK) return rc;
    cr.idx = c->pos.dev.p;
    cr.t = reinterpret_cast<const float*>(c->pos.dev.p + p.n_out);
  }
  const int cur = c->cur, nxt = cur ^ 1;
  cr.last_old = c->last.p + (size_t)cur * B;
  cr.last_new = c->last.p + (size_t)nxt * B;
  cr.out = d_out;
  cr.out_stride = out_stride;
  cr.n_out = p.n_out;
  cr.B = h->B;
  HIP_TRY(rn_launch_capture_resample(cr, s));
  c->rs = p.rs;
  c->cur = nxt;
  if (p.n_out > 0 && recording(h)) {      // audio.rs:716-725
    rc = ring_append(h->rec->mic_ring.p, h->rec->mic, h->rec->cap, d_out, out_stride, p.n_out, h->B, s);
    if (rc != CRISPY_OK) return rc;
  }
  *n_out = p.n_out;
  return CRISPY_OK;
}

// The outputs resample_audio makes of n samples at from_rate (recording.rs:18-36), with its own f64 expressions: output_len
// positions, of which those whose src_index is not below n are not emitted.
long resample_audio_count(long n, double ratio) {
  long count = (long)std::ceil((double)n / ratio);
  while (count > 0 && (long)std::floor((double)(count - 1) * ratio) >= n) --count;
  return count;
}

int check_app_rate(int from_rate, const char* who) {
  if (from_rate < kAppRateMin || from_rate > kAppRateMax)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: from_rate %d outside %d...%d", who, from_rate, kAppRateMin, kAppRateMax);
  return CRISPY_OK;
}

// Arguments checked (check_app_push, check_app_rate), n_frames > 0, the handle's device current.
int app_push_at_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, int from_rate, hipStream_t s,
                            const char* who) {
  if (from_rate == 48000) return app_push_device_impl(h, d_in, in_stride, n_frames, channels, s);      // `samples.to_vec()`
  RnRecord* r = h->rec.get();
  const double ratio = (double)from_rate / (double)48000;
  const long count = resample_audio_count(n_frames, ratio);
  if (count > kAppAtMaxOut)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: %ld resampled samples, above the limit of %ld per push", who, count, kAppAtMaxOut);
  const AppendPlan p = plan_append(r->app, r->cap, count);
  RnRecAppAt a{};
  a.in = d_in;
  a.in_stride = in_stride;
  a.n_in = (int)n_frames;
  a.channels = channels;
  a.ratio = ratio;
  a.skip = p.skip;
  a.ring = r->app_ring.p;
  a.cap = r->cap;
  a.tail = p.tail;
  a.n = p.n;
  a.B = h->B;
  HIP_TRY(rn_launch_rec_app_at(a, s));
  r->app = p.after;
  return CRISPY_OK;
}

}  // namespace

int crispy::ensure_capture_last(crispy_rn* h, const char* who) {
  RnCaptureState* c = capture_of(h);
  if (c->last.p) return CRISPY_OK;
  const size_t bytes = 2 * (size_t)h->B * sizeof(float);
  DevBuf<float> last;
  if (last.alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: resampler state allocation of %zu bytes failed", who, bytes);
  }
  HIP_TRY(hipMemset(last.p, 0, bytes));
  HIP_TRY(hipDeviceSynchronize());
  c->last = std::move(last);
  return CRISPY_OK;
}

extern "C" {

int crispy_rn_bypass_configure(crispy_rn* h, float raw_input_rate) try {
  const char* who = "crispy_rn_bypass_configure";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!(raw_input_rate >= 0.f) || !std::isfinite(raw_input_rate))
    return fail(CRISPY_ERR_INVALID_ARG, "%s: raw_input_rate must be a positive number of Hz, or 0 to leave the arm", who);
  HIP_TRY(hipSetDevice(h->device));
  RnCaptureState* c = capture_of(h);
  if (raw_input_rate > 0.f) {
    const int rc = ensure_capture_last(h, who);
    if (rc != CRISPY_OK) return rc;
  }
  c->bypass_rate = raw_input_rate;
  c->resample = raw_input_rate > 0.f && std::fabs(raw_input_rate - 48000.f) >= 1.f;
  c->rs = LinResState();      // LinearResampler::new (audio.rs:746)
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_bypass_configure")

long crispy_rn_capture_out_len(const crispy_rn* h, long n_frames) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_capture_out_len: NULL handle");
  CapturePlan p;
  const int rc = plan_capture(h, n_frames, nullptr, nullptr, &p, "crispy_rn_capture_out_len");
  return rc != CRISPY_OK ? rc : p.n_out;
} CRISPY_CATCH_RET("crispy_rn_capture_out_len")

int crispy_rn_capture_device(crispy_rn* h, const void* d_in, long in_stride, long n_frames, int channels, int format, float* d_out,
                             long out_stride, float* d_mono, long mono_stride, float* d_rms, long* n_out, void* hip_stream) try {
  const char* who = "crispy_rn_capture_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_out is NULL", who);
  *n_out = 0;
  if (n_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames < 0", who);
  if (n_frames == 0) return CRISPY_OK;
  const int rc = check_capture(d_in, in_stride, n_frames, channels, format, d_out, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return capture_device_impl(h, d_in, in_stride, n_frames, channels, format, d_out, out_stride, d_mono, mono_stride, d_rms, n_out,
                             hip_stream ? (hipStream_t)hip_stream : h->stream, who);
} CRISPY_CATCH_RET("crispy_rn_capture_device")

int crispy_rn_capture(crispy_rn* h, const void* in, long in_stride, long n_frames, int channels, int format, float* out,
                      long out_stride, float* rms, long* n_out) try {
  const char* who = "crispy_rn_capture";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_out is NULL", who);
  *n_out = 0;
  if (n_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames < 0", who);
  if (n_frames == 0) return CRISPY_OK;
  int rc = check_capture(in, in_stride, n_frames, channels, format, out, who);
  if (rc != CRISPY_OK) return rc;
  CapturePlan p;
  rc = plan_capture(h, n_frames, nullptr, nullptr, &p, who);
  if (rc != CRISPY_OK) return rc;
  if (out_stride < p.n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld samples of this capture", who, out_stride, p.n_out);
  HIP_TRY(hipSetDevice(h->device));
  // the raw bytes as they are; rows on a 16-byte pitch, so that the kernel reads them with 16-byte loads where a frame allows
  const size_t B = (size_t)h->B, eb = pcm_bytes(format);
  const size_t row = (size_t)n_frames * channels * eb, pitch = (row + 15) & ~(size_t)15;
  rc = h->stage_reserve(B * pitch, B * (size_t)(p.n_out > 0 ? p.n_out : 1) * sizeof(float), rms ? B * sizeof(float) : 0, who);
  if (rc != CRISPY_OK) return rc;
  float* d_hout = reinterpret_cast<float*>(h->stage_out.p);
  float* d_hrms = rms ? h->stage_aux.p : nullptr;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(h->stage_in.p, pitch, in, (size_t)in_stride * eb, row, B, hipMemcpyHostToDevice, s));
  long got = 0;
  rc = capture_device_impl(h, h->stage_in.p, (long)(pitch / eb), n_frames, channels, format, d_hout, p.n_out, nullptr, 0, d_hrms, &got, s, who);
  if (rc != CRISPY_OK) return rc;
  if (got > 0)
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * sizeof(float), d_hout, (size_t)got * sizeof(float), (size_t)got * sizeof(float), B,
                             hipMemcpyDeviceToHost, s));
  if (rms) HIP_TRY(hipMemcpyAsync(rms, d_hrms, B * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_out = got;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_capture")

int crispy_rn_record_app_push_at_device(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, int from_rate,
                                        void* hip_stream) try {
  const char* who = "crispy_rn_record_app_push_at_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_app_rate(from_rate, who);
  if (rc != CRISPY_OK) return rc;
  rc = check_app_push(h, d_in, in_stride, n_frames, channels, who);
  if (rc != CRISPY_OK || n_frames == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return app_push_at_device_impl(h, d_in, in_stride, n_frames, channels, from_rate, hip_stream ? (hipStream_t)hip_stream : h->stream, who);
} CRISPY_CATCH_RET("crispy_rn_record_app_push_at_device")

int crispy_rn_record_app_push_at(crispy_rn* h, const float* in, long in_stride, long n_frames, int channels, int from_rate) try {
  const char* who = "crispy_rn_record_app_push_at";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_app_rate(from_rate, who);
  if (rc != CRISPY_OK) return rc;
  rc = check_app_push(h, in, in_stride, n_frames, channels, who);
  if (rc != CRISPY_OK || n_frames == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t row = (size_t)n_frames * channels;
  rc = h->stage_reserve((size_t)h->B * row * sizeof(float), 0, 0, who);
  if (rc != CRISPY_OK) return rc;
  float* d_hin = reinterpret_cast<float*>(h->stage_in.p);
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(d_hin, row * sizeof(float), in, (size_t)in_stride * sizeof(float), row * sizeof(float), (size_t)h->B,
                           hipMemcpyHostToDevice, s));
  rc = app_push_at_device_impl(h, d_hin, (long)row, n_frames, channels, from_rate, s, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_app_push_at")

}  // extern "C"

// rn_io.cpp -- the host side of the live path around the frame kernels, for every stream of a handle at once:
//   crispy_rn_push*      RnnNoiseProcessor::push_sample (src-tauri/src/audio.rs:242-295): capture-rate adapter in, frames,
//                        adapter out, and what it returns appended to the playback ring and to the recording ring
//   crispy_rn_pull*      the output callback's next_sample (audio.rs:297-314, 610-657)
//   crispy_rn_record_* / crispy_rn_level*   push_mono_to_buffers, the app-audio handlers, the recording worker
//                        (audio.rs:701-729, src-tauri/src/commands/recording.rs:196-264)
// The kernels are rn_adapter.hip, rn_playback.hip and rn_record.hip, driven through the launchers of rn_common.h; the state is
// rn_handle.h.  Resampler positions, ring heads and lengths, the worker's trims live here, on the host: the streams of a
// handle are pushed and pulled in lock step, so they are the same for all of them and do not depend on the samples.
// Every entry point allocates before it changes anything: a failure returns with the handle's state as it was
// (tests/asan/harness.cpp, rn-oom-sweep).
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

int PinnedUpload::reserve(size_t words, const char* who) {
  if (dev.grow(words * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: position table of %zu bytes failed", who, words * sizeof(int));
  }
  HIP_TRY(ev.ensure(2, hipEventDisableTiming));
  if (host_words[slot] < words) {
    int* fresh = nullptr;
    if (hipHostMalloc(&fresh, words * sizeof(int), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: pinned allocation of %zu bytes failed", who, words * sizeof(int));
    }
    Slot next(fresh, hipHostFree);
    HIP_TRY(hipEventSynchronize(ev[slot]));
    host[slot] = std::move(next);      // (the old slot is freed here)
    host_words[slot] = words;
  }
  return CRISPY_OK;
}

namespace {

constexpr long kPushMaxIn = 1L << 24;       // capture samples per stream and push
constexpr long kPullMaxFrames = 1L << 24;   // output frames per pull
constexpr long kLevelMaxIn = 1L << 24;      // samples per stream and call: the f32 count is exact
constexpr long REC_MAX_DESYNC = 2400;       // (SAMPLE_RATE / 20).max(frame_size): 50 ms at 48 kHz
constexpr long REC_DEFAULT_CAP = 48000L * 10;   // recording::SAMPLE_RATE * 10
constexpr long REC_MAX_CAP = 1L << 28;      // ring indices and the elements of a drained row stay inside 32 bits

inline size_t pcm_bytes(int format) { return format == CRISPY_PCM_F32 ? 4 : 2; }
inline long rec_elems_per_frame(int format) { return format == CRISPY_PCM_F32 ? REC_FRAME : 2L * REC_FRAME; }

}  // namespace

// What rn_capture_io.cpp uses as well is declared in rn_handle.h and defined in namespace crispy; the rest stays local.

// ---- rings ------------------------------------------------------------------------------------------------------------

namespace crispy {

AppendPlan plan_append(const RingPos& r, int cap, long n) {
  AppendPlan p;
  if (n >= cap) {                    // everything that was there is evicted, and the front of this block with it
    p.skip = n - cap;
    p.n = cap;
    p.tail = 0;
    p.after.head = 0;
    p.after.len = cap;
  } else {
    p.n = (int)n;
    p.tail = (int)(((long)r.head + r.len) % cap);
    const long over = (long)r.len + n - cap;
    if (over > 0) {
      p.after.head = (int)(((long)r.head + over) % cap);
      p.after.len = cap;
    } else {
      p.after.head = r.head;
      p.after.len = r.len + (int)n;
    }
  }
  return p;
}

int ring_append(float* ring, RingPos& pos, int cap, const float* d_rows, long stride, long n, int B, hipStream_t s) {
  const AppendPlan p = plan_append(pos, cap, n);
  RnRingAppend a{};
  a.src = d_rows + p.skip;
  a.src_stride = stride;
  a.ring = ring;
  a.cap = cap;
  a.tail = p.tail;
  a.n = p.n;
  a.B = B;
  HIP_TRY(rn_launch_ring_append(a, s));
  pos = p.after;
  return CRISPY_OK;
}

// ---- push -------------------------------------------------------------------------------------------------------------

// LinearResampler::process_sample's position arithmetic (audio.rs:108-133), the reference's own f64 recurrence run
// sample by sample -- from the first sample of a stream on, never a closed form, so it is the reference's sequence for
// the whole life of a stream, also past 2^29 outputs where the running sum starts to round.  The positions do not depend
// on the sample values: one run per push serves every stream of a handle.
// Feeds n_in samples; every output is (m, t): it interpolates samples m - 1 and m of these n_in (m == 0: the last sample
// before them) at t.  idx / t may be null (count only).  Stops and returns -1 once more than `limit` outputs were made.
long linres_advance(LinResState& st, double step, long n_in, long limit, std::vector<int>* idx, std::vector<float>* t) {
  long n = 0;
  for (long m = 0; m < n_in; ++m) {
    if (!st.has_last) {
      st.has_last = true;
      st.input_pos = 0.;
      st.next_pos = 0.;
      continue;
    }
    st.input_pos += 1.0;
    while (st.next_pos <= st.input_pos) {
      if (n >= limit) return -1;
      if (idx) {
        float f = (float)(st.next_pos - (st.input_pos - 1.0));
        f = f < 0.f ? 0.f : (f > 1.f ? 1.f : f);
        idx->push_back((int)m);
        t->push_back(f);
      }
      ++n;
      st.next_pos += step;
    }
  }
  return n;
}

}  // namespace crispy

namespace {

RnRecord* record_of(crispy_rn* h) {
  if (!h->rec) h->rec.reset(new RnRecord());      // (std::bad_alloc: the entry point's guard makes it CRISPY_ERR_OOM)
  return h->rec.get();
}

// The carry and last-sample halves are state: both new buffers exist before either is installed.
int ensure_adapter_state(crispy_rn* h, RnAdapter* a, const char* who) {
  if (a->carry.p && a->last.p) return CRISPY_OK;
  const size_t B = (size_t)h->B;
  DevBuf<float> carry, last;
  if (carry.alloc(2 * B * RN_FRAME * sizeof(float)) != hipSuccess || last.alloc(2 * B * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: adapter state allocation failed", who);
  }
  a->carry = std::move(carry);
  a->last = std::move(last);
  HIP_TRY(hipMemset(a->carry.p, 0, 2 * B * RN_FRAME * sizeof(float)));
  HIP_TRY(hipMemset(a->last.p, 0, 2 * B * sizeof(float)));
  HIP_TRY(hipDeviceSynchronize());
  return CRISPY_OK;
}

}  // namespace

namespace crispy {

RnAdapter* adapter_of(crispy_rn* h) {
  if (!h->ad) h->ad.reset(new RnAdapter());       // (std::bad_alloc: the entry point's guard makes it CRISPY_ERR_OOM)
  return h->ad.get();
}
const RnAdapter* adapter_of(const crispy_rn* h) {
  static const RnAdapter fresh;
  return h->ad ? h->ad.get() : &fresh;
}

int plan_push(const RnAdapter* a, long n_in, std::vector<int>* idx, std::vector<float>* t, PushPlan* p, const char* who) {
  if (n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in < 0", who);
  if (n_in > kPushMaxIn) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in %ld above the limit of %ld samples per push", who, n_in, kPushMaxIn);
  p->rs = a->rs;
  if (a->resample) {
    if (idx) { idx->clear(); t->clear(); }
    const double step = (double)(a->rate / 48000.f);
    p->n_new = linres_advance(p->rs, step, n_in, kPushMaxNew, idx, t);
    if (p->n_new < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: more than %ld resampled samples per push", who, kPushMaxNew);
  } else {
    p->n_new = n_in;
  }
  const long total = a->carry_len + p->n_new;
  p->frames = (int)(total / RN_FRAME);
  p->carry_len = (int)(total % RN_FRAME);
  p->n_out = (long)(p->frames - (a->first && p->frames > 0 ? 1 : 0)) * RN_FRAME;
  return CRISPY_OK;
}

int push_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_out, long out_stride, float* d_frames48,
                     long frames_stride, float* d_vad, long* n_out, hipStream_t s, const char* who) {
  RnAdapter* a = adapter_of(h);
  PushPlan p;
  int rc = plan_push(a, n_in, &a->idx, &a->t, &p, who);
  if (rc != CRISPY_OK) return rc;
  const long B = h->B;
  const long n_frame = (long)p.frames * RN_FRAME;
  if (in_stride < n_in) return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than n_in %ld", who, in_stride, n_in);
  if (out_stride < p.n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld samples of this push", who, out_stride, p.n_out);
  if (d_frames48 && frames_stride < n_frame)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: frames_stride %ld shorter than the %ld frame samples of this push", who, frames_stride, n_frame);
  {
    const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)((B - 1) * in_stride + n_in) * sizeof(float);
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)((B - 1) * out_stride + p.n_out) * sizeof(float);
    if (i0 == o0 || (p.n_out > 0 && i0 < o1 && o0 < i1)) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_out overlaps d_in", who);
  }
  // every allocation first: a failure from here on returns with the handle's state as it was
  rc = ensure_adapter_state(h, a, who);
  if (rc != CRISPY_OK) return rc;
  const size_t ws_bytes = (size_t)B * n_frame * sizeof(float);
  if (a->stage.grow(ws_bytes) != hipSuccess || a->y.grow(ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: workspace allocation of 2 x %zu bytes failed", who, ws_bytes);
  }
  const bool upload = a->resample && p.n_new > 0;
  if (upload) {
    rc = a->pos.reserve((size_t)2 * p.n_new, who);
    if (rc != CRISPY_OK) return rc;
  }
  if (h->timing) HIP_TRY(a->ev.ensure(4, 0));

  // ---- enqueue ----
  RnAdaptIn ai{};
  ai.in = d_in;
  ai.in_stride = in_stride;
  ai.n_in = n_in;
  if (upload) {
    rc = a->pos.send((size_t)2 * p.n_new, s, [&](int* slot) {
      std::memcpy(slot, a->idx.data(), (size_t)p.n_new * sizeof(int));
      std::memcpy(slot + p.n_new, a->t.data(), (size_t)p.n_new * sizeof(float));
    });
    if (rc != CRISPY_OK) return rc;
    ai.idx = a->pos.dev.p;     // (null when the push adds no 48 kHz sample, e.g. the one that primes the resampler)
    ai.t = reinterpret_cast<const float*>(a->pos.dev.p + p.n_new);
  }
  const int cur = a->cur, nxt = cur ^ 1;
  ai.carry_len = a->carry_len;
  ai.n_new = p.n_new;
  ai.frames = p.frames;
  ai.carry_old = a->carry.p + (size_t)cur * B * RN_FRAME;
  ai.carry_new = a->carry.p + (size_t)nxt * B * RN_FRAME;
  ai.last_old = a->last.p + (size_t)cur * B;
  ai.last_new = a->last.p + (size_t)nxt * B;
  ai.stage = a->stage.p;
  ai.frames48 = d_frames48;
  ai.frames_stride = frames_stride;
  ai.B = h->B;
  const bool timed = h->timing;
  if (timed) HIP_TRY(hipEventRecord(a->ev[0], s));
  HIP_TRY(rn_launch_adapt_in(ai, s));
  if (timed) HIP_TRY(hipEventRecord(a->ev[1], s));
  // the adapter's own state is committed here: what follows is the frames' business
  a->rs = p.rs;
  a->carry_len = p.carry_len;
  a->cur = nxt;
  const long skip = a->first && p.frames > 0 ? RN_FRAME : 0;
  if (p.frames > 0) a->first = false;
  a->timed = false;
  if (p.frames > 0) {
    // one call of that many frames, stream-major (BTF): frame stride 480, stream stride frames x 480
    rc = rn_process_frames_device(h, a->stage.p, a->y.p, d_vad, p.frames, (long)RN_FRAME, n_frame, s);
    if (rc != CRISPY_OK) return rc;
  }
  if (p.n_out > 0) {
    RnAdaptOut ao{};
    ao.y = a->y.p;
    ao.y_stride = n_frame;
    ao.skip = skip;
    ao.out = d_out;
    ao.out_stride = out_stride;
    ao.n_out = p.n_out;
    ao.volume = a->volume;
    ao.B = h->B;
    if (timed) HIP_TRY(hipEventRecord(a->ev[2], s));
    HIP_TRY(rn_launch_adapt_out(ao, s));
    if (timed) HIP_TRY(hipEventRecord(a->ev[3], s));
    a->timed = timed;
    if (h->lg) h->lg->rec_rate = a->resample ? 48000.f : a->rate;      // the callback resampler's set_rates: it passes through (audio.rs:706-709)
    if (RnPlayback* pb = h->pb.get()) {      // playback configured: what push_sample appends to output_buf (audio.rs:280-285)
      rc = ring_append(pb->ring.p, pb->buf, pb->cap, d_out, out_stride, p.n_out, h->B, s);
      if (rc != CRISPY_OK) return rc;
    }
    if (recording(h)) {     // what push_mono_to_buffers appends to the recording ring (audio.rs:701-726)
      rc = ring_append(h->rec->mic_ring.p, h->rec->mic, h->rec->cap, d_out, out_stride, p.n_out, h->B, s);
      if (rc != CRISPY_OK) return rc;
    }
  }
  *n_out = p.n_out;
  return CRISPY_OK;
}

}  // namespace crispy

// ---- pull -------------------------------------------------------------------------------------------------------------

// next_sample (audio.rs:297-314), n_frames times, on copies of the state: the reference's own recurrence, never a closed form
PullPlan crispy::plan_pull(RnPlayback* p, long n_frames) {
  const double step = (double)p->in_rate / (double)p->out_rate;
  PullPlan pl;
  pl.len = p->buf.len;
  pl.pos = p->pos;
  p->off.resize((size_t)n_frames);
  p->frac.resize((size_t)n_frames);
  for (long f = 0; f < n_frames; ++f) {
    p->off[f] = -1;
    p->frac[f] = 0.f;
    if (pl.len < 2) continue;
    while (pl.pos >= 1.0 && pl.len >= 2) {
      ++pl.pops;
      --pl.len;
      pl.pos -= 1.0;
    }
    if (pl.len < 2) continue;         // ran dry while popping: 0.0, the pops and the decrements stay
    p->off[f] = (int)pl.pops;
    p->frac[f] = (float)pl.pos;
    pl.pos += step;
    ++pl.live;
  }
  return pl;
}

namespace {

// A fresh output_buf of one second at in_rate and resample_pos = 0.  The ring is state: it is replaced only when its size
// changes, the new one allocated before the old one goes, so a failure leaves the handle as it was.
int playback_fresh_ring(crispy_rn* h, RnPlayback* p, float in_rate, const char* who) {
  const int cap = (int)(size_t)in_rate;      // `as usize`: 47999 or 48000 (a rate a whole hertz off 48 kHz is resampled to it)
  if (cap < 2) return fail(CRISPY_ERR_INVALID_ARG, "%s: a ring of %d samples", who, cap);
  if (cap != p->cap || !p->ring.p) {
    DevBuf<float> fresh;
    const size_t bytes = (size_t)h->B * cap * sizeof(float);
    if (fresh.alloc(bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: ring allocation of %zu bytes failed", who, bytes);
    }
    p->ring = std::move(fresh);      // (the old one is freed with `fresh`; hipFree waits for the work that still reads it)
  }
  p->in_rate = in_rate;
  p->cap = cap;
  p->buf = RingPos();
  p->pos = 0.;
  return CRISPY_OK;
}

// The arguments every pull checks, before anything is touched.
int check_pull(const crispy_rn* h, long n_frames, int channels, int format, const void* out, long out_stride, const char* who) {
  if (!h->pb) return fail(CRISPY_ERR_INVALID_ARG, "%s: playback not configured (crispy_rn_playback_configure)", who);
  if (n_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames < 0", who);
  if (n_frames > kPullMaxFrames) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames %ld above the limit of %ld frames per pull", who, n_frames, kPullMaxFrames);
  if (channels < 1 || channels > 8) return fail(CRISPY_ERR_INVALID_ARG, "%s: channels %d outside 1...8", who, channels);
  if (format != CRISPY_PCM_F32 && format != CRISPY_PCM_I16 && format != CRISPY_PCM_U16)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown format %d", who, format);
  if (n_frames == 0) return CRISPY_OK;
  if (!out) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL output pointer", who);
  if (out_stride < n_frames * channels)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld elements of this pull", who, out_stride, n_frames * channels);
  return CRISPY_OK;
}

// Arguments checked (check_pull), n_frames > 0, the handle's device current.
int pull_device_impl(crispy_rn* h, long n_frames, int channels, int format, void* d_out, long out_stride, long* n_live, hipStream_t s,
                     const char* who) {
  RnPlayback* p = h->pb.get();
  const PullPlan pl = plan_pull(p, n_frames);
  const long len = pl.len, pops = pl.pops, live = pl.live;
  const double pos = pl.pos;
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
  RnPull a{};
  a.ring = p->ring.p;
  a.cap = p->cap;
  a.head = p->buf.head;
  a.off = p->frames.dev.p;
  a.frac = reinterpret_cast<const float*>(p->frames.dev.p + n_frames);
  a.out = d_out;
  a.out_stride = out_stride;
  a.n_frames = (unsigned)n_frames;
  a.n_elems = (unsigned)(n_frames * channels);
  a.channels = (unsigned)channels;
  a.B = h->B;
  HIP_TRY(rn_launch_pull(a, format, s));
  p->buf.head = (int)((p->buf.head + pops) % p->cap);
  p->buf.len = (int)len;
  p->pos = pos;
  if (n_live) *n_live = live;
  return CRISPY_OK;
}

}  // namespace

// ---- record -----------------------------------------------------------------------------------------------------------

namespace crispy {

int check_app_push(const crispy_rn* h, const float* in, long in_stride, long n_frames, int channels, const char* who) {
  if (!recording(h)) return fail(CRISPY_ERR_INVALID_ARG, "%s: recording not configured (crispy_rn_record_configure)", who);
  if (n_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames < 0", who);
  if (n_frames > kLevelMaxIn) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames %ld above the limit of %ld frames per push", who, n_frames, kLevelMaxIn);
  if (channels < 1 || channels > 8) return fail(CRISPY_ERR_INVALID_ARG, "%s: channels %d outside 1...8", who, channels);
  if (n_frames == 0) return CRISPY_OK;
  if (!in) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL audio pointer", who);
  if (in_stride < n_frames * channels)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than the %ld samples of this push", who, in_stride, n_frames * channels);
  return CRISPY_OK;
}

// Arguments checked (check_app_push), n_frames > 0, the handle's device current.
int app_push_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, hipStream_t s) {
  RnRecord* r = h->rec.get();
  const AppendPlan p = plan_append(r->app, r->cap, n_frames);
  RnRecApp a{};
  a.in = d_in + p.skip * channels;
  a.in_stride = in_stride;
  a.ring = r->app_ring.p;
  a.cap = r->cap;
  a.tail = p.tail;
  a.n = p.n;
  a.channels = channels;
  a.B = h->B;
  HIP_TRY(rn_launch_rec_app(a, s));
  r->app = p.after;
  return CRISPY_OK;
}

}  // namespace crispy

namespace {

int check_level(const float* in, long in_stride, long n_in, const float* rms, const char* who) {
  if (n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in < 0", who);
  if (n_in > kLevelMaxIn) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in %ld above the limit of %ld samples per call", who, n_in, kLevelMaxIn);
  if (n_in == 0) return CRISPY_OK;
  if (!in || !rms) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL pointer", who);
  if (in_stride < n_in) return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than n_in %ld", who, in_stride, n_in);
  return CRISPY_OK;
}

}  // namespace

int crispy::level_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_rms, hipStream_t s) {
  RnLevel a{};
  a.in = d_in;
  a.in_stride = in_stride;
  a.n = (int)n_in;
  a.rms = d_rms;
  a.B = h->B;
  HIP_TRY(rn_launch_level(a, s));
  return CRISPY_OK;
}

namespace {

// The arguments every drain checks before it plans.
int check_drain(const crispy_rn* h, long max_frames, int format, const void* out, const long* n_frames, const char* who) {
  if (!recording(h)) return fail(CRISPY_ERR_INVALID_ARG, "%s: recording not configured (crispy_rn_record_configure)", who);
  if (max_frames < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: max_frames < 0", who);
  if (format != CRISPY_PCM_F32 && format != CRISPY_PCM_I16) return fail(CRISPY_ERR_INVALID_ARG, "%s: unknown format %d", who, format);
  if (!out || !n_frames) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL out / n_frames pointer", who);
  return CRISPY_OK;
}

// Arguments checked (check_drain), the handle's device current.  stride_of(n): the output rows and the row stride to use for n
// frames (the host form sizes its staging rows from it), or an error status with the message recorded.
template <class StrideOf>
int drain_device_impl(crispy_rn* h, long max_frames, int format, StrideOf stride_of, long* n_frames, hipStream_t s, const char* who,
                      void** d_out_used, long* stride_used) {
  RnRecord* r = h->rec.get();
  // frames a drain of at most max_frames writes now, and their positions
  long cap_frames = r->mic.len / REC_FRAME;
  if (cap_frames > max_frames) cap_frames = max_frames;
  r->mic_off.resize((size_t)cap_frames);
  r->app_off.resize((size_t)cap_frames);
  long mic_left = 0, app_left = 0;
  const long n = crispy_record_worker_plan(r->mic.len, r->app.len, max_frames, r->mic_off.data(), r->app_off.data(), &mic_left, &app_left);
  if (n < 0) return (int)n;
  if (n == 0) {
    *n_frames = 0;
    return CRISPY_OK;
  }
  void* d_out = nullptr;
  long out_stride = 0;
  int rc = stride_of(n, &d_out, &out_stride);
  if (rc != CRISPY_OK) return rc;
  // nothing is launched on an offset that leaves what the ring holds
  for (long f = 0; f < n; ++f) {
    if (r->mic_off[f] < 0 || r->mic_off[f] + REC_FRAME > r->mic.len || (r->app_off[f] >= 0 && r->app_off[f] + REC_FRAME > r->app.len))
      return fail(CRISPY_ERR_HIP, "%s: frame %ld of the plan lies outside the rings (mic %ld of %d, app %ld of %d)", who, f, r->mic_off[f],
                  r->mic.len, r->app_off[f], r->app.len);
  }
  // every allocation first: a failure from here on returns with the handle's state as it was
  const size_t words = (size_t)2 * n;
  rc = r->offs.reserve(words, who);
  if (rc != CRISPY_OK) return rc;

  // ---- enqueue ----
  rc = r->offs.send(words, s, [&](int* slot) {
    for (long f = 0; f < n; ++f) {
      slot[f] = (int)r->mic_off[f];
      slot[n + f] = (int)r->app_off[f];
    }
  });
  if (rc != CRISPY_OK) return rc;
  RnRecDrain a{};
  a.mic = r->mic_ring.p;
  a.app = r->app_ring.p;
  a.cap = r->cap;
  a.mic_head = r->mic.head;
  a.app_head = r->app.head;
  a.mic_off = r->offs.dev.p;
  a.app_off = r->offs.dev.p + n;
  a.out = d_out;
  a.out_stride = out_stride;
  a.n_samples = (unsigned)(n * REC_FRAME);
  a.B = h->B;
  HIP_TRY(rn_launch_rec_drain(a, format, s));
  r->mic.head = (int)(((long)r->mic.head + (r->mic.len - mic_left)) % r->cap);
  r->mic.len = (int)mic_left;
  r->app.head = (int)(((long)r->app.head + (r->app.len - app_left)) % r->cap);
  r->app.len = (int)app_left;
  *n_frames = n;
  if (d_out_used) *d_out_used = d_out;
  if (stride_used) *stride_used = out_stride;
  return CRISPY_OK;
}

}  // namespace

extern "C" {

// ---- push -------------------------------------------------------------------------------------------------------------

int crispy_rn_adapter_configure(crispy_rn* h, float input_rate, float volume) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_configure: NULL handle");
  if (!(input_rate > 0.f) || !std::isfinite(input_rate))
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_configure: input_rate must be a positive number of Hz");
  if (volume != volume) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_configure: volume is NaN");
  HIP_TRY(hipSetDevice(h->device));
  const bool resample = std::fabs(input_rate - 48000.f) >= 1.f;
  // NsState::Legacy: a fresh SharedAudio of the same kind (audio.rs:136-149) -- the ring holds raw samples at the raw rate
  const bool legacy = legacy_active(h);
  // the new processor's output_buf and resample_pos, on a handle with playback configured; first, as it may allocate
  int rc = h->pb ? playback_fresh_ring(h, h->pb.get(), resample && !legacy ? 48000.f : input_rate, "crispy_rn_adapter_configure") : CRISPY_OK;
  if (rc != CRISPY_OK) return rc;
  if (legacy) {
    (void)adapter_of(h);       // (may throw: before anything changes)
    h->lg->rng = NS_LCG_SEED;
  } else {
    rc = rn_zero_state(h, -1);
    if (rc != CRISPY_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  RnAdapter* a = adapter_of(h);
  a->rate = input_rate;
  a->resample = resample;
  a->volume = volume < 0.f ? 0.f : (volume > 1.f ? 1.f : volume);
  a->first = true;
  a->rs = LinResState();
  a->carry_len = 0;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_adapter_configure")

int crispy_rn_adapter_set_volume(crispy_rn* h, float volume) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_set_volume: NULL handle");
  if (volume != volume) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_set_volume: volume is NaN");
  RnAdapter* a = adapter_of(h);
  a->volume = volume < 0.f ? 0.f : (volume > 1.f ? 1.f : volume);
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_adapter_set_volume")

int crispy_rn_adapter_produced_rate_hz(const crispy_rn* h, float* rate_hz) try {
  if (!h || !rate_hz) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_produced_rate_hz: NULL argument");
  const RnAdapter* a = adapter_of(h);
  *rate_hz = a->resample && !legacy_active(h) ? 48000.f : a->rate;      // NsState::Legacy: s.input_rate, the raw rate
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_adapter_produced_rate_hz")

long crispy_rn_push_out_len(const crispy_rn* h, long n_in) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_out_len: NULL handle");
  PushPlan p;
  const int rc = plan_push(adapter_of(h), n_in, nullptr, nullptr, &p, "crispy_rn_push_out_len");
  if (rc == CRISPY_OK && legacy_active(h)) return n_in;      // SharedAudio::push_sample: Some(vec![processed])
  return rc != CRISPY_OK ? rc : p.n_out;
} CRISPY_CATCH_RET("crispy_rn_push_out_len")

int crispy_rn_push_device(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_out, long out_stride,
                          float* d_frames48, long frames_stride, float* d_vad, long* n_out, void* hip_stream) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_device: NULL handle");
  if (!n_out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_device: n_out is NULL");
  *n_out = 0;
  if (n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_device: n_in < 0");
  if (n_in == 0) return CRISPY_OK;
  if (!d_in || !d_out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_device: NULL audio pointer");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  if (legacy_active(h)) {
    if (d_frames48 || d_vad) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_device: a Legacy model has no frames and no VAD (d_frames48 / d_vad must be NULL)");
    return h->lg->push(h, d_in, in_stride, n_in, d_out, out_stride, n_out, s, "crispy_rn_push_device");
  }
  return push_device_impl(h, d_in, in_stride, n_in, d_out, out_stride, d_frames48, frames_stride, d_vad, n_out, s, "crispy_rn_push_device");
} CRISPY_CATCH_RET("crispy_rn_push_device")

int crispy_rn_push(crispy_rn* h, const float* in, long in_stride, long n_in, float* out, long out_stride, float* vad,
                   long* n_out) try {
  const char* who = "crispy_rn_push";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_out is NULL", who);
  *n_out = 0;
  if (n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_in < 0", who);
  if (n_in == 0) return CRISPY_OK;
  if (!in || !out) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL audio pointer", who);
  if (in_stride < n_in) return fail(CRISPY_ERR_INVALID_ARG, "%s: in_stride %ld shorter than n_in %ld", who, in_stride, n_in);
  PushPlan p;
  int rc = plan_push(adapter_of(h), n_in, nullptr, nullptr, &p, who);
  if (rc != CRISPY_OK) return rc;
  const bool legacy = legacy_active(h);
  if (legacy) {
    if (vad) return fail(CRISPY_ERR_INVALID_ARG, "%s: a Legacy model has no VAD (vad must be NULL)", who);
    p.n_out = n_in;
    p.frames = 0;
  }
  if (out_stride < p.n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld samples of this push", who, out_stride, p.n_out);
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)h->B;
  rc = h->stage_reserve(B * (size_t)n_in * sizeof(float), B * (size_t)(p.n_out > 0 ? p.n_out : 1) * sizeof(float),
                        vad ? B * (size_t)(p.frames > 0 ? p.frames : 1) * sizeof(float) : 0, who);
  if (rc != CRISPY_OK) return rc;
  float* d_hin = reinterpret_cast<float*>(h->stage_in.p);
  float* d_hout = reinterpret_cast<float*>(h->stage_out.p);
  float* d_hvad = vad ? h->stage_aux.p : nullptr;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(d_hin, (size_t)n_in * sizeof(float), in, (size_t)in_stride * sizeof(float), (size_t)n_in * sizeof(float),
                           B, hipMemcpyHostToDevice, s));
  long got = 0;
  rc = legacy ? h->lg->push(h, d_hin, n_in, n_in, d_hout, p.n_out, &got, s, who)
              : push_device_impl(h, d_hin, n_in, n_in, d_hout, p.n_out, nullptr, 0, d_hvad, &got, s, who);
  if (rc != CRISPY_OK) return rc;
  if (got > 0)
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * sizeof(float), d_hout, (size_t)got * sizeof(float), (size_t)got * sizeof(float),
                             B, hipMemcpyDeviceToHost, s));
  if (vad && p.frames > 0)
    HIP_TRY(hipMemcpyAsync(vad, d_hvad, (size_t)p.frames * B * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *n_out = got;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_push")

int crispy_rn_last_push_ms(crispy_rn* h, float* adapt_in_ms, float* adapt_out_ms) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_last_push_ms: NULL handle");
  const RnAdapter* a = adapter_of(static_cast<const crispy_rn*>(h));
  if (!a->timed) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_last_push_ms: no timed push that returned samples recorded");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipEventSynchronize(a->ev[3]));
  float ms_in = 0.f, ms_out = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_in, a->ev[0], a->ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms_out, a->ev[2], a->ev[3]));
  if (adapt_in_ms) *adapt_in_ms = ms_in;
  if (adapt_out_ms) *adapt_out_ms = ms_out;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_last_push_ms")

long crispy_linear_resampler_count(float input_rate, float output_rate, long n_before, long n_in) try {
  if (n_before < 0 || n_in < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_linear_resampler_count: negative sample count");
  if (!(input_rate > 0.f) || !(output_rate > 0.f) || !std::isfinite(input_rate) || !std::isfinite(output_rate))
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_linear_resampler_count: rates must be positive numbers of Hz");
  if (std::fabs(input_rate - output_rate) < 1.f) return n_in;
  const double step = (double)(input_rate / output_rate);
  const long no_limit = 0x7fffffffffffffffL;
  LinResState st;
  (void)linres_advance(st, step, n_before, no_limit, nullptr, nullptr);
  return linres_advance(st, step, n_in, no_limit, nullptr, nullptr);
} CRISPY_CATCH_RET("crispy_linear_resampler_count")

// ---- pull -------------------------------------------------------------------------------------------------------------

int crispy_rn_playback_configure(crispy_rn* h, float output_rate) try {
  const char* who = "crispy_rn_playback_configure";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!(output_rate > 0.f) || !std::isfinite(output_rate))
    return fail(CRISPY_ERR_INVALID_ARG, "%s: output_rate must be a positive number of Hz", who);
  HIP_TRY(hipSetDevice(h->device));
  float in_rate = 48000.f;
  int rc = crispy_rn_adapter_produced_rate_hz(h, &in_rate);
  if (rc != CRISPY_OK) return rc;
  if (!h->pb) {
    std::unique_ptr<RnPlayback> fresh(new RnPlayback());      // (std::bad_alloc: the guard makes it CRISPY_ERR_OOM)
    rc = playback_fresh_ring(h, fresh.get(), in_rate, who);
    if (rc != CRISPY_OK) return rc;
    h->pb = std::move(fresh);
  } else {
    rc = playback_fresh_ring(h, h->pb.get(), in_rate, who);
    if (rc != CRISPY_OK) return rc;
  }
  h->pb->out_rate = output_rate;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_playback_configure")

long crispy_rn_playback_buffered(const crispy_rn* h) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_playback_buffered: NULL handle");
  return h->pb ? h->pb->buf.len : 0;
} CRISPY_CATCH_RET("crispy_rn_playback_buffered")

int crispy_rn_pull_device(crispy_rn* h, long n_frames, int channels, int format, void* d_out, long out_stride, long* n_live,
                          void* hip_stream) try {
  const char* who = "crispy_rn_pull_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_pull(h, n_frames, channels, format, d_out, out_stride, who);
  if (rc != CRISPY_OK) return rc;
  if (n_live) *n_live = 0;
  if (n_frames == 0) return CRISPY_OK;
  HIP_TRY(hipSetDevice(h->device));
  const auto pull = legacy_active(h) ? h->lg->pull : pull_device_impl;
  return pull(h, n_frames, channels, format, d_out, out_stride, n_live, hip_stream ? (hipStream_t)hip_stream : h->stream, who);
} CRISPY_CATCH_RET("crispy_rn_pull_device")

int crispy_rn_pull(crispy_rn* h, long n_frames, int channels, int format, void* out, long out_stride, long* n_live) try {
  const char* who = "crispy_rn_pull";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_pull(h, n_frames, channels, format, out, out_stride, who);
  if (rc != CRISPY_OK) return rc;
  if (n_live) *n_live = 0;
  if (n_frames == 0) return CRISPY_OK;
  HIP_TRY(hipSetDevice(h->device));
  const size_t row = (size_t)n_frames * channels * pcm_bytes(format);       // a multiple of 16 when it matters: rows stay aligned
  const size_t pitch = (row + 15) & ~(size_t)15;
  rc = h->stage_reserve(0, (size_t)h->B * pitch, 0, who);
  if (rc != CRISPY_OK) return rc;
  hipStream_t s = h->stream;
  const auto pull = legacy_active(h) ? h->lg->pull : pull_device_impl;
  rc = pull(h, n_frames, channels, format, h->stage_out.p, (long)(pitch / pcm_bytes(format)), n_live, s, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * pcm_bytes(format), h->stage_out.p, pitch, row, (size_t)h->B, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_pull")

// ---- record -----------------------------------------------------------------------------------------------------------

// The recording worker's loop (commands/recording.rs:196-264) on lengths alone.
long crispy_record_worker_plan(long mic_len, long app_len, long max_frames, long* mic_off, long* app_off, long* mic_left,
                               long* app_left) try {
  if (mic_len < 0 || app_len < 0 || max_frames < 0)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_record_worker_plan: negative length or frame count");
  long n = 0, mic_pop = 0, app_pop = 0;
  while (mic_len >= REC_FRAME && n < max_frames) {
    // align the heads when one source is more than 50 ms ahead (commands/recording.rs:221-239)
    if (mic_len > app_len + REC_MAX_DESYNC) {
      const long trim = mic_len - app_len - REC_MAX_DESYNC;
      mic_pop += trim;
      mic_len -= trim;
    } else if (app_len > mic_len + REC_MAX_DESYNC) {
      const long trim = app_len - mic_len - REC_MAX_DESYNC;
      app_pop += trim;
      app_len -= trim;
    }
    if (mic_off) mic_off[n] = mic_pop;
    mic_pop += REC_FRAME;
    mic_len -= REC_FRAME;
    if (app_len >= REC_FRAME) {
      if (app_off) app_off[n] = app_pop;
      app_pop += REC_FRAME;
      app_len -= REC_FRAME;
    } else if (app_off) {
      app_off[n] = -1;           // a frame of zeros; the app deque stays as it is
    }
    ++n;
  }
  if (mic_left) *mic_left = mic_len;
  if (app_left) *app_left = app_len;
  return n;
} CRISPY_CATCH_RET("crispy_record_worker_plan")

int crispy_rn_record_configure(crispy_rn* h, long ring_samples) try {
  const char* who = "crispy_rn_record_configure";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const long cap = ring_samples == 0 ? REC_DEFAULT_CAP : ring_samples;
  if (cap < 2 * REC_FRAME || cap > REC_MAX_CAP)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: ring_samples %ld outside %d...%ld (0 = %ld)", who, ring_samples, 2 * REC_FRAME, REC_MAX_CAP,
                REC_DEFAULT_CAP);
  HIP_TRY(hipSetDevice(h->device));
  RnRecord* r = record_of(h);
  if (cap != r->cap) {
    // the rings are state: both new ones before an old one goes, so a failure leaves the handle as it was
    DevBuf<float> mic, app;
    const size_t bytes = (size_t)h->B * (size_t)cap * sizeof(float);
    if (mic.alloc(bytes) != hipSuccess || app.alloc(bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: ring allocation of 2 x %zu bytes failed", who, bytes);
    }
    r->mic_ring = std::move(mic);      // (the old ones are freed with the locals; hipFree waits for the work that still reads them)
    r->app_ring = std::move(app);
    r->cap = (int)cap;
  }
  r->mic = RingPos();
  r->app = RingPos();
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_configure")

int crispy_rn_record_buffered(const crispy_rn* h, long* mic, long* app) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_record_buffered: NULL handle");
  const bool on = recording(h);
  if (mic) *mic = on ? h->rec->mic.len : 0;
  if (app) *app = on ? h->rec->app.len : 0;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_buffered")

long crispy_rn_record_frames_ready(const crispy_rn* h) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_record_frames_ready: NULL handle");
  if (!recording(h)) return 0;
  return crispy_record_worker_plan(h->rec->mic.len, h->rec->app.len, 0x7fffffffffffffffL, nullptr, nullptr, nullptr, nullptr);
} CRISPY_CATCH_RET("crispy_rn_record_frames_ready")

int crispy_rn_record_app_push_device(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, void* hip_stream) try {
  const char* who = "crispy_rn_record_app_push_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_app_push(h, d_in, in_stride, n_frames, channels, who);
  if (rc != CRISPY_OK || n_frames == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return app_push_device_impl(h, d_in, in_stride, n_frames, channels, hip_stream ? (hipStream_t)hip_stream : h->stream);
} CRISPY_CATCH_RET("crispy_rn_record_app_push_device")

int crispy_rn_record_app_push(crispy_rn* h, const float* in, long in_stride, long n_frames, int channels) try {
  const char* who = "crispy_rn_record_app_push";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_app_push(h, in, in_stride, n_frames, channels, who);
  if (rc != CRISPY_OK || n_frames == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t row = (size_t)n_frames * channels;
  rc = h->stage_reserve((size_t)h->B * row * sizeof(float), 0, 0, who);
  if (rc != CRISPY_OK) return rc;
  float* d_hin = reinterpret_cast<float*>(h->stage_in.p);
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(d_hin, row * sizeof(float), in, (size_t)in_stride * sizeof(float), row * sizeof(float), (size_t)h->B,
                           hipMemcpyHostToDevice, s));
  rc = app_push_device_impl(h, d_hin, (long)row, n_frames, channels, s);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_app_push")

int crispy_rn_level_device(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_rms, void* hip_stream) try {
  const char* who = "crispy_rn_level_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_level(d_in, in_stride, n_in, d_rms, who);
  if (rc != CRISPY_OK || n_in == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return level_device_impl(h, d_in, in_stride, n_in, d_rms, hip_stream ? (hipStream_t)hip_stream : h->stream);
} CRISPY_CATCH_RET("crispy_rn_level_device")

int crispy_rn_level(crispy_rn* h, const float* in, long in_stride, long n_in, float* rms) try {
  const char* who = "crispy_rn_level";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_level(in, in_stride, n_in, rms, who);
  if (rc != CRISPY_OK || n_in == 0) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)h->B;
  rc = h->stage_reserve(B * (size_t)n_in * sizeof(float), 0, B * sizeof(float), who);
  if (rc != CRISPY_OK) return rc;
  float* d_hin = reinterpret_cast<float*>(h->stage_in.p);
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(d_hin, (size_t)n_in * sizeof(float), in, (size_t)in_stride * sizeof(float), (size_t)n_in * sizeof(float), B,
                           hipMemcpyHostToDevice, s));
  rc = level_device_impl(h, d_hin, n_in, n_in, h->stage_aux.p, s);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(rms, h->stage_aux.p, B * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_level")

int crispy_rn_record_drain_device(crispy_rn* h, long max_frames, int format, void* d_out, long out_stride, long* n_frames,
                                  void* hip_stream) try {
  const char* who = "crispy_rn_record_drain_device";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  const int rc = check_drain(h, max_frames, format, d_out, n_frames, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  auto stride_of = [&](long n, void** p, long* stride) {
    if (out_stride < n * rec_elems_per_frame(format))
      return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld elements of this drain", who, out_stride,
                  n * rec_elems_per_frame(format));
    *p = d_out;
    *stride = out_stride;
    return (int)CRISPY_OK;
  };
  return drain_device_impl(h, max_frames, format, stride_of, n_frames, hip_stream ? (hipStream_t)hip_stream : h->stream, who, nullptr, nullptr);
} CRISPY_CATCH_RET("crispy_rn_record_drain_device")

int crispy_rn_record_drain(crispy_rn* h, long max_frames, int format, void* out, long out_stride, long* n_frames) try {
  const char* who = "crispy_rn_record_drain";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_drain(h, max_frames, format, out, n_frames, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  const size_t eb = pcm_bytes(format);
  auto stride_of = [&](long n, void** p, long* stride) {
    const long elems = n * rec_elems_per_frame(format);        // a row is a multiple of 16 bytes: staging rows stay aligned
    if (out_stride < elems)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld elements of this drain", who, out_stride, elems);
    const int rc_stage = h->stage_reserve(0, (size_t)h->B * (size_t)elems * eb, 0, who);
    if (rc_stage != CRISPY_OK) return rc_stage;
    *p = h->stage_out.p;
    *stride = elems;
    return (int)CRISPY_OK;
  };
  hipStream_t s = h->stream;
  long n = 0, stride = 0;
  void* d_out = nullptr;
  rc = drain_device_impl(h, max_frames, format, stride_of, &n, s, who, &d_out, &stride);
  if (rc != CRISPY_OK) return rc;
  if (n > 0) {
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * eb, d_out, (size_t)stride * eb, (size_t)stride * eb, (size_t)h->B,
                             hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  *n_frames = n;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_record_drain")

}  // extern "C"

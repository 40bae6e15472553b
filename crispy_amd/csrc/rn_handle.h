// rn_handle.h -- the RNNoise handle behind `crispy_rn` (include/crispy_hip.h) and the state of its three halves, shared by
// the translation units that implement its entry points: crispy_api.cpp (create / process / reset ...), rn_io.cpp
// (crispy_rn_push*, crispy_rn_pull*, crispy_rn_record_*, crispy_rn_level*), rn_capture_io.cpp (crispy_rn_capture*,
// crispy_rn_bypass_configure, crispy_rn_record_app_push_at*) and rn_legacy_io.cpp (crispy_rn_model*, the Legacy arm).  Everything here owns what it holds: device
// buffers are DevBuf, events EventList (api_util.h), streams Stream, the halves unique_ptr members -- deleting the handle
// releases all of it, streams last.  The types are plain state; the logic that drives them is in the .cpp files.
#pragma once
#include <cstddef>
#include <memory>
#include <vector>

#include "../../include/crispy_hip.h"
#include "api_util.h"
#include "rn_common.h"

namespace crispy {

// A stream the handle created: destroyed with it.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
};

// A table of 32-bit words that a call works out on the host and its kernel reads: the device table, two pinned host slots
// used in turns, and one event per slot -- the slot's copy has been read.  A slot is never rewritten before its previous
// upload has been read, so a call does not wait for the one before it, only for the one before that.
struct PinnedUpload {
  // A pinned allocation, released through the deleter reserve() gives it (rn_io.cpp): this header and crispy_api.cpp, which
  // deletes the handle, stay free of the pinned-memory API.
  using Slot = std::unique_ptr<int, hipError_t (*)(void*)>;
  DevBuf<int> dev;
  Slot host[2] = {Slot(nullptr, nullptr), Slot(nullptr, nullptr)};
  size_t host_words[2] = {0, 0};
  EventList ev;
  int slot = 0;
  // Every allocation of an upload of `words` words (rn_io.cpp).  The table is scratch (DevBuf::grow); the slot is replaced only
  // once the new one exists and the old one's upload has been read.
  int reserve(size_t words, const char* who);
  // fill(int* slot) writes the `words` reserved words; they are in `dev` once what is enqueued on s here has run.
  template <class Fill>
  int send(size_t words, hipStream_t s, Fill fill) {
    HIP_TRY(hipEventSynchronize(ev[slot]));      // the upload that used this slot two calls ago (no-op before)
    fill(host[slot].get());
    HIP_TRY(hipMemcpyAsync(dev.p, host[slot].get(), words * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(ev[slot], s));
    slot ^= 1;
    return CRISPY_OK;
  }
};

// A deque of the reference kept as a ring: where the front is and how many samples it holds.
struct RingPos {
  int head = 0;
  int len = 0;
};

// LinearResampler::process_sample's position state (audio.rs:108-133); the same for every stream of a handle.
struct LinResState {
  bool has_last = false;
  double input_pos = 0., next_pos = 0.;
};

// RnnNoiseProcessor's state around process_frame (audio.rs:202-213) for all streams of a handle, and the adapter's buffers.
// Created with the defaults -- 48 kHz, volume 1 -- when a handle is first pushed to or configured.
struct RnAdapter {
  float rate = 48000.f;     // capture rate as configured; within 1 Hz of 48 kHz: no resampler
  bool resample = false;
  float volume = 1.f;
  bool first = true;        // first_frame
  LinResState rs;           // LinearResampler::has_last / input_pos / next_output_pos
  int carry_len = 0;        // input_buf.len(), < 480 between pushes
  int cur = 0;              // which half of the double-buffered per-stream state is current
  DevBuf<float> carry;      // state [2][B][480]
  DevBuf<float> last;       // state [2][B]: LinearResampler::last_sample
  DevBuf<float> stage, y;   // scratch [B][frames * 480] each: frames into / out of the frame kernels
  PinnedUpload pos;         // (idx[n], t[n]) of the current push
  std::vector<int> idx;     // host scratch of one push
  std::vector<float> t;
  EventList ev;             // timing, four: around rn_adapt_in_kernel / rn_adapt_out_kernel
  bool timed = false;
};

// NsState's playback side (audio.rs:208-212: output_buf, max_output_len, resample_pos, output_rate) for all streams of a
// handle.  Created by crispy_rn_playback_configure; a handle without one has no ring and pushes as before.
struct RnPlayback {
  float out_rate = 48000.f;
  float in_rate = 48000.f;   // effective input rate: 48000 with the input resampler, else the configured capture rate
  int cap = 0;               // max_output_len = in_rate as usize
  RingPos buf;               // output_buf
  double pos = 0.;           // resample_pos
  DevBuf<float> ring;        // state [B][cap]
  PinnedUpload frames;       // (off[n], frac[n]) of the current pull
  std::vector<int> off;      // host scratch of one pull
  std::vector<float> frac;
};

// The recording state's two buffers (the mic ring that push_mono_to_buffers fills, the app ring of the capture handlers) for
// all streams of a handle.  The object is created on first use; the rings exist, and the handle records, from
// crispy_rn_record_configure on (cap > 0).
struct RnRecord {
  int cap = 0;
  RingPos mic, app;
  DevBuf<float> mic_ring;    // state [B][cap]
  DevBuf<float> app_ring;
  PinnedUpload offs;         // (mic_off[n], app_off[n]) of the current drain
  std::vector<long> mic_off, app_off;     // host scratch of one drain
};

// The capture callback in front of push_sample (crispy_rn_capture*): the mono row of the current capture and, for the
// `shared == None` arm of push_mono_to_buffers (audio.rs:697-714), the callback's own LinearResampler(input_rate, 48000).
// Created on first use; a handle without one captures into the RNNoise arm.
struct RnCaptureState {
  float bypass_rate = 0.f;  // > 0: noise suppression off, the raw capture rate; 0: the RNNoise arm
  bool resample = false;    // the bypass resampler is in: the rate is 1 Hz or more off 48 kHz
  LinResState rs;           // its has_last / input_pos / next_output_pos
  int cur = 0;              // which half of `last` is current
  DevBuf<float> last;       // state [2][B]: its last_sample
  PinnedUpload pos;         // (idx[n], t[n]) of the current capture
  std::vector<int> idx;     // host scratch of one capture
  std::vector<float> t;
  DevBuf<float> mono;       // scratch [B][mono_stride]: the mono of a capture whose caller does not ask for it
};

// NsState's other variant, Legacy(SharedAudio) (audio.rs:47-71, 136-200, 317-358), and which variant the handle is: created by
// the first crispy_rn_model_configure; a handle without one is the RNNoise arm.  SharedAudio's rates and volume are the
// adapter's (RnAdapter::rate, ::volume), its buffer, max_len and resample_pos the playback ring's (RnPlayback, sized from the
// raw rate); its own are the model kind and the LCG state, the same for every stream as ring heads are.
// crispy_api.cpp and rn_io.cpp read and write the plain fields and reach the arm's code only through the pointers here,
// which crispy_rn_model_configure sets: they link without rn_legacy_io.cpp and rn_legacy.hip (tests/asan/harness.cpp).
struct RnLegacy {
  int model = CRISPY_NS_RNNOISE;
  uint32_t rng = NS_LCG_SEED;     // rng_state: one step per sample a Noisy push returned or a Noisy pull found live
  // input_rate of the capture callback's LinearResampler(_, 48000) (audio.rs:701-709), whose positions and last samples are
  // RnCaptureState's: what the last push that returned samples produced.  A Legacy push that produces 1 Hz or more off
  // it is the callback's set_rates: the resampler starts afresh.
  float rec_rate = 48000.f;
  DevBuf<float> rec;              // scratch [B][stride]: what that resampler emitted of one push, on its way to the mic ring
  // SharedAudio::push_sample over a block + the rest of push_mono_to_buffers; arguments checked as push_device_impl's
  int (*push)(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_out, long out_stride, long* n_out, hipStream_t s,
              const char* who) = nullptr;
  // SharedAudio::next_sample over a block; the contract of rn_io.cpp's pull_device_impl
  int (*pull)(crispy_rn* h, long n_frames, int channels, int format, void* d_out, long out_stride, long* n_live, hipStream_t s,
              const char* who) = nullptr;
};

}  // namespace crispy

struct crispy_rn {
  int device = 0;
  int B = 0;
  // The streams come first: members go in reverse order, so every buffer and event is released before a stream is.
  crispy::Stream stream;
  crispy::Stream hp_stream;   // helper stream: the latency-bound high-pass runs beside the frame kernel
  crispy::Stream h2d_stream, d2h_stream;   // pipelined host path: copy-in / copy-out beside the compute stream
  crispy::EventList ev_begin;        // one
  crispy::EventList ev_hp;           // one per sub-chunk: high-pass done
  // constants
  crispy::DevBuf<crispy::RnTables> d_tab;
  crispy::DevBuf<uint32_t> d_wpack;
  // state
  crispy::DevBuf<float> d_hp_mem;
  crispy::DevBuf<float> d_synth;       // overlap-add tails [B][480]
  crispy::DevBuf<float> d_ceps;
  crispy::DevBuf<float> d_lastg;
  crispy::DevBuf<float> d_rnn;
  crispy::DevBuf<float> d_last_gain;
  crispy::DevBuf<int> d_last_period;
  crispy::DevBuf<int> d_memid;
  // workspace
  crispy::DevBuf<float> d_xhp;
  long xhp_stride = 0;
  // Frames per high-pass launch.  A high-pass wave keeps the VALU of its SIMD ~35 % busy (nine dependent f64
  // operations per sample) and a frame-kernel launch lasts as long as its slowest wave, so a sub-chunk's high-pass as
  // one 0.3 ms kernel delays the four frame waves that share its SIMD by ~0.08 ms per launch (0.8 ms per 100-frame
  // step, measured with CRISPY_RN_HP=upfront).  As kernels of two frames the 64 waves land on other SIMDs every
  // ~50 us and the delay spreads: 8.17 -> 7.68 ms per step (1 frame: 7.83, 3: 8.07, 4: 8.15, 6: 8.0, whole: 8.17).
  int hp_split = 2;
  // Waves per stream of the frame kernel: 1 = one wave runs the whole frame (every pipe of the chip is busy from ~4 waves per
  // SIMD = 4096 streams up); 3 = the frame's three stages on three waves, a frame apart (rn_frame3_kernel: a stream
  // advances a frame per ~10 k quad-cycles instead of ~26 k -- what counts while there are fewer waves than SIMD slots).
  // Chosen at create time from the stream count; CRISPY_RN_WAVES=1|3 overrides (tests run both forms).
  int waves = 1;
  int hp_ahead = 0;          // > 0: the high-pass runs at most this many sub-chunks in front of the frame kernels
  crispy::EventList ev_fr;   // one per sub-chunk: frame kernel done (only used with hp_ahead)
  bool hp_deep = false;      // the high-pass requests 32 samples ahead (80 registers): set where a wave of it fits beside the frame waves
  bool hp_upfront = false;   // diagnostic (CRISPY_RN_HP=upfront): every high-pass of a call segment first, on the main stream
  // Sub-chunk 0 of a segment of a one-wave handle is filtered by ONE launch of the deep kernel instead of hp_split
  // launches of the 32-register one (crispy_api.cpp, process_device_impl, says what that relies on).
  // CRISPY_RN_HP_FIRST=0 (developer knob) restores the split form.
  bool hp_first_deep = true;
  // Pipeline grain of this handle: frames per frame-kernel launch, and the shorter sub-chunks a segment starts with
  // (crispy_api.cpp: kSubFrames, default_ramp).  Read once at create time; CRISPY_RN_SUB_FRAMES and CRISPY_RN_RAMP
  // (developer knobs) override them per handle, so that one process can time several grains side by side.
  int sub_frames = 0;
  std::vector<int> ramp;
  crispy::DevBuf<float> d_dbg;
  // Host-pointer staging, one set for every entry point that takes host arrays (process, push, pull, app_push, level, drain):
  // each of them synchronises before it returns, so a buffer is only live inside one call.  Scratch (DevBuf::grow).
  crispy::DevBuf<unsigned char> stage_in;    // the call's input rows
  crispy::DevBuf<unsigned char> stage_out;   // the call's output rows
  crispy::DevBuf<float> stage_aux;           // per-frame or per-stream scalars: VAD, level
  int stage_reserve(size_t in_bytes, size_t out_bytes, size_t aux_bytes, const char* who) {
    if (stage_in.grow(in_bytes) != hipSuccess || stage_out.grow(out_bytes) != hipSuccess || stage_aux.grow(aux_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return crispy::fail(CRISPY_ERR_OOM, "%s: staging allocation of %zu + %zu + %zu bytes failed", who, in_bytes, out_bytes, aux_bytes);
    }
    return CRISPY_OK;
  }
  crispy::EventList ev_in, ev_done;          // pipelined host path: per piece
  // timing
  bool timing = false;
  crispy::EventList ev;        // per segment: begin, (frame_begin, frame_end) x sub-chunks, end
  size_t ev_used = 0;
  std::vector<int> seg_subs;   // sub-chunks of every timed segment
  std::unique_ptr<crispy::RnAdapter> ad;     // the capture-rate adapter (crispy_rn_push*): created on first use
  std::unique_ptr<crispy::RnPlayback> pb;    // the playback ring (crispy_rn_pull*): created by crispy_rn_playback_configure
  std::unique_ptr<crispy::RnRecord> rec;     // the recording rings (crispy_rn_record_*): created on first use
  std::unique_ptr<crispy::RnCaptureState> cap;   // the capture callback's state (crispy_rn_capture*): created on first use
  std::unique_ptr<crispy::RnLegacy> lg;      // the Legacy arm and the model switch (crispy_rn_model*): created on first use

  // Every stream the handle created is drained before anything it holds goes.
  ~crispy_rn() {
    (void)hipSetDevice(device);
    for (hipStream_t s : {stream.s, hp_stream.s, h2d_stream.s, d2h_stream.s})
      if (s) (void)hipStreamSynchronize(s);
  }
};

namespace crispy {
// crispy_api.cpp, what rn_io.cpp uses of it: zero the DenoiseState of one stream (>= 0) or all (-1) on the handle's stream;
// enqueue n_frames frames of every stream with explicit element strides of (frame, stream) -- the path of
// crispy_rn_process_device
int rn_zero_state(crispy_rn* h, int stream);
int rn_process_frames_device(crispy_rn* h, const float* d_in, float* d_out, float* d_vad, int n_frames, long stride_t, long stride_b,
                             hipStream_t s);

// rn_io.cpp, what rn_capture_io.cpp uses of it.
// Appending n samples to a ring of cap (audio.rs:280-285, 719-724: the oldest sample is dropped for each one that does not
// fit): how many of the n are skipped at the front, where the first one kept goes, and the ring's position afterwards.
struct AppendPlan {
  long skip = 0;
  int n = 0;
  int tail = 0;
  RingPos after;
};
AppendPlan plan_append(const RingPos& r, int cap, long n);
// The n > 0 samples per stream a call has just written to d_rows [B][stride], appended to ring [B][cap] at pos on s.
int ring_append(float* ring, RingPos& pos, int cap, const float* d_rows, long stride, long n, int B, hipStream_t s);
// LinearResampler::process_sample's position recurrence over n_in samples (see the definition).
long linres_advance(LinResState& st, double step, long n_in, long limit, std::vector<int>* idx, std::vector<float>* t);
constexpr long kPushMaxNew = 1L << 28;      // 48 kHz samples per stream and push (or bypassed capture)
// the handle's adapter, created with the defaults when there is none; of a const handle: the defaults themselves
RnAdapter* adapter_of(crispy_rn* h);
const RnAdapter* adapter_of(const crispy_rn* h);
inline bool recording(const crispy_rn* h) { return h->rec && h->rec->cap > 0; }
// NsState::Legacy: pushes and pulls go through RnLegacy's pointers
inline bool legacy_active(const crispy_rn* h) { return h->lg && h->lg->model != CRISPY_NS_RNNOISE; }
// What a push of n_in samples will do, worked out on the host without touching the handle.
struct PushPlan {
  LinResState rs;      // resampler state behind the push
  long n_new = 0;      // 48 kHz samples the push adds per stream
  int frames = 0;      // frames completed: (carry + n_new) / 480
  int carry_len = 0;   // remainder behind the push
  long n_out = 0;      // samples returned: 480 x (frames, minus the dropped first one)
};
// who: the entry point named in the error message.  idx / t: where a push records its positions; null: count only.
int plan_push(const RnAdapter* a, long n_in, std::vector<int>* idx, std::vector<float>* t, PushPlan* p, const char* who);
// crispy_rn_push_device behind its NULL checks, the handle's device current
int push_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_out, long out_stride, float* d_frames48,
                     long frames_stride, float* d_vad, long* n_out, hipStream_t s, const char* who);
// crispy_rn_record_app_push*: the argument checks, and the enqueue behind them (n_frames > 0, the handle's device current)
int check_app_push(const crispy_rn* h, const float* in, long in_stride, long n_frames, int channels, const char* who);
int app_push_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_frames, int channels, hipStream_t s);
// crispy_rn_level_device behind its checks
int level_device_impl(crispy_rn* h, const float* d_in, long in_stride, long n_in, float* d_rms, hipStream_t s);
// next_sample's recurrence (audio.rs:297-314, the same in SharedAudio: 167-199) over n_frames on copies of the playback
// state: per frame the samples popped since the start and resample_pos as f32 into p->off / p->frac (off < 0: a dry frame).
struct PullPlan {
  long len = 0, pops = 0, live = 0;
  double pos = 0.;
};
PullPlan plan_pull(RnPlayback* p, long n_frames);

// rn_capture_io.cpp, what rn_legacy_io.cpp uses of it: the capture state with the callback resampler's last-sample halves
// allocated (state: they exist before an arm that needs them is entered); CRISPY_ERR_OOM leaves the handle as it was.
int ensure_capture_last(crispy_rn* h, const char* who);
}  // namespace crispy

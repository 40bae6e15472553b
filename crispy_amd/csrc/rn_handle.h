// rn_handle.h -- the RNNoise handle behind `crispy_rn` (include/crispy_hip.h), shared by the translation units that
// implement its entry points: crispy_api.cpp (create / process / reset ...), rn_adapter.hip (crispy_rn_push*) and
// rn_playback.hip (crispy_rn_pull*), rn_record.hip (crispy_rn_record_*, crispy_rn_level*).
#pragma once
#include <cstddef>
#include <vector>

#include "../../include/crispy_hip.h"
#include "rn_common.h"

namespace crispy {
struct RnAdapter;   // rn_adapter.hip
struct RnPlayback;  // rn_playback.hip
struct RnRecord;    // rn_record.hip
}

struct crispy_rn {
  int device = 0;
  int B = 0;
  hipStream_t stream = nullptr;
  hipStream_t hp_stream = nullptr;   // helper stream: the latency-bound high-pass runs beside the frame kernel
  hipEvent_t ev_begin = nullptr;
  std::vector<hipEvent_t> ev_hp;     // one per sub-chunk: high-pass done
  // constants
  crispy::RnTables* d_tab = nullptr;
  uint32_t* d_wpack = nullptr;
  // state
  float* d_hp_mem = nullptr;
  float* d_synth = nullptr;       // overlap-add tails [B][480]
  float* d_ceps = nullptr;
  float* d_lastg = nullptr;
  float* d_rnn = nullptr;
  float* d_last_gain = nullptr;
  int* d_last_period = nullptr;
  int* d_memid = nullptr;
  // workspace
  float* d_xhp = nullptr;
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
  std::vector<hipEvent_t> ev_fr;   // one per sub-chunk: frame kernel done (only used with hp_ahead)
  bool hp_deep = false;      // the high-pass requests 32 samples ahead (80 registers): set where a wave of it fits beside the frame waves
  bool hp_upfront = false;   // diagnostic (CRISPY_RN_HP=upfront): every high-pass of a call segment first, on the main stream
  float* d_dbg = nullptr;
  // host-pointer staging
  float* d_stage_in = nullptr;
  float* d_stage_out = nullptr;
  float* d_stage_vad = nullptr;
  size_t stage_frames = 0;
  // pipelined host path: copy-in / compute / copy-out streams and per-piece events
  hipStream_t h2d_stream = nullptr;
  hipStream_t d2h_stream = nullptr;
  std::vector<hipEvent_t> ev_in, ev_done;
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;  // per segment: begin, (frame_begin, frame_end) x sub-chunks, end
  size_t ev_used = 0;
  std::vector<int> seg_subs;   // sub-chunks of every timed segment
  // the capture-rate adapter (crispy_rn_push*, rn_adapter.hip): created on first use, released through its own hook
  crispy::RnAdapter* ad = nullptr;
  void (*ad_free)(crispy::RnAdapter*) = nullptr;
  // the playback ring (crispy_rn_playback_* / crispy_rn_pull*, rn_playback.hip): created by crispy_rn_playback_configure
  crispy::RnPlayback* pb = nullptr;
  void (*pb_free)(crispy::RnPlayback*) = nullptr;
  // the recording rings (crispy_rn_record_*, rn_record.hip): created on first use, recording from crispy_rn_record_configure on
  crispy::RnRecord* rec = nullptr;
  void (*rec_free)(crispy::RnRecord*) = nullptr;
};

namespace crispy {
// crispy_api.cpp: zero the DenoiseState of one stream (>= 0) or all (-1) on the handle's stream; enqueue n_frames frames of
// every stream with explicit element strides of (frame, stream) -- the path of crispy_rn_process_device
int rn_zero_state(crispy_rn* h, int stream);
int rn_process_frames_device(crispy_rn* h, const float* d_in, float* d_out, float* d_vad, int n_frames, long stride_t, long stride_b,
                             hipStream_t s);
// rn_playback.hip, both no-ops on a handle without playback configured: a new processor at effective input rate in_rate
// (empty ring of in_rate samples, resample_pos 0; the output rate stays); the n samples per stream a push has just written to
// d_rows [B][stride] appended to the ring on s
int rn_playback_adapter_configured(crispy_rn* h, float in_rate, const char* who);
int rn_playback_append(crispy_rn* h, const float* d_rows, long stride, long n, hipStream_t s);
// rn_playback.hip: its append kernel for any ring [B][cap] -- n <= cap samples per stream from src [B][src_stride] to ring
// indices tail, tail + 1, ... modulo cap
hipError_t rn_launch_ring_append(const float* src, long src_stride, float* ring, int cap, int tail, int n, int B, hipStream_t s);
// rn_record.hip, a no-op on a handle that does not record: the n samples per stream a push has just written to d_rows
// [B][stride] appended to the mic ring on s
int rn_record_append_mic(crispy_rn* h, const float* d_rows, long stride, long n, hipStream_t s);
}  // namespace crispy

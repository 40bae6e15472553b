// rn_playback.hip -- crispy_rn_playback_* / crispy_rn_pull*: the playback half of RnnNoiseProcessor for every stream of a
// handle at once.  push_sample appends what it returns to `output_buf`, a deque of at most one second (src-tauri/src/audio.rs:
// 280-285); the output callback reads next_sample() once per output frame (audio.rs:297-314, 610-657), a linear-interpolating
// read at input_rate / output_rate, converts the sample to the device's format and writes it to every channel of the frame.
//   rn_ring_append_kernel   the samples a push returned, copied into the ring [n_streams][cap] at the tail (modulo cap)
//   rn_pull_kernel          per output frame: gather ring[head + offset] and its successor, interpolate (three separately
//                           rounded f32 operations), convert to f32 / i16 / u16, store to `channels` interleaved outputs
// Head, length and resample_pos live on the host: the streams of a handle are pushed and pulled in lock step, so they are the
// same for all of them and do not depend on the samples.  The host runs the reference's f64 recurrence once per pull, frame by
// frame, and uploads one (offset, fraction) pair per output frame.
// Both kernels are streaming passes: lanes run along the samples of one stream, a workgroup covers consecutive ones.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "api_util.h"
#include "rn_common.h"
#include "rn_handle.h"

namespace crispy {
namespace {

constexpr int PB_THREADS = 256;
constexpr int PB_COPY_TILE = PB_THREADS * 4;       // samples per workgroup of the append
constexpr long PB_MAX_BLOCKS = 1L << 23;           // per launch: a handle of several hundred thousand streams goes in turns

struct RnRingAppend {
  const float* src;    // [B][src_stride]: the rows the push has just written, from the first sample that is kept
  long src_stride;
  float* ring;         // [B][cap]
  int cap;
  int tail;            // where the first sample goes, < cap
  int n;               // samples per stream, <= cap
  int B;
};

struct RnPull {
  const float* ring;   // [B][cap]
  int cap;
  int head;            // ring index of output_buf[0] at the start of the pull, < cap
  const int* off;      // [n_frames]: samples popped since the start of the pull (< cap - 1); < 0: an underrun, the frame is 0.0
  const float* frac;   // [n_frames]: resample_pos as f32
  void* out;           // [B][out_stride] elements of the format
  long out_stride;
  unsigned n_frames;
  unsigned n_elems;    // n_frames x channels, <= 2^27
  unsigned channels;
  int B;
};

__host__ __device__ inline long pb_tiles(long n, long tile) { return n > 0 ? (n + tile - 1) / tile : 1; }

// A pure copy: the ring holds exactly the bits the push returned.  A lane's four samples are 256 apart, so that every store
// of a wave covers consecutive addresses wherever the tail stands.
__global__ __launch_bounds__(PB_THREADS) void rn_ring_append_kernel(RnRingAppend a) {
  const unsigned tiles = (unsigned)pb_tiles(a.n, PB_COPY_TILE);
  const long b = blockIdx.x / tiles;
  const int tile0 = (int)(blockIdx.x - (unsigned)b * tiles) * PB_COPY_TILE;
  const float* src = a.src + b * a.src_stride;
  float* ring = a.ring + b * a.cap;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = tile0 + e * PB_THREADS + (int)threadIdx.x;
    if (r < a.n) {
      int i = a.tail + r;          // < 2 x cap
      if (i >= a.cap) i -= a.cap;
      ring[i] = src[r];
    }
  }
}

// s0 + (s1 - s0) * frac with the subtract, the multiply and the add rounded separately, as next_sample's are (Rust never
// contracts).  hipcc fuses a * b + c by default: contraction is switched off here and in the conversions below, and
// tests/test_playback_host.py looks at the ISA.
__device__ __forceinline__ float pull_lerp(float s0, float s1, float frac) {
#pragma clang fp contract(off)
  const float d = s1 - s0;
  const float p = d * frac;
  return s0 + p;
}

__device__ __forceinline__ float pull_sample(const RnPull& a, const float* ring, unsigned f) {
  const int off = a.off[f];
  if (off < 0) return 0.f;
  int i0 = a.head + off;           // < 2 x cap
  if (i0 >= a.cap) i0 -= a.cap;
  const int i1 = i0 + 1 == a.cap ? 0 : i0 + 1;
  return pull_lerp(ring[i0], ring[i1], a.frac[f]);
}

__device__ __forceinline__ float clamp_pm1(float s) { return s < -1.f ? -1.f : (s > 1.f ? 1.f : s); }     // f32::clamp: a NaN stays a NaN

// The output callback's conversions (audio.rs:613-650).  Rust's `as` truncates toward zero and makes a NaN 0.
template <int FMT> struct Pcm;
template <> struct Pcm<CRISPY_PCM_F32> {
  using T = float;
  static __device__ __forceinline__ uint32_t bits(float s) { return __float_as_uint(s); }
  static __device__ __forceinline__ T elem(uint32_t w) { return __uint_as_float(w); }
};
template <> struct Pcm<CRISPY_PCM_I16> {
  using T = int16_t;
  static __device__ __forceinline__ uint32_t bits(float s) {
#pragma clang fp contract(off)
    const float x = clamp_pm1(s) * 32767.f;
    const int q = s != s ? 0 : (int)x;       // |x| <= 32767
    return (uint32_t)q & 0xffffu;
  }
  static __device__ __forceinline__ T elem(uint32_t w) { return (int16_t)(uint16_t)w; }
};
template <> struct Pcm<CRISPY_PCM_U16> {
  using T = uint16_t;
  static __device__ __forceinline__ uint32_t bits(float s) {
#pragma clang fp contract(off)
    const float h = clamp_pm1(s) * 0.5f;
    const float u = h + 0.5f;
    const float x = u * 65535.f;
    const int q = s != s ? 0 : (int)x;       // 0 <= x <= 65535
    return (uint32_t)q;
  }
  static __device__ __forceinline__ T elem(uint32_t w) { return (uint16_t)w; }
};

// A row of `out` is n_frames x channels elements, element e belonging to frame e / channels.
// VEC: every row is 16-byte aligned (pointer and stride): a lane takes the 16 / sizeof(T) consecutive elements of one
// 16-byte store and works out each frame they touch once; the row's last, partial piece goes element by element.
// Otherwise a lane's elements are 256 apart, so that a wave's store still covers consecutive addresses.
template <int FMT, bool VEC>
__global__ __launch_bounds__(PB_THREADS) void rn_pull_kernel(RnPull a) {
  using P = Pcm<FMT>;
  using T = typename P::T;
  constexpr int EPV = 16 / (int)sizeof(T);
  constexpr unsigned TILE = PB_THREADS * EPV;
  const unsigned tiles = (unsigned)pb_tiles(a.n_elems, TILE);
  const long b = blockIdx.x / tiles;
  const unsigned tile0 = (blockIdx.x - (unsigned)b * tiles) * TILE;
  const float* ring = a.ring + b * a.cap;
  T* out = reinterpret_cast<T*>(a.out) + b * a.out_stride;
  if (VEC) {
    const unsigned e0 = tile0 + threadIdx.x * EPV;
    if (e0 >= a.n_elems) return;
    unsigned f = e0 / a.channels;
    unsigned c = e0 - f * a.channels;
    uint32_t cur = P::bits(pull_sample(a, ring, f));
    uint32_t w[EPV];
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
      w[k] = cur;
      if (++c == a.channels) {
        c = 0;
        ++f;
        if (k + 1 < EPV && f < a.n_frames) cur = P::bits(pull_sample(a, ring, f));
      }
    }
    if (e0 + EPV <= a.n_elems) {
      uint4 v;
      if constexpr (EPV == 4) v = make_uint4(w[0], w[1], w[2], w[3]);
      else v = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
      *reinterpret_cast<uint4*>(out + e0) = v;
    } else {
#pragma unroll
      for (int k = 0; k < EPV; ++k)
        if (e0 + k < a.n_elems) out[e0 + k] = P::elem(w[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
      const unsigned e = tile0 + k * PB_THREADS + threadIdx.x;
      if (e < a.n_elems) out[e] = P::elem(P::bits(pull_sample(a, ring, e / a.channels)));
    }
  }
}

hipError_t launch_append(const RnRingAppend& a, hipStream_t s) {
  const long tiles = pb_tiles(a.n, PB_COPY_TILE);
  const long per = PB_MAX_BLOCKS / tiles;              // streams per launch (tiles <= 47 for a cap of one second, <= 2^18 for a recording ring)
  for (long b0 = 0; b0 < a.B; b0 += per) {
    RnRingAppend c = a;
    c.B = (int)(a.B - b0 < per ? a.B - b0 : per);
    c.src += b0 * a.src_stride;
    c.ring += b0 * a.cap;
    hipLaunchKernelGGL(rn_ring_append_kernel, dim3((unsigned)(c.B * tiles)), dim3(PB_THREADS), 0, s, c);
  }
  return hipGetLastError();
}

template <int FMT>
hipError_t launch_pull_fmt(const RnPull& a, hipStream_t s) {
  using T = typename Pcm<FMT>::T;
  const long tiles = pb_tiles(a.n_elems, PB_THREADS * (16 / (long)sizeof(T)));       // <= 2^17
  const long per = PB_MAX_BLOCKS / tiles;
  const bool vec = (((uintptr_t)a.out | (uintptr_t)(a.out_stride * (long)sizeof(T))) & 15) == 0;
  for (long b0 = 0; b0 < a.B; b0 += per) {
    RnPull c = a;
    c.B = (int)(a.B - b0 < per ? a.B - b0 : per);
    c.ring += b0 * a.cap;
    c.out = reinterpret_cast<T*>(a.out) + b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL((rn_pull_kernel<FMT, true>), grid, dim3(PB_THREADS), 0, s, c);
    else hipLaunchKernelGGL((rn_pull_kernel<FMT, false>), grid, dim3(PB_THREADS), 0, s, c);
  }
  return hipGetLastError();
}

hipError_t launch_pull(const RnPull& a, int format, hipStream_t s) {
  switch (format) {
    case CRISPY_PCM_F32: return launch_pull_fmt<CRISPY_PCM_F32>(a, s);
    case CRISPY_PCM_I16: return launch_pull_fmt<CRISPY_PCM_I16>(a, s);
    default: return launch_pull_fmt<CRISPY_PCM_U16>(a, s);
  }
}

constexpr long kPullMaxFrames = 1L << 24;     // output frames per pull
inline size_t pcm_bytes(int format) { return format == CRISPY_PCM_F32 ? 4 : 2; }

}  // namespace

// NsState's playback side (audio.rs:208-212: output_buf, max_output_len, resample_pos, output_rate) for all streams of a
// handle.  Created by crispy_rn_playback_configure; a handle without one has no ring and pushes as before.
struct RnPlayback {
  float out_rate = 48000.f;
  float in_rate = 48000.f;   // effective input rate: 48000 with the input resampler, else the configured capture rate
  int cap = 0;               // max_output_len = in_rate as usize
  int head = 0;              // ring index of output_buf[0]
  int len = 0;               // output_buf.len()
  double pos = 0.;           // resample_pos
  DevBuf<float> ring;        // [B][cap]
  DevBuf<int> d_pos;         // (off[n], frac[n]) of the current pull
  int* h_pos[2] = {nullptr, nullptr};     // pinned upload slots, used in turns; ev_pos: the slot's copy has been read
  long h_pos_cap[2] = {0, 0};
  hipEvent_t ev_pos[2] = {nullptr, nullptr};
  int slot = 0;
  std::vector<int> off;      // host scratch of one pull
  std::vector<float> frac;
  DevBuf<unsigned char> d_hout;   // crispy_rn_pull: device copy of the host array
};

namespace {

// crispy_rn::pb_free (the caller has made the handle's device current and drained its stream)
void playback_free(RnPlayback* p) {
  for (int* q : p->h_pos)
    if (q) (void)hipHostFree(q);
  for (hipEvent_t e : p->ev_pos)
    if (e) (void)hipEventDestroy(e);
  delete p;
}

// A fresh output_buf of one second at in_rate and resample_pos = 0.  The ring is replaced only when its size changes, the new
// one allocated before the old one goes: a failure leaves the handle as it was.
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
  p->head = 0;
  p->len = 0;
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
  RnPlayback* p = h->pb;
  // next_sample (audio.rs:297-314), n_frames times, on copies of the state: the reference's own recurrence, never a closed form
  const double step = (double)p->in_rate / (double)p->out_rate;
  long len = p->len, pops = 0, live = 0;
  double pos = p->pos;
  p->off.resize((size_t)n_frames);
  p->frac.resize((size_t)n_frames);
  for (long f = 0; f < n_frames; ++f) {
    p->off[f] = -1;
    p->frac[f] = 0.f;
    if (len < 2) continue;
    while (pos >= 1.0 && len >= 2) {
      ++pops;
      --len;
      pos -= 1.0;
    }
    if (len < 2) continue;         // ran dry while popping: 0.0, the pops and the decrements stay
    p->off[f] = (int)pops;
    p->frac[f] = (float)pos;
    pos += step;
    ++live;
  }
  // every allocation first: a failure from here on returns with the handle's state as it was
  const size_t words = (size_t)2 * n_frames;
  if (p->d_pos.grow(words * sizeof(int)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: position buffer of %zu bytes failed", who, words * sizeof(int));
  }
  const int slot = p->slot;
  if (p->h_pos_cap[slot] < (long)words) {
    int* fresh = nullptr;
    if (hipHostMalloc(&fresh, words * sizeof(int), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CRISPY_ERR_OOM, "%s: pinned allocation of %zu bytes failed", who, words * sizeof(int));
    }
    if (p->ev_pos[slot]) HIP_TRY(hipEventSynchronize(p->ev_pos[slot]));
    if (p->h_pos[slot]) (void)hipHostFree(p->h_pos[slot]);
    p->h_pos[slot] = fresh;
    p->h_pos_cap[slot] = (long)words;
  }
  if (!p->ev_pos[slot]) HIP_TRY(hipEventCreateWithFlags(&p->ev_pos[slot], hipEventDisableTiming));

  // ---- enqueue ----
  HIP_TRY(hipEventSynchronize(p->ev_pos[slot]));      // the upload that used this slot two pulls ago (no-op before)
  std::memcpy(p->h_pos[slot], p->off.data(), (size_t)n_frames * sizeof(int));
  std::memcpy(p->h_pos[slot] + n_frames, p->frac.data(), (size_t)n_frames * sizeof(float));
  HIP_TRY(hipMemcpyAsync(p->d_pos.p, p->h_pos[slot], words * sizeof(int), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(p->ev_pos[slot], s));
  p->slot = slot ^ 1;
  RnPull a{};
  a.ring = p->ring.p;
  a.cap = p->cap;
  a.head = p->head;
  a.off = p->d_pos.p;
  a.frac = reinterpret_cast<const float*>(p->d_pos.p + n_frames);
  a.out = d_out;
  a.out_stride = out_stride;
  a.n_frames = (unsigned)n_frames;
  a.n_elems = (unsigned)(n_frames * channels);
  a.channels = (unsigned)channels;
  a.B = h->B;
  HIP_TRY(launch_pull(a, format, s));
  p->head = (int)((p->head + pops) % p->cap);
  p->len = (int)len;
  p->pos = pos;
  if (n_live) *n_live = live;
  return CRISPY_OK;
}

}  // namespace

// what rn_record.hip uses of this file (rn_handle.h): the append kernel on a ring of its own
hipError_t rn_launch_ring_append(const float* src, long src_stride, float* ring, int cap, int tail, int n, int B, hipStream_t s) {
  RnRingAppend a{};
  a.src = src;
  a.src_stride = src_stride;
  a.ring = ring;
  a.cap = cap;
  a.tail = tail;
  a.n = n;
  a.B = B;
  return launch_append(a, s);
}

// what rn_adapter.hip uses of this file (rn_handle.h)
int rn_playback_adapter_configured(crispy_rn* h, float in_rate, const char* who) {
  return h->pb ? playback_fresh_ring(h, h->pb, in_rate, who) : CRISPY_OK;
}

int rn_playback_append(crispy_rn* h, const float* d_rows, long stride, long n, hipStream_t s) {
  RnPlayback* p = h->pb;
  if (!p || n <= 0) return CRISPY_OK;
  RnRingAppend a{};
  a.src_stride = stride;
  a.ring = p->ring.p;
  a.cap = p->cap;
  a.B = h->B;
  int head = p->head, len = p->len;
  if (n >= p->cap) {                 // everything that was there is evicted, and the front of this push with it
    a.src = d_rows + (n - p->cap);
    a.n = p->cap;
    a.tail = 0;
    head = 0;
    len = p->cap;
  } else {
    a.src = d_rows;
    a.n = (int)n;
    a.tail = (head + len) % p->cap;
    const long over = len + n - p->cap;      // push_sample pops the oldest sample for each one that does not fit
    if (over > 0) {
      head = (int)((head + over) % p->cap);
      len = p->cap;
    } else {
      len += (int)n;
    }
  }
  HIP_TRY(launch_append(a, s));
  p->head = head;
  p->len = len;
  return CRISPY_OK;
}

}  // namespace crispy

using namespace crispy;

extern "C" {

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
    h->pb = fresh.release();
    h->pb_free = playback_free;
  } else {
    rc = playback_fresh_ring(h, h->pb, in_rate, who);
    if (rc != CRISPY_OK) return rc;
  }
  h->pb->out_rate = output_rate;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_playback_configure")

long crispy_rn_playback_buffered(const crispy_rn* h) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_playback_buffered: NULL handle");
  return h->pb ? h->pb->len : 0;
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
  return pull_device_impl(h, n_frames, channels, format, d_out, out_stride, n_live, hip_stream ? (hipStream_t)hip_stream : h->stream, who);
} CRISPY_CATCH_RET("crispy_rn_pull_device")

int crispy_rn_pull(crispy_rn* h, long n_frames, int channels, int format, void* out, long out_stride, long* n_live) try {
  const char* who = "crispy_rn_pull";
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  int rc = check_pull(h, n_frames, channels, format, out, out_stride, who);
  if (rc != CRISPY_OK) return rc;
  if (n_live) *n_live = 0;
  if (n_frames == 0) return CRISPY_OK;
  HIP_TRY(hipSetDevice(h->device));
  RnPlayback* p = h->pb;
  const size_t row = (size_t)n_frames * channels * pcm_bytes(format);       // a multiple of 16 when it matters: rows stay aligned
  const size_t pitch = (row + 15) & ~(size_t)15;
  if (p->d_hout.grow((size_t)h->B * pitch) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: staging allocation of %zu bytes failed", who, (size_t)h->B * pitch);
  }
  hipStream_t s = h->stream;
  rc = pull_device_impl(h, n_frames, channels, format, p->d_hout.p, (long)(pitch / pcm_bytes(format)), n_live, s, who);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * pcm_bytes(format), p->d_hout.p, pitch, row, (size_t)h->B, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_pull")

}  // extern "C"

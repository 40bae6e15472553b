// rn_adapter.hip -- crispy_rn_push*: what RnnNoiseProcessor::push_sample (src-tauri/src/audio.rs:242-295) does per sample
// around process_frame, for one block of capture samples of every stream of a handle at once.  Kernels and the entry
// points that drive them live together here; the handle itself is rn_handle.h.
//   rn_adapt_in_kernel    LinearResampler (audio.rs:108-133) + frame assembly: carried remainder, then the new 48 kHz samples,
//                         x32768 into the staging rows the high-pass reads; the new remainder into the carry buffer
//   (frame kernels)       the completed frames as one call through crispy_rn_process_device's enqueue path
//   rn_adapt_out_kernel   clamp(y / 32768, -1, 1) x volume (audio.rs:270-273), first frame skipped (audio.rs:275-278)
//   (ring append)         on a handle with playback configured: the returned samples into output_buf (rn_playback.hip);
//                         on a handle that records: into the recording ring as well (rn_record.hip)
// Both kernels are streaming passes: lanes run along the samples of one stream, a workgroup covers 1024 consecutive samples.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "api_util.h"
#include "rn_common.h"
#include "rn_handle.h"

namespace crispy {
namespace {

constexpr int AD_THREADS = 256;
constexpr int AD_TILE = AD_THREADS * 4;   // samples per workgroup: four consecutive ones per lane, one 16-byte store

__host__ __device__ inline long ad_tiles(long n) { return n > 0 ? (n + AD_TILE - 1) / AD_TILE : 1; }

// last + (sample - last) * t with the multiply and the add rounded separately, as the reference's are (Rust never
// contracts).  hipcc fuses a * b + c by default, __fmul_rn / __fadd_rn included (they are plain operators to it), so
// contraction is switched off for these three operations; tests/test_rn_push_host.py looks at the ISA.
__device__ __forceinline__ float lerp_unfused(float last, float cur, float t) {
#pragma clang fp contract(off)
  const float d = cur - last;
  const float p = d * t;
  return last + p;
}

// The position arithmetic of the resampler (f64 recurrence) is done once per push on the host, for all streams; the
// kernel gets (idx, t) per output and does the interpolation, last + (sample - last) * t, as three separately rounded f32
// operations (lerp_unfused).
template <bool RESAMPLE>
__global__ __launch_bounds__(AD_THREADS) void rn_adapt_in_kernel(RnAdaptIn a) {
  const unsigned tiles = (unsigned)ad_tiles((long)a.carry_len + a.n_new);      // <= 2^23: the launcher's limit
  const long b = blockIdx.x / tiles;
  const long q0 = ((long)(blockIdx.x - (unsigned)b * tiles) * AD_THREADS + threadIdx.x) * 4;
  const long total = (long)a.carry_len + a.n_new;
  const long n_frame = (long)a.frames * RN_FRAME;       // samples of the push that complete frames
  const float* in = a.in + b * a.in_stride;
  if (q0 == 0) a.last_new[b] = in[a.n_in - 1];
  if (q0 >= total) return;
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long q = q0 + e;
    float x = 0.f;
    if (q < a.carry_len) {
      x = a.carry_old[b * RN_FRAME + q];
    } else if (q < total) {
      const long r = q - a.carry_len;
      if (RESAMPLE) {
        const int m = a.idx[r];
        const float cur = in[m];
        const float last = m > 0 ? in[m - 1] : a.last_old[b];
        x = lerp_unfused(last, cur, a.t[r]);
      } else {
        x = in[r];
      }
    }
    v[e] = x;
  }
  if (q0 + 4 <= n_frame) {      // n_frame is a multiple of 4: a lane's four samples are all frame samples or none is
    const float4 s4 = make_float4(v[0] * 32768.f, v[1] * 32768.f, v[2] * 32768.f, v[3] * 32768.f);
    *reinterpret_cast<float4*>(a.stage + b * n_frame + q0) = s4;
    if (a.frames48) {
      float* f = a.frames48 + b * a.frames_stride + q0;
      if (((uintptr_t)f & 15) == 0) {
        *reinterpret_cast<float4*>(f) = s4;
      } else {
        f[0] = s4.x; f[1] = s4.y; f[2] = s4.z; f[3] = s4.w;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (q0 + e < total) a.carry_new[b * RN_FRAME + (q0 + e - n_frame)] = v[e];
  }
}

__device__ __forceinline__ float adapt_out_sample(float y, float volume) {
  const float s = y / 32768.f;
  return (s < -1.f ? -1.f : (s > 1.f ? 1.f : s)) * volume;      // f32::clamp: a NaN stays a NaN
}

// VEC: every row of `out` is 16-byte aligned (pointer and stride): one float4 per lane; otherwise a lane stores the four
// samples 256 apart, so that a wave's store still covers consecutive addresses
template <bool VEC>
__global__ __launch_bounds__(AD_THREADS) void rn_adapt_out_kernel(RnAdaptOut a) {
  const unsigned tiles = (unsigned)ad_tiles(a.n_out);
  const long b = blockIdx.x / tiles;
  const long tile0 = (long)(blockIdx.x - (unsigned)b * tiles) * AD_TILE;
  const float* y = a.y + b * a.y_stride + a.skip;
  float* out = a.out + b * a.out_stride;
  if (VEC) {
    const long r = tile0 + threadIdx.x * 4;        // n_out is a multiple of 4
    if (r >= a.n_out) return;
    const float4 y4 = *reinterpret_cast<const float4*>(y + r);
    *reinterpret_cast<float4*>(out + r) = make_float4(adapt_out_sample(y4.x, a.volume), adapt_out_sample(y4.y, a.volume),
                                                      adapt_out_sample(y4.z, a.volume), adapt_out_sample(y4.w, a.volume));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long r = tile0 + e * AD_THREADS + threadIdx.x;
      if (r < a.n_out) out[r] = adapt_out_sample(y[r], a.volume);
    }
  }
}

}  // namespace

// A launch covers at most 2^23 workgroups (the runtime refuses 2^32 work-items per grid dimension and more): a handle of
// several hundred thousand streams is covered in turns of streams, each turn with its own row pointers.
constexpr long AD_MAX_BLOCKS = 1L << 23;

hipError_t rn_launch_adapt_in(const RnAdaptIn& a, hipStream_t s) {
  const long tiles = ad_tiles((long)a.carry_len + a.n_new);
  if (tiles > AD_MAX_BLOCKS) return hipErrorInvalidValue;
  const long per = AD_MAX_BLOCKS / tiles;                  // streams per launch
  for (long b0 = 0; b0 < a.B; b0 += per) {
    RnAdaptIn c = a;
    c.B = (int)(a.B - b0 < per ? a.B - b0 : per);
    c.in += b0 * a.in_stride;
    c.carry_old += b0 * RN_FRAME;
    c.carry_new += b0 * RN_FRAME;
    c.last_old += b0;
    c.last_new += b0;
    c.stage += b0 * a.frames * RN_FRAME;
    if (c.frames48) c.frames48 += b0 * a.frames_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (a.idx) hipLaunchKernelGGL(rn_adapt_in_kernel<true>, grid, dim3(AD_THREADS), 0, s, c);
    else hipLaunchKernelGGL(rn_adapt_in_kernel<false>, grid, dim3(AD_THREADS), 0, s, c);
  }
  return hipGetLastError();
}

hipError_t rn_launch_adapt_out(const RnAdaptOut& a, hipStream_t s) {
  const long tiles = ad_tiles(a.n_out);
  if (tiles > AD_MAX_BLOCKS) return hipErrorInvalidValue;
  const long per = AD_MAX_BLOCKS / tiles;
  const bool vec = (((uintptr_t)a.out | (uintptr_t)(a.out_stride * sizeof(float))) & 15) == 0;
  for (long b0 = 0; b0 < a.B; b0 += per) {
    RnAdaptOut c = a;
    c.B = (int)(a.B - b0 < per ? a.B - b0 : per);
    c.y += b0 * a.y_stride;
    c.out += b0 * a.out_stride;
    const dim3 grid((unsigned)(c.B * tiles));
    if (vec) hipLaunchKernelGGL(rn_adapt_out_kernel<true>, grid, dim3(AD_THREADS), 0, s, c);
    else hipLaunchKernelGGL(rn_adapt_out_kernel<false>, grid, dim3(AD_THREADS), 0, s, c);
  }
  return hipGetLastError();
}


// =============================================================================================
// host side
// =============================================================================================
namespace {

// LinearResampler::process_sample's position arithmetic (audio.rs:108-133), the reference's own f64 recurrence run
// sample by sample -- from the first sample of a stream on, never a closed form, so it is the reference's sequence for
// the whole life of a stream, also past 2^29 outputs where the running sum starts to round.  The positions do not depend
// on the sample values: one run per push serves every stream of a handle.
struct LinResState {
  bool has_last = false;
  double input_pos = 0., next_pos = 0.;
};
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
constexpr long kPushMaxIn = 1L << 24;     // capture samples per stream and push
constexpr long kPushMaxNew = 1L << 28;    // 48 kHz samples per stream and push

}  // namespace

// RnnNoiseProcessor's state around process_frame (audio.rs:202-213) for all streams of a handle, and the adapter's buffers.
// Created with the defaults -- 48 kHz, volume 1 -- when a handle is first pushed to or configured.
struct RnAdapter {
  float rate = 48000.f;     // capture rate as configured; within 1 Hz of 48 kHz: no resampler
  bool resample = false;
  float volume = 1.f;
  bool first = true;        // first_frame
  LinResState rs;           // LinearResampler::has_last / input_pos / next_output_pos (the same for every stream)
  int carry_len = 0;        // input_buf.len(), < 480 between pushes
  int cur = 0;              // which half of the double-buffered per-stream state is current
  float* d_carry = nullptr; // [2][B][480]
  float* d_last = nullptr;  // [2][B]: LinearResampler::last_sample
  float* d_stage = nullptr; // workspace [B][ws_frames * 480]: frames into / out of the frame kernels
  float* d_y = nullptr;
  long ws_frames = 0;
  int* d_pos = nullptr;     // (idx[n], t[n]) of the current push
  size_t pos_cap = 0;
  int* h_pos[2] = {nullptr, nullptr};   // pinned upload slots, used in turns; ev_pos: the slot's copy has been read
  long h_pos_cap[2] = {0, 0};
  hipEvent_t ev_pos[2] = {nullptr, nullptr};
  int slot = 0;
  std::vector<int> idx;     // host scratch of one push
  std::vector<float> t;
  float* d_hin = nullptr;   // crispy_rn_push: device copies of the host arrays
  float* d_hout = nullptr;
  float* d_hvad = nullptr;
  size_t hin_cap = 0, hout_cap = 0, hvad_cap = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // timing: around rn_adapt_in_kernel / rn_adapt_out_kernel
  bool timed = false;
};

namespace {

// crispy_rn::ad_free (the caller has made the handle's device current and drained its stream)
void adapter_free(RnAdapter* a) {
  void* ptrs[] = {a->d_carry, a->d_last, a->d_stage, a->d_y, a->d_pos, a->d_hin, a->d_hout, a->d_hvad};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  for (int* p : a->h_pos)
    if (p) (void)hipHostFree(p);
  for (hipEvent_t e : a->ev_pos)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : a->ev)
    if (e) (void)hipEventDestroy(e);
  delete a;
}

RnAdapter* adapter_of(crispy_rn* h) {
  if (!h->ad) {
    h->ad = new RnAdapter();       // (std::bad_alloc: the entry point's guard makes it CRISPY_ERR_OOM)
    h->ad_free = adapter_free;
  }
  return h->ad;
}
const RnAdapter* adapter_of(const crispy_rn* h) {
  static const RnAdapter fresh;
  return h->ad ? h->ad : &fresh;
}

// What a push of n_in samples will do, worked out on the host without touching the handle.
struct PushPlan {
  LinResState rs;      // resampler state behind the push
  long n_new = 0;      // 48 kHz samples the push adds per stream
  int frames = 0;      // frames completed: (carry + n_new) / 480
  int carry_len = 0;   // remainder behind the push
  long n_out = 0;      // samples returned: 480 x (frames, minus the dropped first one)
};

// who: the entry point named in the error message.  idx / t: where a push records its positions; null: count only.
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

// Grow-only device buffer: the new one is allocated before the old one goes, so a failure leaves the handle as it was.
template <typename T>
int grow(T** buf, size_t* cap, size_t want, const char* who) {
  if (*cap >= want) return CRISPY_OK;
  T* fresh = nullptr;
  if (hipMalloc(&fresh, want * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CRISPY_ERR_OOM, "%s: workspace allocation of %zu bytes failed", who, want * sizeof(T));
  }
  if (*buf) (void)hipFree(*buf);      // (waits for the work that still reads it)
  *buf = fresh;
  *cap = want;
  return CRISPY_OK;
}

int ensure_adapter_state(crispy_rn* h, RnAdapter* a, const char* who) {
  if (a->d_carry && a->d_last) return CRISPY_OK;
  const size_t B = (size_t)h->B;
  float *carry = nullptr, *last = nullptr;
  if (hipMalloc(&carry, 2 * B * RN_FRAME * sizeof(float)) != hipSuccess || hipMalloc(&last, 2 * B * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    if (carry) (void)hipFree(carry);
    return fail(CRISPY_ERR_OOM, "%s: adapter state allocation failed", who);
  }
  a->d_carry = carry;
  a->d_last = last;
  HIP_TRY(hipMemset(carry, 0, 2 * B * RN_FRAME * sizeof(float)));
  HIP_TRY(hipMemset(last, 0, 2 * B * sizeof(float)));
  HIP_TRY(hipDeviceSynchronize());
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
  if (p.frames > a->ws_frames) {
    const size_t want = (size_t)B * n_frame;
    float *stage = nullptr, *y = nullptr;
    if (hipMalloc(&stage, want * sizeof(float)) != hipSuccess || hipMalloc(&y, want * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      if (stage) (void)hipFree(stage);
      return fail(CRISPY_ERR_OOM, "%s: workspace allocation of 2 x %zu bytes failed", who, want * sizeof(float));
    }
    if (a->d_stage) (void)hipFree(a->d_stage);
    if (a->d_y) (void)hipFree(a->d_y);
    a->d_stage = stage;
    a->d_y = y;
    a->ws_frames = p.frames;
  }
  const int slot = a->slot;
  if (a->resample && p.n_new > 0) {
    rc = grow(&a->d_pos, &a->pos_cap, (size_t)2 * p.n_new, who);
    if (rc != CRISPY_OK) return rc;
    if (a->h_pos_cap[slot] < 2 * p.n_new) {
      int* fresh = nullptr;
      if (hipHostMalloc(&fresh, (size_t)2 * p.n_new * sizeof(int), hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(CRISPY_ERR_OOM, "%s: pinned allocation of %zu bytes failed", who, (size_t)2 * p.n_new * sizeof(int));
      }
      if (a->ev_pos[slot]) HIP_TRY(hipEventSynchronize(a->ev_pos[slot]));
      if (a->h_pos[slot]) (void)hipHostFree(a->h_pos[slot]);
      a->h_pos[slot] = fresh;
      a->h_pos_cap[slot] = 2 * p.n_new;
    }
    if (!a->ev_pos[slot]) HIP_TRY(hipEventCreateWithFlags(&a->ev_pos[slot], hipEventDisableTiming));
  }
  if (h->timing)
    for (hipEvent_t& e : a->ev)
      if (!e) HIP_TRY(hipEventCreate(&e));

  // ---- enqueue ----
  RnAdaptIn ai{};
  ai.in = d_in;
  ai.in_stride = in_stride;
  ai.n_in = n_in;
  if (a->resample && p.n_new > 0) {
    HIP_TRY(hipEventSynchronize(a->ev_pos[slot]));      // the upload that used this slot two pushes ago (no-op before)
    std::memcpy(a->h_pos[slot], a->idx.data(), (size_t)p.n_new * sizeof(int));
    std::memcpy(a->h_pos[slot] + p.n_new, a->t.data(), (size_t)p.n_new * sizeof(float));
    HIP_TRY(hipMemcpyAsync(a->d_pos, a->h_pos[slot], (size_t)2 * p.n_new * sizeof(int), hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(a->ev_pos[slot], s));
    a->slot = slot ^ 1;
    ai.idx = a->d_pos;     // (null when the push adds no 48 kHz sample, e.g. the one that primes the resampler)
    ai.t = reinterpret_cast<const float*>(a->d_pos + p.n_new);
  }
  const int cur = a->cur, nxt = cur ^ 1;
  ai.carry_len = a->carry_len;
  ai.n_new = p.n_new;
  ai.frames = p.frames;
  ai.carry_old = a->d_carry + (size_t)cur * B * RN_FRAME;
  ai.carry_new = a->d_carry + (size_t)nxt * B * RN_FRAME;
  ai.last_old = a->d_last + (size_t)cur * B;
  ai.last_new = a->d_last + (size_t)nxt * B;
  ai.stage = a->d_stage;
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
    rc = rn_process_frames_device(h, a->d_stage, a->d_y, d_vad, p.frames, (long)RN_FRAME, n_frame, s);
    if (rc != CRISPY_OK) return rc;
  }
  if (p.n_out > 0) {
    RnAdaptOut ao{};
    ao.y = a->d_y;
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
    if (h->pb) {      // playback configured: what push_sample appends to output_buf (audio.rs:280-285)
      rc = rn_playback_append(h, d_out, out_stride, p.n_out, s);
      if (rc != CRISPY_OK) return rc;
    }
    if (h->rec) {     // recording: what push_mono_to_buffers appends to the recording ring (audio.rs:701-726)
      rc = rn_record_append_mic(h, d_out, out_stride, p.n_out, s);
      if (rc != CRISPY_OK) return rc;
    }
  }
  *n_out = p.n_out;
  return CRISPY_OK;
}

}  // namespace

}  // namespace crispy

using namespace crispy;

extern "C" {

int crispy_rn_adapter_configure(crispy_rn* h, float input_rate, float volume) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_configure: NULL handle");
  if (!(input_rate > 0.f) || !std::isfinite(input_rate))
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_configure: input_rate must be a positive number of Hz");
  if (volume != volume) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_adapter_configure: volume is NaN");
  HIP_TRY(hipSetDevice(h->device));
  const bool resample = std::fabs(input_rate - 48000.f) >= 1.f;
  // the new processor's output_buf and resample_pos, on a handle with playback configured; first, as it may allocate
  int rc = rn_playback_adapter_configured(h, resample ? 48000.f : input_rate, "crispy_rn_adapter_configure");
  if (rc != CRISPY_OK) return rc;
  rc = rn_zero_state(h, -1);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
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
  *rate_hz = a->resample ? 48000.f : a->rate;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_rn_adapter_produced_rate_hz")

long crispy_rn_push_out_len(const crispy_rn* h, long n_in) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_rn_push_out_len: NULL handle");
  PushPlan p;
  const int rc = plan_push(adapter_of(h), n_in, nullptr, nullptr, &p, "crispy_rn_push_out_len");
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
  return push_device_impl(h, d_in, in_stride, n_in, d_out, out_stride, d_frames48, frames_stride, d_vad, n_out,
                          hip_stream ? (hipStream_t)hip_stream : h->stream, "crispy_rn_push_device");
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
  RnAdapter* a = adapter_of(h);
  PushPlan p;
  int rc = plan_push(a, n_in, nullptr, nullptr, &p, who);
  if (rc != CRISPY_OK) return rc;
  if (out_stride < p.n_out) return fail(CRISPY_ERR_INVALID_ARG, "%s: out_stride %ld shorter than the %ld samples of this push", who, out_stride, p.n_out);
  HIP_TRY(hipSetDevice(h->device));
  const size_t B = (size_t)h->B;
  rc = grow(&a->d_hin, &a->hin_cap, B * (size_t)n_in, who);
  if (rc == CRISPY_OK) rc = grow(&a->d_hout, &a->hout_cap, B * (size_t)(p.n_out > 0 ? p.n_out : 1), who);
  if (rc == CRISPY_OK && vad) rc = grow(&a->d_hvad, &a->hvad_cap, B * (size_t)(p.frames > 0 ? p.frames : 1), who);
  if (rc != CRISPY_OK) return rc;
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpy2DAsync(a->d_hin, (size_t)n_in * sizeof(float), in, (size_t)in_stride * sizeof(float), (size_t)n_in * sizeof(float),
                           B, hipMemcpyHostToDevice, s));
  long got = 0;
  rc = push_device_impl(h, a->d_hin, n_in, n_in, a->d_hout, p.n_out, nullptr, 0, vad ? a->d_hvad : nullptr, &got, s, who);
  if (rc != CRISPY_OK) return rc;
  if (got > 0)
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)out_stride * sizeof(float), a->d_hout, (size_t)got * sizeof(float), (size_t)got * sizeof(float),
                             B, hipMemcpyDeviceToHost, s));
  if (vad && p.frames > 0)
    HIP_TRY(hipMemcpyAsync(vad, a->d_hvad, (size_t)p.frames * B * sizeof(float), hipMemcpyDeviceToHost, s));
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

}  // extern "C"

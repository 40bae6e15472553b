// pk_mel_api.cpp -- host side of Parakeet's log-mel front end (include/crispy_hip.h, "Parakeet front end"; kernels in pk_mel.hip):
// the tables (window, twiddles, the built-in Slaney filters, a filter matrix cut to runs), the checks of a call's sample offsets,
// the tile plan, the workspace and the three launches.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "api_util.h"
#include "pk_internal.h"

using crispy::fail;
using namespace crispy::pk;

namespace crispy {
namespace pk {

// Slaney's mel scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 steps per factor 6.4)
static double hz_to_mel(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; }
static double mel_to_hz(double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; }

// M triangles between 0 and 8000 Hz whose corners are equally spaced in mel, each scaled by 2 / (its width in Hz), over the
// 257 bin frequencies k * 8000 / 256: in double, rounded once (the convention of fbank_tables).
void mel_slaney(int M, float* fb) {
  const double lo = hz_to_mel(0.0), hi = hz_to_mel(8000.0), step = (hi - lo) / (double)(M + 1);
  std::vector<double> edge((size_t)M + 2);
  for (int i = 0; i < M + 2; ++i) edge[(size_t)i] = mel_to_hz(i == M + 1 ? hi : lo + (double)i * step);
  for (int m = 0; m < M; ++m) {
    const double left = edge[(size_t)m], center = edge[(size_t)m + 1], right = edge[(size_t)m + 2];
    const double norm = 2.0 / (right - left);
    for (int k = 0; k < kMelSpec; ++k) {
      const double f = (double)k * (8000.0 / (double)(kMelSpec - 1));
      const double down = -(left - f) / (center - left), up = (right - f) / (right - center);
      const double w = std::fmin(down, up) > 0.0 ? std::fmin(down, up) : 0.0;      // never -0
      fb[(size_t)m * kMelSpec + k] = (float)(w * norm);
    }
  }
}

int mel_tables(const char* who, int M, const float* fb, MelTables& t) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < kMelFft; ++k) {
    t.w512[k].x = (float)std::cos(2.0 * pi * k / (double)kMelFft);
    t.w512[k].y = (float)-std::sin(2.0 * pi * k / (double)kMelFft);
  }
  for (int i = 0; i < kMelWin; ++i) t.window[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * i / (double)(kMelWin - 1)));
  for (int i = 0; i < kMelMaxTaps; ++i) t.taps[i] = 0.0f;
  for (int m = 0; m < kMelMaxBins; ++m) t.meta[m] = 0;
  t.pad[0] = t.pad[1] = t.pad[2] = 0;
  long n_taps = 0;
  for (int m = 0; m < M; ++m) {
    const float* row = fb + (size_t)m * kMelSpec;
    int k0 = -1, k1 = -1;
    for (int k = 0; k < kMelSpec; ++k) {
      if (!std::isfinite(row[k])) return fail(CRISPY_ERR_INVALID_ARG, "%s: filter %d has a non-finite weight at bin %d", who, m, k);
      if (row[k] != 0.0f) {
        if (k0 < 0) k0 = k;
        k1 = k;
      }
    }
    const int len = k0 < 0 ? 0 : k1 - k0 + 1;
    if (n_taps + len > kMelMaxTaps)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: the filters' runs hold more than %d taps in all (at filter %d)", who, kMelMaxTaps, m);
    for (int q = 0; q < len; ++q) t.taps[n_taps + q] = row[k0 + q];
    t.meta[m] = (unsigned)(k0 < 0 ? 0 : k0) | ((unsigned)len << 9) | ((unsigned)n_taps << 18);
    n_taps += len;
  }
  t.n_taps = (int)n_taps;
  return CRISPY_OK;
}

int mel_check_offsets(const char* who, const long* sample_offset, int n_clips) {
  if (n_clips < 1 || n_clips > kMaxClips) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_clips %d outside 1 ... %d", who, n_clips, kMaxClips);
  if (!sample_offset) return fail(CRISPY_ERR_INVALID_ARG, "%s: sample_offset is NULL", who);
  if (sample_offset[0] != 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: sample_offset[0] is %ld, not 0", who, sample_offset[0]);
  for (int c = 0; c < n_clips; ++c) {
    const long a = sample_offset[c], b = sample_offset[c + 1];      // a >= 0 here: the difference cannot overflow
    if (b < a) return fail(CRISPY_ERR_INVALID_ARG, "%s: clip %d ends at %ld, before it starts (%ld)", who, c, b, a);
    const long n = b - a;
    if (n < kMelMinSamples) return fail(CRISPY_ERR_INVALID_ARG, "%s: clip %d has %ld samples, fewer than %ld (two rows)", who, c, n, kMelMinSamples);
    if (mel_rows(n) > kMaxRows) return fail(CRISPY_ERR_INVALID_ARG, "%s: clip %d has %ld rows, more than %d", who, c, mel_rows(n), kMaxRows);
  }
  return CRISPY_OK;
}

namespace {

struct MelCarve {      // pieces on 256-byte boundaries; with p == NULL it only adds up the size
  char* p = nullptr;
  size_t used = 0;
  template <class T> T* take(size_t n) {
    T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};

struct MelWork {
  MelClip* clips;
  MelTile* tiles;
  double* part;      // [tiles][3][M]
  float *raw, *stats;
};

void mel_carve(MelCarve& c, MelWork& w, size_t n_clips, size_t n_tiles, size_t rows, size_t M, bool own_raw, bool own_stats) {
  w.clips = c.take<MelClip>(n_clips);
  w.tiles = c.take<MelTile>(n_tiles);
  w.part = c.take<double>(n_tiles * 3 * M);
  w.raw = own_raw ? c.take<float>(rows * M) : nullptr;
  w.stats = own_stats ? c.take<float>(n_clips * 2 * M) : nullptr;
}

// the device copy of the tables for M bins: the caller's matrix if one is set, else the built-in filters
int mel_ensure_tables(crispy_pk* h, const char* who, int M, hipStream_t st) {
  if (h->mel_tab.p && h->mel_tab_bins == M) return CRISPY_OK;
  std::vector<float> own;
  const float* fb = h->mel_fb.data();
  if (h->mel_fb.empty()) {
    own.resize((size_t)M * kMelSpec);
    mel_slaney(M, own.data());
    fb = own.data();
  }
  std::vector<MelTables> t(1);
  const int rc = mel_tables(who, M, fb, t[0]);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(h->mel_tab.grow(sizeof(MelTables)));
  HIP_TRY(hipMemcpyAsync(h->mel_tab.p, t.data(), sizeof(MelTables), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));      // `t` goes with this scope
  h->mel_tab_bins = M;
  return CRISPY_OK;
}

}  // namespace

int mel_enqueue(crispy_pk* h, const char* who, int M, const float* d_pcm, const long* sample_offset, int n_clips, float* d_feats, float* d_raw_tap,
                float* d_stats_tap, hipStream_t st) {
  size_t rows = 0, n_tiles = 0;
  for (int c = 0; c < n_clips; ++c) {
    const size_t r = (size_t)mel_rows(sample_offset[c + 1] - sample_offset[c]);
    rows += r;
    n_tiles += (r + kMelTileFrames - 1) / kMelTileFrames;
  }
  MelCarve size;
  MelWork w{};
  mel_carve(size, w, (size_t)n_clips, n_tiles, rows, (size_t)M, !d_raw_tap, !d_stats_tap);
  if (size.used > h->mel_work.bytes) {      // before any launch: what does not fit is refused with nothing enqueued
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (size.used > free_b + h->mel_work.bytes)
      return fail(CRISPY_ERR_OOM, "%s: the call needs a workspace of %zu bytes, the device has %zu free", who, size.used, free_b + h->mel_work.bytes);
    HIP_TRY(h->mel_work.grow(size.used));
  }
  const int rc = mel_ensure_tables(h, who, M, st);
  if (rc != CRISPY_OK) return rc;
  MelCarve place;
  place.p = h->mel_work.p;
  mel_carve(place, w, (size_t)n_clips, n_tiles, rows, (size_t)M, !d_raw_tap, !d_stats_tap);
  // the clip and tile lists, in one host block that stays until the next call
  const size_t clips_b = (size_t)n_clips * sizeof(MelClip), tiles_b = n_tiles * sizeof(MelTile);
  h->mel_host.assign(clips_b + tiles_b, 0);
  MelClip* hc = reinterpret_cast<MelClip*>(h->mel_host.data());
  MelTile* ht = reinterpret_cast<MelTile*>(h->mel_host.data() + clips_b);
  long row0 = 0;
  int tile = 0;
  for (int c = 0; c < n_clips; ++c) {
    const long n = sample_offset[c + 1] - sample_offset[c];
    MelClip& k = hc[c];
    k.first = sample_offset[c];
    k.row0 = row0;
    k.n = (int)n;
    k.rows = (int)mel_rows(n);
    k.tile0 = tile;
    k.n_tiles = (k.rows + kMelTileFrames - 1) / kMelTileFrames;
    for (int t = 0; t < k.n_tiles; ++t) {
      ht[tile + t].clip = c;
      ht[tile + t].frame0 = t * kMelTileFrames;
    }
    tile += k.n_tiles;
    row0 += k.rows;
  }
  float* raw = d_raw_tap ? d_raw_tap : w.raw;
  float* stats = d_stats_tap ? d_stats_tap : w.stats;
  HIP_TRY(hipMemcpyAsync(w.clips, hc, clips_b, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.tiles, ht, tiles_b, hipMemcpyHostToDevice, st));
  // Developer aid (CRISPY_PK_MEL_TIMELINE in the dev build): device time of the three launches, to stderr; it waits for the call.
  const bool timeline = crispy::dev_env("CRISPY_PK_MEL_TIMELINE") != nullptr;
  crispy::EventList ev;
  if (timeline) HIP_TRY(ev.ensure(4, 0));
  if (timeline) HIP_TRY(hipEventRecord(ev[0], st));
  HIP_TRY(launch_mel_frames(reinterpret_cast<const MelTables*>(h->mel_tab.p), M, d_pcm, w.clips, w.tiles, (int)n_tiles, raw, w.part, st));
  if (timeline) HIP_TRY(hipEventRecord(ev[1], st));
  HIP_TRY(launch_mel_stats(w.clips, n_clips, M, w.part, stats, st));
  if (timeline) HIP_TRY(hipEventRecord(ev[2], st));
  HIP_TRY(launch_mel_normalise(w.clips, w.tiles, (int)n_tiles, M, raw, stats, d_feats, st));
  if (timeline) {
    HIP_TRY(hipEventRecord(ev[3], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms[3] = {0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ev[(size_t)i], ev[(size_t)i + 1]));
    std::fprintf(stderr, "crispy_pk_mel timeline: %zu rows in %zu tiles, frames %.3f ms, statistics %.3f ms, normalise %.3f ms\n", rows, n_tiles, ms[0], ms[1],
                 ms[2]);
  }
  return CRISPY_OK;
}

}  // namespace pk
}  // namespace crispy

namespace {

// what every features call checks before it touches the device
int check_features(const char* who, const crispy_pk* h, int mel_bins, const long* sample_offset, int n_clips) {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (mel_bins < 1 || mel_bins > kMelMaxBins) return fail(CRISPY_ERR_INVALID_ARG, "%s: mel_bins %d outside 1 ... %d", who, mel_bins, kMelMaxBins);
  if (h->weights.p && mel_bins != h->cfg.mel_bins)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: mel_bins %d is not the loaded encoder's (%d)", who, mel_bins, h->cfg.mel_bins);
  if (!h->mel_fb.empty() && mel_bins != h->mel_fb_bins)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: mel_bins %d is not that of the filters set with crispy_pk_set_mel_filters (%d)", who, mel_bins, h->mel_fb_bins);
  return mel_check_offsets(who, sample_offset, n_clips);
}

}  // namespace

extern "C" {

long crispy_pk_feature_rows(long samples) try {
  return mel_rows(samples);
}
CRISPY_CATCH_RET("crispy_pk_feature_rows")

int crispy_pk_mel_filters(int mel_bins, float* fb) try {
  const char* who = "crispy_pk_mel_filters";
  if (mel_bins < 1 || mel_bins > kMelMaxBins) return fail(CRISPY_ERR_INVALID_ARG, "%s: mel_bins %d outside 1 ... %d", who, mel_bins, kMelMaxBins);
  if (!fb) return fail(CRISPY_ERR_INVALID_ARG, "%s: fb is NULL", who);
  mel_slaney(mel_bins, fb);
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_mel_filters")

int crispy_pk_set_mel_filters(void* hv, int mel_bins, const float* fb) try {
  const char* who = "crispy_pk_set_mel_filters";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!fb) {      // back to the built-in filters
    h->mel_fb.clear();
    h->mel_fb_bins = 0;
    h->mel_tab_bins = 0;
    return CRISPY_OK;
  }
  if (mel_bins < 1 || mel_bins > kMelMaxBins) return fail(CRISPY_ERR_INVALID_ARG, "%s: mel_bins %d outside 1 ... %d", who, mel_bins, kMelMaxBins);
  std::vector<MelTables> t(1);      // cut to runs here, so that a matrix that does not fit is refused by this call
  const int rc = mel_tables(who, mel_bins, fb, t[0]);
  if (rc != CRISPY_OK) return rc;
  h->mel_fb.assign(fb, fb + (size_t)mel_bins * kMelSpec);
  h->mel_fb_bins = mel_bins;
  h->mel_tab_bins = 0;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_set_mel_filters")

int crispy_pk_features_device(void* hv, int mel_bins, const float* d_pcm, const long* sample_offset, int n_clips, float* d_feats, float* d_raw_tap,
                              float* d_stats_tap, void* hip_stream) try {
  const char* who = "crispy_pk_features_device";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  const int rc0 = check_features(who, h, mel_bins, sample_offset, n_clips);
  if (rc0 != CRISPY_OK) return rc0;
  if (!d_pcm || !d_feats) return fail(CRISPY_ERR_INVALID_ARG, "%s: d_pcm or d_feats is NULL", who);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream;
  const int rc = mel_enqueue(h, who, mel_bins, d_pcm, sample_offset, n_clips, d_feats, d_raw_tap, d_stats_tap, st);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_features_device")

int crispy_pk_features(void* hv, int mel_bins, const float* pcm, const long* sample_offset, int n_clips, float* feats, float* raw_tap,
                       float* stats_tap) try {
  const char* who = "crispy_pk_features";
  crispy_pk* h = static_cast<crispy_pk*>(hv);
  const int rc0 = check_features(who, h, mel_bins, sample_offset, n_clips);
  if (rc0 != CRISPY_OK) return rc0;
  if (!pcm || !feats) return fail(CRISPY_ERR_INVALID_ARG, "%s: pcm or feats is NULL", who);
  const size_t M = (size_t)mel_bins, n = (size_t)sample_offset[n_clips];
  size_t rows = 0;
  for (int c = 0; c < n_clips; ++c) rows += (size_t)mel_rows(sample_offset[c + 1] - sample_offset[c]);
  auto round = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t pcm_b = round(n * sizeof(float)), rows_b = round(rows * M * sizeof(float)), stats_b = round((size_t)n_clips * 2 * M * sizeof(float));
  const size_t need = pcm_b + rows_b * (raw_tap ? 2 : 1) + (stats_tap ? stats_b : 0);
  HIP_TRY(hipSetDevice(h->device));
  if (need > h->io.bytes) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b + h->io.bytes) return fail(CRISPY_ERR_OOM, "%s: the call's buffers need %zu bytes, the device has %zu free", who, need, free_b + h->io.bytes);
    HIP_TRY(h->io.grow(need));
  }
  char* at = h->io.p;
  float* d_pcm = reinterpret_cast<float*>(at); at += pcm_b;
  float* d_feats = reinterpret_cast<float*>(at); at += rows_b;
  float* d_raw = nullptr; if (raw_tap) { d_raw = reinterpret_cast<float*>(at); at += rows_b; }
  float* d_stats = stats_tap ? reinterpret_cast<float*>(at) : nullptr;
  HIP_TRY(hipMemcpyAsync(d_pcm, pcm, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const int rc = mel_enqueue(h, who, mel_bins, d_pcm, sample_offset, n_clips, d_feats, d_raw, d_stats, h->stream);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(feats, d_feats, rows * M * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (raw_tap) HIP_TRY(hipMemcpyAsync(raw_tap, d_raw, rows * M * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (stats_tap) HIP_TRY(hipMemcpyAsync(stats_tap, d_stats, (size_t)n_clips * 2 * M * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_pk_features")

}  // extern "C"

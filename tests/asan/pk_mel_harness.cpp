// pk_mel_harness.cpp -- TEST INFRASTRUCTURE ONLY.  The device-free host logic of Parakeet's log-mel front end under AddressSanitizer +
// UBSan on the CPU box: pk_mel_api.cpp is compiled HERE, unmodified, against the host-memory HIP stand-in of
// tests/asan/hip/hip_runtime.h; the launchers it calls are the checkers below.  What runs for real: crispy_pk_feature_rows, the
// built-in filters, filter matrices cut to runs from arrays of exactly the stated sizes, the tap cap, the checks of hostile sample
// offsets, the tile plan and the workspace carving (the "kernels" below touch the first and last element of every buffer at the
// size the plan implies), NULL and non-NULL taps, and the limits.  Built and driven by tests/test_pk_mel_sanitizers.py; never linked
// into the product.  Exit status 0 = every case answered as expected; a sanitizer report ends the process.
#include <climits>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "hip/hip_runtime.h"
static size_t shim_free_bytes = (size_t)1 << 30;
static inline hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) { *free_b = *total_b = shim_free_bytes; return hipSuccess; }

#include "../../crispy_amd/csrc/api_util.cpp"
#include "../../crispy_amd/csrc/pk_mel_api.cpp"

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, crispy::last_error_cstr()); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

// what the last call's launches saw
static long seen_tiles = -1, seen_rows = -1, seen_launches = 0;
static int seen_taps = -1;

namespace crispy {
namespace pk {
// The frame "kernel": walks the plan as the real one does and writes the first and last value of every row and partial sum it owns.
hipError_t launch_mel_frames(const MelTables* tab, int M, const float* pcm, const MelClip* clips, const MelTile* tiles, int n_tiles, float* raw,
                             double* part, hipStream_t) {
  ++seen_launches;
  seen_tiles = n_tiles;
  seen_taps = tab->n_taps;
  long rows = 0;
  for (int m = 0; m < M; ++m) {      // every run inside the spectrum and inside the taps
    const unsigned meta = tab->meta[m];
    const int k0 = (int)(meta & 0x1ffu), len = (int)((meta >> 9) & 0x1ffu), off = (int)(meta >> 18);
    EXPECT(k0 + len <= kMelSpec && off + len <= tab->n_taps && tab->n_taps <= kMelMaxTaps);
  }
  for (int t = 0; t < n_tiles; ++t) {
    const MelClip& c = clips[tiles[t].clip];
    EXPECT(tiles[t].frame0 % kMelTileFrames == 0 && tiles[t].frame0 < c.rows && t >= c.tile0 && t < c.tile0 + c.n_tiles);
    const int nf = std::min(kMelTileFrames, c.rows - tiles[t].frame0);
    for (int f = 0; f < nf; ++f) {
      float* r = raw + (c.row0 + tiles[t].frame0 + f) * M;
      r[0] = pcm[c.first] + pcm[c.first + c.n - 1];      // the clip's first and last sample
      r[M - 1] = 0.0f;
      ++rows;
    }
    part[(long)t * 3 * M] = 0.0;
    part[(long)t * 3 * M + 3 * M - 1] = 0.0;
  }
  seen_rows = rows;
  return hipSuccess;
}
hipError_t launch_mel_stats(const MelClip* clips, int n_clips, int M, const double* part, float* stats, hipStream_t) {
  ++seen_launches;
  for (int c = 0; c < n_clips; ++c) {
    stats[(long)c * 2 * M] = (float)part[(long)clips[c].tile0 * 3 * M];
    stats[(long)c * 2 * M + 2 * M - 1] = (float)part[((long)clips[c].tile0 + clips[c].n_tiles) * 3 * M - 1];
  }
  return hipSuccess;
}
hipError_t launch_mel_normalise(const MelClip* clips, const MelTile* tiles, int n_tiles, int M, const float* raw, const float* stats, float* feats,
                                hipStream_t) {
  ++seen_launches;
  for (int t = 0; t < n_tiles; ++t) {
    const MelClip& c = clips[tiles[t].clip];
    const int nf = std::min(kMelTileFrames, c.rows - tiles[t].frame0);
    const long base = (c.row0 + tiles[t].frame0) * M;
    feats[base] = raw[base] + stats[(long)tiles[t].clip * 2 * M];
    feats[base + (long)nf * M - 1] = raw[base + (long)nf * M - 1];
  }
  return hipSuccess;
}
}  // namespace pk
}  // namespace crispy

static void rows_and_filters() {
  EXPECT(crispy_pk_feature_rows(0) == 0 && crispy_pk_feature_rows(319) == 1 && crispy_pk_feature_rows(320) == 2 && crispy_pk_feature_rows(479) == 2);
  EXPECT(crispy_pk_feature_rows(480) == 3 && crispy_pk_feature_rows(6400000) == 40000 && crispy_pk_feature_rows(6400160) == 40001);
  EXPECT(crispy_pk_feature_rows(-1) == 0 && crispy_pk_feature_rows(LONG_MIN) == 0 && crispy_pk_feature_rows(LONG_MAX) == LONG_MAX / 160);
  for (int M : {1, 2, 80, 128}) {
    std::vector<float> fb((size_t)M * 257);      // exactly [M][257]
    EXPECT(crispy_pk_mel_filters(M, fb.data()) == CRISPY_OK);
    crispy::pk::MelTables t;
    EXPECT(crispy::pk::mel_tables("harness", M, fb.data(), t) == CRISPY_OK && t.n_taps > 0 && t.n_taps <= 2 * 257 + M);
  }
  float one = 0.0f;
  EXPECT(crispy_pk_mel_filters(0, &one) == CRISPY_ERR_INVALID_ARG && crispy_pk_mel_filters(129, &one) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_mel_filters(INT_MIN, &one) == CRISPY_ERR_INVALID_ARG && crispy_pk_mel_filters(80, nullptr) == CRISPY_ERR_INVALID_ARG);
}

static void set_filters() {
  void* h = nullptr;
  EXPECT(crispy_pk_create(0, &h) == CRISPY_OK && h);
  // runs at exactly the stated sizes: 15 dense rows and one of 241 weights are 4096 taps, one more is refused
  std::vector<float> fb((size_t)16 * 257, 0.0f);
  for (int m = 0; m < 15; ++m)
    for (int k = 0; k < 257; ++k) fb[(size_t)m * 257 + k] = 1.0f;
  for (int k = 16; k < 257; ++k) fb[(size_t)15 * 257 + k] = 0.5f;      // 241 weights: 3855 + 241 = 4096
  EXPECT(crispy_pk_set_mel_filters(h, 16, fb.data()) == CRISPY_OK);
  fb[(size_t)15 * 257 + 15] = 0.5f;                                     // 4097
  EXPECT(crispy_pk_set_mel_filters(h, 16, fb.data()) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "4096"));
  // a run is first non-zero ... last non-zero: two weights at the ends of the spectrum cost 257 taps
  std::vector<float> ends((size_t)16 * 257, 0.0f);
  for (int m = 0; m < 16; ++m) ends[(size_t)m * 257] = ends[(size_t)m * 257 + 256] = 1.0f;      // 16 x 257 = 4112
  EXPECT(crispy_pk_set_mel_filters(h, 16, ends.data()) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_set_mel_filters(h, 15, ends.data()) == CRISPY_OK);      // 3855
  std::vector<float> zeros((size_t)128 * 257, 0.0f);                       // all-zero filters: runs of length 0
  EXPECT(crispy_pk_set_mel_filters(h, 128, zeros.data()) == CRISPY_OK);
  zeros[5] = NAN;
  EXPECT(crispy_pk_set_mel_filters(h, 128, zeros.data()) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "non-finite"));
  EXPECT(crispy_pk_set_mel_filters(h, 0, zeros.data()) == CRISPY_ERR_INVALID_ARG && crispy_pk_set_mel_filters(h, 129, zeros.data()) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_set_mel_filters(nullptr, 80, zeros.data()) == CRISPY_ERR_INVALID_ARG);
  // the handle still holds the 128 all-zero filters: a call with another width is refused, NULL restores the built-in ones
  const long off[2] = {0, 320};
  std::vector<float> pcm(320, 0.25f), feats((size_t)2 * 128), feats80((size_t)2 * 80);
  EXPECT(crispy_pk_features(h, 80, pcm.data(), off, 1, feats80.data(), nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, 128, pcm.data(), off, 1, feats.data(), nullptr, nullptr) == CRISPY_OK && seen_taps == 0);
  EXPECT(crispy_pk_set_mel_filters(h, 12345, nullptr) == CRISPY_OK);
  EXPECT(crispy_pk_features(h, 80, pcm.data(), off, 1, feats80.data(), nullptr, nullptr) == CRISPY_OK && seen_taps > 0);
  std::mt19937 rng(3);
  for (int i = 0; i < 300; ++i) {      // random sparse matrices: accepted within the cap, refused above it, never a crash
    const int M = 1 + (int)(rng() % 128);
    std::vector<float> r((size_t)M * 257, 0.0f);
    long taps = 0;
    for (int m = 0; m < M; ++m) {
      const int a = (int)(rng() % 257), b = (int)(rng() % 257), k0 = std::min(a, b), k1 = std::max(a, b);
      if (rng() % 8 == 0) continue;
      r[(size_t)m * 257 + k0] = r[(size_t)m * 257 + k1] = 1.0f;
      taps += k1 - k0 + 1;
    }
    EXPECT(crispy_pk_set_mel_filters(h, M, r.data()) == (taps <= 4096 ? CRISPY_OK : CRISPY_ERR_INVALID_ARG));
  }
  crispy_pk_destroy(h);
}

static void plans() {
  void* h = nullptr;
  EXPECT(crispy_pk_create(0, &h) == CRISPY_OK && h);
  const int M = 128;
  // a ragged call at the tile's edges, buffers of exactly the stated sizes, with and without taps
  const long lens[] = {320, 321, 479, 480, 160 * 31, 160 * 32 + 159, 160 * 33, 160 * 64, 160 * 65 + 1};
  const int n = (int)(sizeof(lens) / sizeof(lens[0]));
  std::vector<long> off(1, 0);
  long rows = 0, tiles = 0;
  for (long l : lens) {
    off.push_back(off.back() + l);
    rows += l / 160;
    tiles += (l / 160 + 31) / 32;
  }
  std::vector<float> pcm((size_t)off.back(), 0.5f), feats((size_t)rows * M), raw((size_t)rows * M), stats((size_t)n * 2 * M);
  for (int taps = 0; taps < 4; ++taps) {
    seen_launches = 0;
    EXPECT(crispy_pk_features(h, M, pcm.data(), off.data(), n, feats.data(), (taps & 1) ? raw.data() : nullptr, (taps & 2) ? stats.data() : nullptr) == CRISPY_OK);
    EXPECT(seen_launches == 3 && seen_tiles == tiles && seen_rows == rows);
    EXPECT(crispy_pk_features_device(h, M, pcm.data(), off.data(), n, feats.data(), (taps & 1) ? raw.data() : nullptr, (taps & 2) ? stats.data() : nullptr,
                                     nullptr) == CRISPY_OK);
  }
  // one clip of 40000 rows (the limit) and one row more
  {
    const long big[2] = {0, 6400000 + 159}, over[2] = {0, 6400160};
    std::vector<float> p((size_t)big[1], 0.0f), f((size_t)40000 * M);
    EXPECT(crispy_pk_features(h, M, p.data(), big, 1, f.data(), nullptr, nullptr) == CRISPY_OK && seen_rows == 40000 && seen_tiles == 1250);
    seen_launches = 0;
    EXPECT(crispy_pk_features(h, M, p.data(), over, 1, f.data(), nullptr, nullptr) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "clip 0"));
    EXPECT(seen_launches == 0);
  }
  // hostile offsets: every answer a status that names the clip, nothing launched
  seen_launches = 0;
  float x[4] = {0}, y[4] = {0};
  const long short_clip[3] = {0, 320, 639}, descending[3] = {0, 400, 80}, negative[3] = {0, -320, 0}, not_zero[2] = {1, 400};
  const long huge[3] = {0, LONG_MAX, LONG_MIN}, wrap[2] = {0, LONG_MAX}, first_neg[2] = {LONG_MIN, 0};
  EXPECT(crispy_pk_features(h, M, x, short_clip, 2, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "clip 1"));
  EXPECT(crispy_pk_features(h, M, x, descending, 2, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "clip 1"));
  EXPECT(crispy_pk_features(h, M, x, negative, 2, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "clip 0"));
  EXPECT(crispy_pk_features(h, M, x, not_zero, 1, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, huge, 2, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, wrap, 1, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, first_neg, 1, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, nullptr, 1, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, off.data(), 0, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, off.data(), 4097, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, nullptr, off.data(), n, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, M, x, off.data(), n, nullptr, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, 0, x, off.data(), n, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(h, 129, x, off.data(), n, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features(nullptr, M, x, off.data(), n, y, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_features_device(h, M, x, descending, 2, y, nullptr, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(seen_launches == 0);
  std::mt19937_64 rng(4);
  for (int i = 0; i < 2000; ++i) {      // random offsets, in and out of range: a status, never a crash, never a launch when refused
    long o[5] = {0, 0, 0, 0, 0};
    const int k = 1 + (int)(rng() % 4);
    bool ok = true;
    for (int c = 0; c < k; ++c) {
      const unsigned r = (unsigned)rng();
      const long len = (r & 7) == 0 ? (long)(rng() % 640) - 160 : (r & 7) == 1 ? (long)rng() : 320 + (long)(rng() % 3000);
      o[c + 1] = (long)((unsigned long)o[c] + (unsigned long)len);
      ok = ok && o[c + 1] >= o[c] && o[c + 1] - o[c] >= 320 && (o[c + 1] - o[c]) / 160 <= 40000;
    }
    seen_launches = 0;
    int rc;
    if (ok) {
      long r = 0;
      for (int c = 0; c < k; ++c) r += (o[c + 1] - o[c]) / 160;
      std::vector<float> p((size_t)o[k], 0.0f), f((size_t)r * 80);
      rc = crispy_pk_features(h, 80, p.data(), o, k, f.data(), nullptr, nullptr);
      EXPECT(rc == CRISPY_OK && seen_rows == r);
    } else {
      rc = crispy_pk_features(h, 80, x, o, k, y, nullptr, nullptr);
      EXPECT(rc == CRISPY_ERR_INVALID_ARG && seen_launches == 0);
    }
  }
  // a workspace the device cannot hold is refused before the first launch
  crispy_pk_destroy(h);
  EXPECT(crispy_pk_create(0, &h) == CRISPY_OK && h);
  shim_free_bytes = 1 << 16;
  seen_launches = 0;
  EXPECT(crispy_pk_features_device(h, M, pcm.data(), off.data(), n, feats.data(), nullptr, nullptr, nullptr) == CRISPY_ERR_OOM && seen_launches == 0);
  EXPECT(crispy_pk_features(h, M, pcm.data(), off.data(), n, feats.data(), nullptr, nullptr) == CRISPY_ERR_OOM && seen_launches == 0);
  shim_free_bytes = (size_t)1 << 30;
  EXPECT(crispy_pk_features(h, M, pcm.data(), off.data(), n, feats.data(), nullptr, nullptr) == CRISPY_OK);
  crispy_pk_destroy(h);
}

// crispy_pk_create / crispy_pk_destroy live in pk_api.cpp with the encoder; the harness needs only the handle
extern "C" int crispy_pk_create(int device, void** out) {
  if (!out || device != 0) return CRISPY_ERR_INVALID_ARG;
  crispy_pk* h = new crispy_pk;
  h->device = device;
  (void)hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  *out = h;
  return CRISPY_OK;
}
extern "C" void crispy_pk_destroy(void* h) { delete static_cast<crispy_pk*>(h); }

int main() {
  rows_and_filters();
  set_filters();
  plans();
  std::printf("pk_mel_harness: %d failures\n", failures);
  return failures ? 1 : 0;
}

// diar_front.cpp -- the diarization front end up to the network boundary (include/crispy_hip.h, "Diarization front end"):
// speech segments from the segmentation network's scores (the post-network half of pyannote_get_segments_fixed,
// src-tauri/src/managers/diarization.rs:146-271) on the host, and the host side of the Kaldi fbank the embedding network
// reads (EmbeddingExtractor::compute, :53-75; kernels in diar_fbank.hip).
#include <algorithm>
#include <cmath>
#include <vector>

#include "api_util.h"
#include "diar_internal.h"

using crispy::fail;
using namespace crispy::diar;

namespace {

constexpr int kMaxChunks = 16384;
constexpr long kMaxChunkSamples = 4800000;
constexpr size_t kMaxFeatBytes = (size_t)2 << 30;

long frames_of(long n) { return n < kFbankLen ? 0 : 1 + (n - kFbankLen) / kFbankHop; }

// Rust's `f64 as usize`: truncated, saturating, NaN -> 0 (kept below 2^62 so that sums of two cannot wrap)
size_t as_usize(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 4.611686018427387904e18) return (size_t)1 << 62;
  return (size_t)v;
}

// Everything the two fbank entry points check before a device is touched; fills frame_offset.
int check_fbank_args(const char* who, crispy_diar* h, int pcm_format, const long* first, const long* len, int n_chunks, float scale,
                     long* frame_offset) {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (pcm_format != CRISPY_PCM_I16 && pcm_format != CRISPY_PCM_F32)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: pcm_format %d is neither CRISPY_PCM_I16 nor CRISPY_PCM_F32", who, pcm_format);
  if (n_chunks < 1 || n_chunks > kMaxChunks) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_chunks %d outside 1 ... %d", who, n_chunks, kMaxChunks);
  if (!first || !len || !frame_offset) return fail(CRISPY_ERR_INVALID_ARG, "%s: first, len or frame_offset is NULL", who);
  if (!std::isfinite(scale) || !(scale > 0.0f)) return fail(CRISPY_ERR_INVALID_ARG, "%s: scale %g is not finite and positive", who, (double)scale);
  size_t rows = 0;
  for (int c = 0; c < n_chunks; ++c) {
    if (first[c] < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: first[%d] = %ld < 0", who, c, first[c]);
    if (len[c] < 0 || len[c] > kMaxChunkSamples)
      return fail(CRISPY_ERR_INVALID_ARG, "%s: len[%d] = %ld outside 0 ... %ld", who, c, len[c], kMaxChunkSamples);
    rows += (size_t)frames_of(len[c]);
  }
  if (rows * kFbankBins * sizeof(float) > kMaxFeatBytes)
    return fail(CRISPY_ERR_INVALID_ARG, "%s: %zu rows of features take more than 2 GB", who, rows);
  long at = 0;
  for (int c = 0; c < n_chunks; ++c) {
    frame_offset[c] = at;
    at += frames_of(len[c]);
  }
  frame_offset[n_chunks] = at;
  return CRISPY_OK;
}

// The launches of one call on device pointers; complete on return.  `shift` is subtracted from every first[c] (the host
// form uploads the samples from the smallest first[c] on).
int fbank_device(crispy_diar* h, const void* d_pcm, int pcm_format, const long* first, long shift, int n_chunks, float scale,
                 float* d_feats, float* d_raw, const long* frame_offset, hipStream_t st) {
  if (frame_offset[n_chunks] == 0) return CRISPY_OK;
  if (!h->fbank_tab.p) {
    std::vector<FbankTables> tab(1);
    if (!fbank_tables(tab[0])) return fail(CRISPY_ERR_INTERNAL, "crispy_diar_fbank: the mel filters do not have %d taps", kFbankTaps);
    HIP_TRY(h->fbank_tab.alloc(sizeof(FbankTables)));
    const hipError_t e = hipMemcpy(h->fbank_tab.p, tab.data(), sizeof(FbankTables), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      h->fbank_tab = crispy::DevBuf<char>();      // nothing half-built stays: the next call starts over
      return fail(CRISPY_ERR_HIP, "crispy_diar_fbank: table upload: %s", hipGetErrorString(e));
    }
  }
  std::vector<FbankChunk> chunks((size_t)n_chunks);
  std::vector<FbankTile> tiles;
  for (int c = 0; c < n_chunks; ++c) {
    const int nf = (int)(frame_offset[c + 1] - frame_offset[c]);
    chunks[c] = FbankChunk{first[c] - shift, frame_offset[c], nf, 0};
    for (int f0 = 0; f0 < nf; f0 += kFbankTileFrames) tiles.push_back(FbankTile{c, f0});
  }
  const size_t chunk_bytes = (chunks.size() * sizeof(FbankChunk) + 255) & ~(size_t)255;
  HIP_TRY(h->fbank_descs.grow(chunk_bytes + tiles.size() * sizeof(FbankTile)));
  FbankChunk* d_chunks = h->fbank_descs.as<FbankChunk>();
  FbankTile* d_tiles = reinterpret_cast<FbankTile*>(h->fbank_descs.p + chunk_bytes);
  HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(FbankChunk), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(FbankTile), hipMemcpyHostToDevice, st));
  float* raw = d_raw ? d_raw : d_feats;
  hipError_t e = launch_fbank_frames(h->fbank_tab.as<FbankTables>(), d_pcm, pcm_format, scale, d_chunks, d_tiles, (int)tiles.size(), raw, st);
  if (e == hipSuccess) e = launch_fbank_means(d_chunks, n_chunks, raw, d_feats, st);
  const hipError_t es = hipStreamSynchronize(st);      // the lists above are read until here
  HIP_TRY(e);
  HIP_TRY(es);
  return CRISPY_OK;
}

}  // namespace

extern "C" {

long crispy_diar_fbank_frames(long n_samples) try {
  return frames_of(n_samples);
}
CRISPY_CATCH_RET("crispy_diar_fbank_frames")

long crispy_diar_speech_segments(const float* scores, long n_windows, int n_frames, int n_classes, long n_samples, int sample_rate,
                                 double merge_gap, double* out_start, double* out_end, long* out_first, long* out_len, long cap) try {
  const char* who = "crispy_diar_speech_segments";
  if (sample_rate != 16000) return fail(CRISPY_ERR_INVALID_ARG, "%s: expects 16 kHz mono, got %d Hz", who, sample_rate);
  if (!std::isfinite(merge_gap)) return fail(CRISPY_ERR_INVALID_ARG, "%s: merge_gap is not finite", who);
  if (n_classes < 1 || n_frames < 1) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_frames %d or n_classes %d < 1", who, n_frames, n_classes);
  if (n_windows < 0 || n_samples < 0 || cap < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: negative count", who);
  if (cap > 0 && (!out_start || !out_end || !out_first || !out_len)) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL output with cap > 0", who);
  if (n_samples == 0 || n_windows == 0) return 0;
  if (!scores) return fail(CRISPY_ERR_INVALID_ARG, "%s: scores is NULL", who);
  const size_t total = (size_t)n_samples, window_size = (size_t)sample_rate * 10, frame_step = 270, frame_start = 721;
  struct Span { size_t s, e; };
  std::vector<Span> raw_segments;
  bool current_is_speech = false;
  size_t current_start = 0;
  std::vector<unsigned char> labels((size_t)n_frames), smoothed((size_t)n_frames);
  for (long w = 0; w < n_windows; ++w) {
    const float* win = scores + (size_t)w * n_frames * n_classes;
    // 1. powerset decode: silence (class 0) or speech
    for (int i = 0; i < n_frames; ++i) {
      const float* probs = win + (size_t)i * n_classes;
      float max_val = -INFINITY;
      for (int c = 0; c < n_classes; ++c) max_val = std::fmax(max_val, probs[c]);
      float sum_exp = 0.0f, p_sil = 0.0f;
      for (int c = 0; c < n_classes; ++c) {
        const float e = std::exp(probs[c] - max_val);
        if (c == 0) p_sil = e;
        sum_exp += e;
      }
      p_sil /= sum_exp;
      labels[i] = p_sil > 0.5f ? 0 : 1;
    }
    // 2. the 11-frame median filter, shortened at the window's edges
    for (int i = 0; i < n_frames; ++i) {
      const int a = std::max(i - 5, 0), b = std::min(i + 6, n_frames);
      int count_speech = 0;
      for (int k = a; k < b; ++k) count_speech += labels[k];
      smoothed[i] = count_speech > (b - a) / 2 ? 1 : 0;
    }
    // 3. boundaries, the state carried from window to window
    for (int i = 0; i < n_frames; ++i) {
      const bool is_speech = smoothed[i] == 1;
      if (is_speech == current_is_speech) continue;
      const size_t idx = (size_t)w * window_size + frame_start + (size_t)i * frame_step;
      if (is_speech) {
        current_start = idx < 1600 ? 0 : idx;
      } else {
        const size_t s = std::min(current_start, total), e = std::min(idx, total);
        if (e > s) raw_segments.push_back(Span{s, e});
      }
      current_is_speech = is_speech;
    }
  }
  if (current_is_speech) {
    const size_t s = std::min(current_start, total);
    if (total > s) raw_segments.push_back(Span{s, total});
  }
  // 4. merge, the 1.5 s minimum, the fallback
  std::stable_sort(raw_segments.begin(), raw_segments.end(), [](const Span& a, const Span& b) { return a.s < b.s; });
  const size_t merge_gap_samples = as_usize((double)sample_rate * merge_gap), min_dur = as_usize((double)sample_rate * 1.5);
  std::vector<Span> merged;
  for (const Span& r : raw_segments) {
    if (!merged.empty() && r.s <= merged.back().e + merge_gap_samples) merged.back().e = std::max(merged.back().e, r.e);
    else merged.push_back(r);
  }
  std::vector<Span> out;
  for (const Span& m : merged)
    if (m.e - std::min(m.s, m.e) >= min_dur) out.push_back(m);
  if (out.empty() && !merged.empty()) {
    size_t best = 0;      // max_by_key: the last of equal maxima
    for (size_t i = 1; i < merged.size(); ++i)
      if (merged[i].e - merged[i].s >= merged[best].e - merged[best].s) best = i;
    out.push_back(merged[best]);
  }
  const double rate = (double)sample_rate;
  for (size_t i = 0; i < out.size() && (long)i < cap; ++i) {
    out_start[i] = (double)out[i].s / rate;
    out_end[i] = (double)out[i].e / rate;
    out_first[i] = (long)out[i].s;
    out_len[i] = (long)(out[i].e - out[i].s);
  }
  return (long)out.size();
}
CRISPY_CATCH_RET("crispy_diar_speech_segments")

int crispy_diar_fbank_device(void* hv, const void* d_pcm, int pcm_format, const long* first, const long* len, int n_chunks, float scale,
                             float* d_feats, float* d_raw, long* frame_offset, void* hip_stream) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  const int rc = check_fbank_args("crispy_diar_fbank_device", h, pcm_format, first, len, n_chunks, scale, frame_offset);
  if (rc != CRISPY_OK) return rc;
  if (!d_feats) return CRISPY_OK;      // the sizing call
  if (frame_offset[n_chunks] > 0 && !d_pcm) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_fbank_device: d_pcm is NULL");
  HIP_TRY(hipSetDevice(h->device));
  return fbank_device(h, d_pcm, pcm_format, first, 0, n_chunks, scale, d_feats, d_raw, frame_offset,
                      hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream);
}
CRISPY_CATCH_RET("crispy_diar_fbank_device")

int crispy_diar_fbank(void* hv, const void* pcm, int pcm_format, const long* first, const long* len, int n_chunks, float scale,
                      float* feats, long* frame_offset) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  const int rc = check_fbank_args("crispy_diar_fbank", h, pcm_format, first, len, n_chunks, scale, frame_offset);
  if (rc != CRISPY_OK) return rc;
  if (!feats) return CRISPY_OK;      // the sizing call
  const size_t rows = (size_t)frame_offset[n_chunks];
  if (rows == 0) return CRISPY_OK;
  if (!pcm) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_fbank: pcm is NULL");
  long lo = -1, hi = 0;      // the samples chunks with rows read
  for (int c = 0; c < n_chunks; ++c) {
    if (len[c] < kFbankLen) continue;
    if (lo < 0 || first[c] < lo) lo = first[c];
    hi = std::max(hi, first[c] + len[c]);
  }
  const size_t elem = pcm_format == CRISPY_PCM_F32 ? sizeof(float) : sizeof(short);
  const size_t pcm_bytes = ((size_t)(hi - lo) * elem + 255) & ~(size_t)255, feat_bytes = rows * kFbankBins * sizeof(float);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(h->io.grow(pcm_bytes + feat_bytes));
  float* d_feats = reinterpret_cast<float*>(h->io.p + pcm_bytes);
  HIP_TRY(hipMemcpyAsync(h->io.p, static_cast<const char*>(pcm) + (size_t)lo * elem, (size_t)(hi - lo) * elem, hipMemcpyHostToDevice, h->stream));
  const int rc2 = fbank_device(h, h->io.p, pcm_format, first, lo, n_chunks, scale, d_feats, nullptr, frame_offset, h->stream);
  if (rc2 != CRISPY_OK) return rc2;
  HIP_TRY(hipMemcpyAsync(feats, d_feats, feat_bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_fbank")

}  // extern "C"

// pk_internal.h -- what the host side (pk_api.cpp) and the device side (pk_sub.hip, pk_gemm.hip, pk_gemm_f16.hip, pk_attn.hip, pk_attn_f16.hip) of the Parakeet
// FastConformer encoder share: the handle, the model as the kernels read it and the launch functions; the same for the TDT
// decoder (pk_tdt_api.cpp, pk_tdt.hip) and the log-mel front end (pk_mel_api.cpp, pk_mel.hip).
#pragma once
#include <cstddef>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/crispy_hip.h"
#include "api_util.h"

struct crispy_pk {
  int device = 0;
  hipStream_t stream = nullptr;
  crispy::DevBuf<float> weights;      // the encoder as crispy_pk_load laid it out (PkModel); empty until a load
  crispy_pk_config cfg{};             // of the load
  int precision = 0;                  // crispy_pk_set_precision: 0 f32 operands, 1 f16 operands in every GEMM
  int attn_precision = 0;             // crispy_pk_set_attention_precision: 0 f32 operands, 1 f16 operands in the attention's three products
  crispy::DevBuf<char> weights16;     // mode 1: the GEMM weights packed as f16 (PkHalfModel); empty until the loaded handle is first in mode 1
  crispy::DevBuf<char> scratch;       // a call's workspace, grown on demand and kept
  crispy::DevBuf<char> io;            // host-form features, frames and taps
  // the log-mel front end (pk_mel_api.cpp); usable before a load
  std::vector<float> mel_fb;          // the caller's filter matrix [mel_fb_bins][257] (crispy_pk_set_mel_filters); empty: the built-in filters
  int mel_fb_bins = 0;
  crispy::DevBuf<char> mel_tab;       // MelTables for mel_tab_bins bins; 0: to be built by the next call
  int mel_tab_bins = 0;
  crispy::DevBuf<char> mel_work;      // a features call's clip and tile lists, raw rows, partial sums and statistics
  std::vector<char> mel_host;         // what the call copies to the device: it outlives the call's enqueued copies
  crispy::DevBuf<char> chain;         // crispy_pk_transcribe: the feature rows and the encoder's frames
  crispy::EventList chain_ev;         // "the frames are written", for the decoder's stream
  ~crispy_pk() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct crispy_pk_tdt {
  int device = 0;
  hipStream_t stream = nullptr;
  crispy::DevBuf<float> weights;      // the decoder as crispy_pk_tdt_load laid it out (TdtModel); empty until a load
  crispy_pk_tdt_config cfg{};         // of the load
  crispy::DevBuf<char> scratch;       // a call's workspace, grown on demand and kept
  crispy::DevBuf<char> io;            // host-form frames, steps and taps
  ~crispy_pk_tdt() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace crispy {
namespace pk {

constexpr int kHeadDim = 128;
constexpr int kMaxFrames = 5000;                       // T' of kMaxRows rows: the longest clip an attention pass takes
constexpr int kMaxRows = 40000, kMaxClips = 4096;      // T' <= 5000, the model's max_position_embeddings
constexpr int kMaxTaps = 31, kMaxSubCh = 512;
constexpr double kEps = 1e-5;                          // LayerNorm and BatchNorm
constexpr int kAttnQ = 32, kAttnK = 32;                // query and key tile of the attention kernel
constexpr int kAttnF16Q = 128, kAttnF16K = CRISPY_PK_ATTN_KEY_TILE;      // the same of attention mode 1 (pk_attn_f16.hip)
constexpr int kSubNF = 8;                              // frequencies of one workgroup of the fused depthwise + pointwise kernel

inline long sub_len(long n) { return n < 1 ? 0 : (n - 1) / 2 + 1; }
inline long frames(long rows) { return sub_len(sub_len(sub_len(rows))); }

// Where each tensor sits in the handle's device copy, as the kernels read it.  Every linear weight is [in][out] (the output
// contiguous); absent biases are zeros.  qkv is q, k and v side by side [H][3H]; pointwise_conv1 has its 2H outputs reordered
// in groups of 64 columns: 32 value channels, then their 32 gate channels, so that a GEMM lane holds both halves of a GLU.
// The depthwise weights are [tap][channel]; its bias and the BatchNorm are one (scale, shift) pair folded in double.
struct PkLayer {
  const float *ln_g[5], *ln_b[5];      // norm_feed_forward1, norm_self_att, norm_conv, norm_feed_forward2, norm_out
  const float *ff_w1[2], *ff_b1[2], *ff_w2[2], *ff_b2[2];
  const float *qkv_w, *qkv_b, *o_w, *o_b, *r_w, *bias_u, *bias_v;
  const float *pw1_w, *pw1_b, *dw_w, *dw_scale, *dw_shift, *pw2_w, *pw2_b;
};
struct PkModel {
  const float *conv0_w, *conv0_b;               // [9][C], [C]
  const float *dw_w[2], *dw_b[2];               // [9][C], [C]
  const float *pw_w[2], *pw_b[2];               // [C][C], [C]
  const float *lin_w, *lin_b;                   // [C * M / 8][H], [H]
  const float* inv_freq;                        // [H / 2]
  std::vector<PkLayer> layer;
};
// Mode 1's copies of the GEMM weights: each the f32 matrix of the same name rounded to f16 in the operand order of
// pk_gemm_f16.hip ([N / 32][K / 16][64 lanes][8]); all NULL in mode 0.
struct PkHalfLayer {
  const void *ff_w1[2], *ff_w2[2], *qkv_w, *o_w, *r_w, *pw1_w, *pw2_w;
};
struct PkHalfModel {
  const void* lin_w = nullptr;
  std::vector<PkHalfLayer> layer;
};
// pointwise_conv1's column of output channel o (0 ... 2H - 1): groups of 64 columns hold 32 value channels, then their gates
__host__ __device__ inline size_t glu_column(size_t o, size_t H) {
  const bool gate = o >= H;
  const size_t ch = gate ? o - H : o;
  return (ch / 32) * 64 + (gate ? 32 : 0) + ch % 32;
}
// A call's clips: clip c has feature rows off[0][c] ... off[0][c + 1] and off[s] likewise after s stride-2 convolutions
// (device memory, n_clips + 1 each); max_len[s] is the longest clip's count at stage s.
struct PkTables {
  const int* off[4];
  int n_clips, max_len[4];
};

// feats [rows][M] -> relu(Conv2d(1, C, 3, stride 2, pad 1)) as [T1][M / 2][C]
hipError_t launch_sub_conv0(const PkModel& m, const PkTables& t, const float* d_feats, int M, int C, float* d_out, hipStream_t st);
// stage s (1, 2): in [T_s][F][C] -> relu(pointwise(depthwise stride 2)) as [T_s+1][F / 2][C]; `flat`: as [T_s+1][C * (F / 2)], c * (F / 2) + f
hipError_t launch_sub_dwpw(int s, const PkModel& m, const PkTables& t, const float* d_in, int F, int C, float* d_out, bool flat, hipStream_t st);
// out = LayerNorm(in) * g + b over rows of H; in == out is allowed
hipError_t launch_layernorm(const float* d_in, const float* g, const float* b, float* d_out, long rows, int H, hipStream_t st);
// C [M][N] = epilogue(A [M][K] . Bt [K][N] + bias) on the f32 matrix instruction, k ascending in chains of 64 that are added in order.
// kGemmScale: (v) * alpha; kGemmSilu: silu(v); kGemmResidual: res + alpha * v (res == C allowed); kGemmGlu: N outputs from 2N
// columns in pointwise_conv1's order, value * sigmoid(gate).  K a multiple of 32, the column count of 128; bias nullable.
enum GemmEpilogue { kGemmScale, kGemmSilu, kGemmResidual, kGemmGlu };
hipError_t launch_gemm(GemmEpilogue e, const float* d_a, int K, const float* d_bt, const float* bias, int N, float alpha, const float* d_res,
                       float* d_c, long M, hipStream_t st);
// The encoder's form, by the handle's precision mode (crispy_pk_set_precision).  0: the call above.  1: the same product with both
// operands rounded once to f16, from the packed image d_bp of Bt (launch_pack_f16) on the f16 matrix instruction: one f32
// accumulator per element over k ascending in steps of 16.
hipError_t launch_gemm(int mode, GemmEpilogue e, const float* d_a, int K, const float* d_bt, const void* d_bp, const float* bias, int N, float alpha,
                       const float* d_res, float* d_c, long M, hipStream_t st);
// pk_gemm_f16.hip: mode 1's kernel behind launch_gemm; Bt [K][cols] f32 -> its packed f16 image of K * cols * 2 bytes; and the
// state dict's [cols][K] -> Bt [K][cols] (glu: in pointwise_conv1's column order) for crispy_pk_stage_gemm_device
hipError_t launch_gemm_f16(GemmEpilogue e, const float* d_a, int K, const void* d_bp, const float* bias, int N, float alpha, const float* d_res,
                           float* d_c, long M, hipStream_t st);
hipError_t launch_pack_f16(const float* d_bt, int K, int cols, void* d_out, hipStream_t st);
hipError_t launch_weight_transpose(const float* d_w, int K, int cols, bool glu, float* d_bt, hipStream_t st);
// pos [2 * tmax - 1][H]: row p is d = p - (tmax - 1); sin in the even columns, cos in the odd ones
hipError_t launch_pos_table(const float* inv_freq, int tmax, int H, float* d_pos, hipStream_t st);
// soft-max((q + u) k^T + (q + v) r_{i - j}^T) / sqrt(128)) v per clip and head; qkv [T'][3H], r [2 * tmax - 1][H] -> out [T'][H]
hipError_t launch_attention(const PkLayer& l, const PkTables& t, const float* d_qkv, const float* d_r, int tmax, int heads, float* d_out, hipStream_t st);
// The encoder's form, by the handle's attention mode (crispy_pk_set_attention_precision).  0: the call above.  1: the same with q + u,
// q + v, k, r, v and the soft-max weights rounded once to f16 on the f16 matrix instruction, f32 sums, the soft-max in key tiles of
// CRISPY_PK_ATTN_KEY_TILE (pk_attn_f16.hip: launch_attention_f16).
hipError_t launch_attention(int mode, const PkLayer& l, const PkTables& t, const float* d_qkv, const float* d_r, int tmax, int heads, float* d_out,
                            hipStream_t st);
hipError_t launch_attention_f16(const PkLayer& l, const PkTables& t, const float* d_qkv, const float* d_r, int tmax, int heads, float* d_out, hipStream_t st);
// silu(scale * depthwise K-tap convolution + shift), zero-padded at each clip's own edges; [T'][H] -> [T'][H]
hipError_t launch_dwconv(const PkLayer& l, const PkTables& t, const float* d_in, int H, int K, float* d_out, hipStream_t st);

// ---- the TDT decoder (pk_tdt.hip, pk_tdt_api.cpp) -----------------------------------------------------------------------
constexpr int kTdtRows = 16;         // clips of one workgroup of the skinny products
constexpr int kTdtCols = 64;         // output columns of one workgroup
constexpr int kTdtKBlock = 128;      // k of one LDS block: 32 for each of the four waves; D is a multiple of it
constexpr int kTdtMaxFrames = 5000, kTdtMaxVocab = 65536, kTdtMaxWidth = 2048, kTdtMaxLayers = 8, kTdtMaxDurations = 8, kTdtMaxSymbols = 64;
constexpr int kTdtGroup = 32;        // steps enqueued between two reads of the finished-clips counter

inline long tdt_max_steps(int max_symbols, long frames) { return frames < 1 ? 0 : (long)max_symbols * frames - 1; }

// The decoder as the kernels read it.  Every matrix is [in][out].  An LSTM layer is one matrix [2D][4D]: rows 0 ... D - 1 are
// W_ih, rows D ... 2D - 1 W_hh, and column 4 j + q is gate q (i, f, g, o) of unit j, so that one workgroup's 64 columns are 16
// whole units; its bias is b_ih + b_hh in the same column order.  The head is padded with zero columns to a multiple of 64.
struct TdtModel {
  const float *proj_w, *proj_b;                              // [H][D], [D]
  const float* emb;                                          // [V][D]
  const float *lstm_w[kTdtMaxLayers], *lstm_b[kTdtMaxLayers];
  const float *dp_w, *dp_b;                                  // [D][D], [D]
  const float *head_w, *head_b;                              // [D][n_pad], [n_pad]
  int D, L, V, n_dur, blank, n_pad, dur[kTdtMaxDurations];
};
// A call's clips and everything a step decides, all in device memory.
struct TdtState {
  int n_clips, tiles;            // tiles = n_pad / 64
  const int* off;                // [n + 1] first frame of each clip
  const long* step_off;          // [n + 1] first row of each clip in steps / logits_tap: the running sum of the budgets
  int *t, *tok, *run, *budget, *done, *finished;      // per clip: frame pointer, next input token, "run the prediction network", steps left, finished; one counter
  float *h, *c, *hn;             // [L][n][D]: the LSTM state and a layer's new h until the next launch commits it
  float* g;                      // [n][D] decoder_projector's output
  const float* p;                // [sum T'][D]
  float* part_val;               // [n][tiles] the largest token logit of a column tile ...
  int* part_idx;                 // ... and its column
  float* dur_logit;              // [n][8]
  int *steps, *n_steps;          // the caller's [sum budget][3] and [n]
  float* logits_tap;             // the caller's [sum budget][V + n_dur] or NULL
};

// t = 0, token = blank, (h, c) = 0, n_steps = 0; clips without a budget are finished from the start
hipError_t launch_tdt_init(const TdtModel& m, const TdtState& s, hipStream_t st);
// the prediction network on the clips whose run flag is set: one launch per LSTM layer and one for decoder_projector
hipError_t launch_tdt_predict(const TdtModel& m, const TdtState& s, hipStream_t st);
// logits = head(relu(p[t] + g)) for the unfinished clips; the tap, the duration logits and each column tile's token winner
hipError_t launch_tdt_joint(const TdtModel& m, const TdtState& s, hipStream_t st);
// per clip: the arg-max in index order, the duration rule, the step log, t, the next token and the flags
hipError_t launch_tdt_advance(const TdtModel& m, const TdtState& s, hipStream_t st);

// ---- the log-mel front end (pk_mel.hip, pk_mel_api.cpp) ------------------------------------------------------------------
constexpr int kMelFft = 512, kMelWin = 400, kMelHop = 160, kMelSpec = kMelFft / 2 + 1;
constexpr int kMelMaxBins = 128, kMelMaxTaps = 4096;
constexpr long kMelMinSamples = 2 * kMelHop;      // two rows: the standard deviation divides by rows - 1
constexpr int kMelWaveFrames = 8;                 // consecutive frames one wave transforms
constexpr int kMelTileFrames = 32;                // frames of one workgroup (4 waves)

inline long mel_rows(long samples) { return samples < 0 ? 0 : samples / kMelHop; }

// What the frame kernel copies into LDS once per workgroup (the first n_taps of taps only).  Filter m is one run of weights
// over the power bins [k0, k0 + len): meta[m] = k0 | len << 9 | (offset into taps) << 18.
struct MelTables {
  float2 w512[kMelFft];            // exp(-2 pi i k / 512)
  float window[kMelWin];           // symmetric Hann
  unsigned meta[kMelMaxBins];
  int n_taps, pad[3];
  float taps[kMelMaxTaps];
};
// Clip c of a call: where its samples start in the PCM buffer and how many, where its rows start and how many, its tiles.
struct MelClip {
  long first, row0;
  int n, rows, tile0, n_tiles;
};
// One workgroup's frames: up to kMelTileFrames from frame0 of clip.
struct MelTile {
  int clip, frame0;
};

// host, no device: window and twiddles in double rounded once; `fb` [M][257] cut to runs.  CRISPY_OK, or CRISPY_ERR_INVALID_ARG
// (with the message set) for a non-finite weight or more than kMelMaxTaps taps in all.
int mel_tables(const char* who, int M, const float* fb, MelTables& t);
// host, no device: the built-in Slaney filters [M][257] (Slaney scale and norm, 0 ... 8000 Hz), in double rounded once
void mel_slaney(int M, float* fb);
// checks a call's sample_offset: CRISPY_OK, or CRISPY_ERR_INVALID_ARG naming the clip
int mel_check_offsets(const char* who, const long* sample_offset, int n_clips);
// The front end on n_clips clips; the arguments have been checked.  Enqueues on st and does not wait.
int mel_enqueue(crispy_pk* h, const char* who, int M, const float* d_pcm, const long* sample_offset, int n_clips, float* d_feats, float* d_raw_tap,
                float* d_stats_tap, hipStream_t st);

// raw rows [rows][M] of every tile's frames and, per (tile, bin), part [tile][3][M]: the tile's first value p, the sums of
// (v - p) and (v - p)^2 over its frames in frame order, in double
hipError_t launch_mel_frames(const MelTables* d_tab, int M, const float* d_pcm, const MelClip* d_clips, const MelTile* d_tiles, int n_tiles,
                             float* d_raw, double* d_part, hipStream_t st);
// stats [clip][2][M]: mean and standard deviation (divisor rows - 1) from the clip's tiles in tile order, rounded once to f32
hipError_t launch_mel_stats(const MelClip* d_clips, int n_clips, int M, const double* d_part, float* d_stats, hipStream_t st);
// feats = (raw - mean) / (std + 1e-5f)
hipError_t launch_mel_normalise(const MelClip* d_clips, const MelTile* d_tiles, int n_tiles, int M, const float* d_raw, const float* d_stats,
                                float* d_feats, hipStream_t st);

}  // namespace pk
}  // namespace crispy

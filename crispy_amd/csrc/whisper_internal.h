// whisper_internal.h -- what the four translation units of the Whisper engine share (not part of the ABI):
//   whisper_api.cpp    the model container: tensors, derived copies, precision modes, encoder, workspaces
//   ggml_load.cpp      whisper.cpp GGML model files: reader, de-quantiser, resident block bookkeeping
//   decode_steps.cpp   the decoder: its workspace (DecWs), the start of a pass (DecodePass), the step forms (fused / matrix-vector /
//                      skinny), prompts, captured steps, the greedy / timestamp-rule / beam passes over one window
//   whisper_full.cpp   whisper_full on top of them: seek loop, temperature ladder, segments, results, the recording chunker
//   whisper_align.hip  word-level timestamps: the alignment pass, its kernels, crispy_asr_{align,dtw}_device (reached from
//                      whisper_full.cpp through a hook that file installs: not linked, a dtw request is unsupported)
//   whisper_conf.hip   confidence: the log-probability of a target per logits row, the language soft-max (launchers in
//                      asr_common.h; the host side is conf_* / detect_language in decode_steps.cpp)
// Device memory: every buffer of the handle is a DevBuf member (api_util.h) -- the tensors, the resident blocks (a QTensor reads
// through `d`, which is its own blocks or a dense Tensor's floats), the copies derived from them (crispy_asr::derived, made by
// derived_copy in whisper_api.cpp and summed by crispy_asr_memory_info), the token masks (upload_mask), the de-quantisation slot,
// the workspaces EncWs / DecWs / AlignWs.  crispy_asr_free drops the captured steps, which hold workspace addresses, and deletes
// the handle; nothing is freed by name.
// Reference surface: transcribe_rs::whisper_cpp::WhisperEngine::{load, transcribe} (src-tauri/src/managers/transcription.rs:138-141,
// 183-185).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "../../include/crispy_hip.h"
#include "api_util.h"
#include "asr_common.h"
#include "asr_quant.h"

namespace crispy {
namespace asr {

struct Tensor {
  DevBuf<float> d;
  size_t n = 0;
  bool set = false;
};

// A 2-D tensor kept in HBM as the model file holds it (ggml blocks, asr_quant.h; ttype QT_F32: a dense f32 tensor of a
// mixed file) and a row-wise concatenation of up to three of them (q | k | v, k | v): `crispy_asr_load_resident`.
struct QTensor {
  DevBuf<unsigned char> own;            // the blocks; holds nothing where d aliases a dense Tensor of the handle
  const unsigned char* d = nullptr;     // what the kernels read
  int ttype = 0;
  size_t n = 0;          // elements
  int cols = 0;          // innermost dimension (K)
  size_t nbytes = 0;
};
struct QRef {
  const QTensor* t[3] = {nullptr, nullptr, nullptr};
  int n = 0;
  size_t elems() const { size_t e = 0; for (int i = 0; i < n; ++i) e += t[i]->n; return e; }
};

struct EncLayer {
  QRef r_qkv, r_out, r_fc1, r_fc2;           // resident model: the weights as quantised blocks
  const void *qkv_wh = nullptr, *out_wh = nullptr, *fc1_wh = nullptr, *fc2_wh = nullptr;   // f16 copies (precision mode 1)
  const float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};
struct DecLayer {
  QRef r_qkv, r_out, r_xq, r_xkv, r_xout, r_fc1, r_fc2;
  const float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b;
  const float *lnx_w, *lnx_b, *xq_w, *xq_b, *xkv_w, *xkv_b, *xout_w, *xout_b;
  const void* xkv_wh = nullptr;              // f16 copy of the fused cross K|V projection (precision mode 1)
  const void *out_wh = nullptr, *xout_wh = nullptr, *fc2_wh = nullptr;   // f16 copies of the plain (no LayerNorm in front) decode projections
  const void *qkv_wh = nullptr, *xq_wh = nullptr, *fc1_wh = nullptr;     // f16 copies of the un-folded q | k | v, cross-q, fc1 (precision modes 1 / 2)
  const void *qkv_p = nullptr, *out_p = nullptr, *fc1_p = nullptr, *fc2_p = nullptr;   // ... packed for the fused step kernels (fused_pack_weights)
  const float *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
  // LayerNorm folded into the consuming projection (decode steps with <= 64 clips): gamma-scaled weights, their row
  // sums and beta.W + bias (GemmArgs::ln_s / ln_c)
  const float *qkv_lw, *qkv_ls, *qkv_lc, *xq_lw, *xq_ls, *xq_lc, *fc1_lw, *fc1_ls, *fc1_lc;
};

// Word alignment (whisper_align.hip): while an alignment prefill runs (`on`), layer_cross_and_mlp copies the cross-q rows
// of every layer that holds an alignment head into q [slot][clip][row][n_text_state] -- the rows that layer's own
// cross-attention reads.  Buffers grow on demand and live as long as the handle.
struct AlignWs {
  DevBuf<float> q;
  DevBuf<void> ws;                             // row statistics, matrix, DTW outputs, per-clip arguments
  std::vector<int> slot;                       // [n_text_layer]: the layer's slot in q, -1 = none
  int rows = 0;                                // token rows per clip of the running pass
  bool on = false;
};

// Confidence (whisper_conf.hip): while a teacher-forced prefill runs with `on`, prompt_step projects ALL rows of every step
// onto the vocabulary (into `logits`, rows of their own: h->dw.logits holds one row per clip) and tok_logprob_f32 reads the
// log-probability of the next token off every row.  `logits` is made the first time confidence is asked for, never otherwise.
struct ConfWs {
  DevBuf<float> logits;                        // [SKINNY_MAX_M][logits_ld]
  DevBuf<int> target;                          // [clips][rows] id the row predicts (-1: none)
  DevBuf<float> logp;                          // [clips][rows]
  DevBuf<float> lang;                          // [clips][n_lang] language distribution of a detection step
  int rows = 0;                                // token rows per clip of the running pass
  bool on = false;
};

// The encoder workspace (reserve_enc / reserve_pcm: sizes), grown on demand.
struct EncWs {
  int cap_batch = 0;                         // clips the workspace holds
  long cap_pcm_stride = 0;                   // samples per PCM row
  DevBuf<float> melt, pcm, h1, x, xn, qkv, att, h, enc;
};

// The decoder workspace (reserve_dec: sizes; [cap_rows] = one entry per row the workspace holds).  Captured steps hold these
// addresses: free_dec_ws drops them before it lets the buffers go.
struct DecWs {
  int cap_rows = 0, cap_xclips = 0;          // rows / audio clips the workspace holds
  DevBuf<float> xkv, selfkv, dx, dxn, dq, datt, dh, logits, best;
  DevBuf<int> tok;
  DevBuf<int> tokens_all;
  DevBuf<int> counters;                      // [0] position, [1] generation step (device-side, advanced in-graph)
  // timestamp-mode decoding (whisper.cpp no_timestamps = false)
  DevBuf<TsState> ts_state;                  // [cap_rows]
  DevBuf<int> tids_all;                      // [n_text_ctx][cap_rows]
  DevBuf<int> done_count;
  DevBuf<int> finished;                      // [cap_rows] plain greedy decoding: clip has produced its EOT
  DevBuf<void> xkv_h;                        // f16 copy of the cross K|V (precision mode 1)
  DevBuf<float> plog_all;                    // [n_text_ctx][cap_rows] log-probability of every pick
  DevBuf<float> nosp;                        // [cap_rows] no_speech_prob of the window
  DevBuf<double> u_all;                      // [n_text_ctx][cap_rows] uniform variates of a sampling pass (drawn on the host)
  DevBuf<float> ts_x;                        // [cap_rows][TS_SCRATCH_ROW] the sampling pick's filtered rows
  DevBuf<float> temperature;                 // device scalar
  DevBuf<int> row_off;                       // [cap_rows] left padding of every clip's prompt (cache rows)
  DevBuf<int> beam_parent;                   // [cap_rows]
  DevBuf<BeamRow> beam_row;                  // [cap_rows] a decoder's bookkeeping (beam_advance_kernel)
  DevBuf<int> beam_cand;                     // [3][cap_rows][TS_MAX_CAND] the candidates of a step: ids, timestamp ids, log-probabilities
  DevBuf<int> beam_rec_parent;               // [n_text_ctx][cap_rows] the row a step's sequence came from
  DevBuf<float> fx[3];                       // fused step: residual stream after the self / cross / MLP input sums [rows][dt]
  DevBuf<float> fpart[3];                    // fused step: partial rows of the self / cross out-projection [heads][rows][dt], MLP [dt / 32][rows][dt]
  DevBuf<float> gvpart;                      // gemv step (catalog widths): partial soft-maxes of the cross-attention [GEMV_MAX_M][heads][XA_PARTS][XA_PART_FLOATS]
  // beam search, grown with the pass (decode_beam)
  DevBuf<void> beam_kv;                      // the rows' cache bytes in flight between parents and children
  DevBuf<double> beam_u;                     // [max_new][rows][n_cand] the variates of a beam pass
};

}  // namespace asr
}  // namespace crispy

struct crispy_asr {
  int device = 0;
  crispy_asr_hparams hp{};
  // The effective audio context (crispy_asr_set_audio_ctx; whisper.cpp's whisper_full_params.audio_ctx [UPSTREAM-RECALL]):
  // encoder rows and cross-attention keys per clip of every call, 1 ... hp.n_audio_ctx.  `hp` stays the model's: the
  // workspaces are sized by it, and the leading dimension of the alignment outputs is hp.n_audio_ctx whatever this says.
  // Everything laid out by it (encoder output [clip][audio_ctx][d], cross K | V [layer][clip][K|V][head][audio_ctx][64])
  // is rebuilt by every call from this value; the captured steps bake it in and are dropped by the setter.
  int audio_ctx = 0;
  hipStream_t stream = nullptr;
  crispy_mel* mel = nullptr;
  std::map<std::string, crispy::asr::Tensor> tensors;   // as named by the model file
  std::vector<crispy::DevBuf<void>> derived;   // fused / reordered / f16 / packed copies owned by the handle (derived_copy)
  // resident quantised model (crispy_asr_load_resident): 2-D tensors stay as ggml blocks, de-quantised into ONE scratch
  // slot right in front of the kernel that consumes them (same stream: the consumer has finished before the next fill)
  bool resident = false;
  std::map<std::string, crispy::asr::QTensor> qtensors;
  crispy::DevBuf<void> q_scratch;
  hipEvent_t ev_scratch = nullptr;           // orders a caller's stream against the handle's around the scratch slot
  const crispy::asr::QTensor* q_tok_emb = nullptr;
  bool finalized = false;
  // resolved pointers
  const float *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr, *conv2_b = nullptr, *enc_pos = nullptr;
  const float *ln_post_w = nullptr, *ln_post_b = nullptr;
  const void* tok_emb_hp = nullptr;          // token embedding as f16 in MFMA operand order (precision mode 1: logits)
  const void* conv2_wh = nullptr;            // f16 copy of the reordered conv2 kernel (precision mode 1)
  const void* conv1_wh = nullptr;            // f16 conv1 kernel, rows zero-padded to conv1_kp columns
  int conv1_kp = 0;
  int enc_precision = 0;                     // 0: f32 operands (default), 1: f16 operands for the encoder GEMMs
  // precision modes 1 and 2: the decoder's LayerNorm output rounded to f16 in front of q | k | v, cross q and fc1 (f16 weights) --
  // ggml's mul_mat arithmetic for these products too [UPSTREAM-RECALL].  (Rounds 2 - 4 kept them in f32 in mode 1, with the
  // LayerNorm folded into an f32 GEMM; since round 5 a generated token runs through the fused step kernels of
  // whisper_dec_fused.hip, which multiply f16 LayerNorm outputs, and the staged path follows so that a position's
  // arithmetic does not depend on which path computed it.)
  bool dec_ln16 = false;
  bool dec_attn16 = false;                   // precision mode 2: + the query and the normalised probabilities rounded to f16 inside every attention
  bool ln16_ready = false;
  bool fused_path = true;                    // generated tokens through the fused step kernels when the model allows (CRISPY_ASR_DECODE=stages: never)
  bool half_ready = false;                   // every f16 weight copy of mode 1 exists (set after the last one and a stream sync)
  int xcd_swizzle = 1;                       // mode 1 GEMMs: column tiles of a row tile on one XCD (CRISPY_ASR_XCD=0 turns it off)
  std::vector<crispy::asr::EncLayer> enc;
  const float *tok_emb = nullptr, *dec_pos = nullptr, *dec_ln_w = nullptr, *dec_ln_b = nullptr;
  std::vector<crispy::asr::DecLayer> dec;
  // token masks [n_vocab] (upload_mask)
  crispy::DevBuf<unsigned char> d_suppress;        // tokens never emitted by the greedy decoder
  crispy::DevBuf<unsigned char> d_suppress_first;  // additionally suppressed at the first sampled position
  crispy::DevBuf<unsigned char> d_lang_mask;       // everything but the language tokens (auto-detection)
  crispy::asr::EncWs ew;                     // encoder workspace
  crispy::asr::DecWs dw;                     // decoder workspace
  // timestamp-mode decoding (whisper.cpp no_timestamps = false)
  crispy::DevBuf<unsigned char> d_ts_mask;         // whisper.cpp's always-suppressed specials
  crispy::DevBuf<unsigned char> d_ts_mask_first;   // ... plus suppress_blank (" " and EOT) at the first position
  crispy::DevBuf<unsigned char> d_ts_mask_nst;     // the two masks with whisper.cpp's non-speech tokens added (opts.suppress_nst; built on first use)
  crispy::DevBuf<unsigned char> d_ts_mask_first_nst;
  std::vector<int> prompt_past;              // conditioning text the last single-chunk call ended with (opts.carry_context)
  // captured window-decode steps by what is baked into them: key class, kind of pick (greedy / sampling: different kernels),
  // rows, rows per clip, rules and mask.  A transcribe call alternates between several of them -- the greedy pass over all
  // clips, sampling passes over the failed ones x best_of, windows with and without the text so far -- and with one
  // slot per class every switch re-captured the step (1 - 2 ms each).
  struct TsKey {
    int kc, sampling, rows, xgroup, rules;     // sampling: 0 greedy pick under the timestamp rules, 1 sampling pick, 2 plain arg-max (no timestamps)
    const unsigned char* mask;
    int steps;                                 // generated tokens per replay
    bool operator<(const TsKey& o) const {
      if (steps != o.steps) return steps < o.steps;
      if (kc != o.kc) return kc < o.kc;
      if (sampling != o.sampling) return sampling < o.sampling;
      if (rows != o.rows) return rows < o.rows;
      if (xgroup != o.xgroup) return xgroup < o.xgroup;
      if (rules != o.rules) return rules < o.rules;
      return mask < o.mask;
    }
  };
  std::map<TsKey, hipGraphExec_t> ts_graphs;
  void drop_graphs() {
    for (auto& kv : ts_graphs)
      if (kv.second) (void)hipGraphExecDestroy(kv.second);
    ts_graphs.clear();
  }
  int eot = 50257;
  std::vector<unsigned char> sup_all, sup_first;   // host copies of the two suppression lists
  std::vector<std::string> vocab;                  // token byte strings of a loaded model file
  crispy::asr::AlignWs align;                      // word alignment (opts.dtw_token_timestamps)
  crispy::asr::ConfWs conf;                        // token / language probabilities
  bool confidence = false;                         // crispy_asr_set_confidence: transcribe calls collect them
};

namespace crispy {
namespace asr {

// ---- whisper_api.cpp ----
std::map<std::string, size_t> expected_tensors(const crispy_asr_hparams& hp);
// dense copy of a (row-concatenated) resident tensor in the handle's scratch slot, enqueued on `s` right in front of its consumer
int dq(crispy_asr* h, const QRef& r, bool f16, const float* gamma, hipStream_t s, const void** out);
void free_dec_ws(crispy_asr* h);
// uploads a host byte vector [n_vocab] into one of the handle's token masks, allocating it on first use
int upload_mask(DevBuf<unsigned char>& mask, const std::vector<unsigned char>& host);
// the widths the kernels are built for: tiny, base, small, medium, large
inline bool whisper_width_ok(int d) { return d == 384 || d == 512 || d == 768 || d == 1024 || d == 1280; }
int reserve_enc(crispy_asr* h, int batch);
int reserve_pcm(crispy_asr* h, long stride);
GemmArgs gemm(const float* A, long lda, const float* W, long ldw, float* C, long ldc, const float* bias, int M, int N, int K);

// ---- decode_steps.cpp ----
long logits_ld(const crispy_asr* h);
int reserve_dec(crispy_asr* h, int batch, int xclips = 0);
bool gemv_ref_ok(const QRef& r);
// rows of one group of fallback passes (whole clips x best_of); a grouping choice only -- every row's bits are those of
// its clip decoded alone.  The widest step the decode kernels take (SKINNY_MAX_M): a row costs less in a wide step (2.3 us at
// 512 rows against 2.6 at 128, Whisper-tiny), and 64 clips x best_of 5 are one group instead of three.
constexpr int kLadderRowsMax = 512;
struct Special {
  int sot, lang0, n_lang, n_lang_slots, translate, transcribe, solm, prev, nosp, not_, beg;
  bool multilingual;
};
Special vocab_specials(int n_vocab);
Special special_tokens(const crispy_asr* h);
int decode_ts(crispy_asr* h, const float* d_enc, int batch, const std::vector<std::vector<int>>& prompts, int rules,
              const int* seek, const int* seek_end, int max_new, const unsigned char* mask, const unsigned char* mask_first,
              float temperature, const double* u, int* tokens_out, int* tids_out, float* plog_out, float* nosp_out,
              int* n_out, int xgroup = 1);
double canonical(std::mt19937& g);
int decode_beam(crispy_asr* h, const float* d_enc, int n_clips, int n_dec, int n_cand, const std::vector<std::vector<int>>& clip_prompts,
                int rules, const int* seek, const int* seek_end, int max_new, const unsigned char* mask, const unsigned char* mask_first,
                float temperature, const std::vector<std::mt19937*>& rng, int* tokens_out, int* tids_out, float* plog_out,
                float* nosp_out, int* n_out);

// What a decode call fixes for all of its steps.  begin_pass makes it and every step function takes it: which kernel form
// runs, whether the self K|V cache holds halves or floats and how many key slots an attention gets follow from the call
// in hand, never from what an earlier call left on the handle.
struct DecodePass {
  int rows = 0;                    // sequences, each with a self K|V cache of its own
  int xgroup = 1;                  // rows per audio clip: the best-of / beam decoders of a clip are rows of their own over ONE cross K|V
  int max_keys = 0;                // positions the call can reach (prompt + new tokens)
  const int* row_off = nullptr;    // [rows] left padding of every row's prompt (cache rows); null: none
};
struct PassStart {
  DecodePass pass;
  std::vector<int> tok_mat;        // [rows][n_rows] the prompts right-aligned, token 0 in front of the shorter ones
  int n_rows = 0;                  // the longest prompt
};
// Begins a pass over one prompt per row: checks the tokens and lengths (`who` names the pass in a message: "decode:"),
// left-pads, reserves the workspace, reads the decode-path knob and -- row_offsets -- uploads the padding per row and waits
// for it.  max_keys = fixed_keys, or (0) the longest prompt + max_new.
int begin_pass(crispy_asr* h, const char* who, const std::vector<std::vector<int>>& prompts, int xgroup, int max_new, int fixed_keys,
               bool row_offsets, PassStart* out);
int prefill(crispy_asr* h, const DecodePass& pass, const float* d_enc, const int* tok_mat, int n_rows, hipStream_t s, int* pos_out);
// whisper_lang_auto_detect for `batch` clips: the most probable language token per clip and -- probs_out non-null -- the
// soft-max over the language tokens, host [batch][n_lang]
int detect_language(crispy_asr* h, const char* who, const float* d_enc, int batch, int* lang_tokens_out, float* probs_out);
// Teacher-forced token log-probabilities: conf_begin readies the workspace for a prefill over tok_mat [batch][n_rows] (begin_pass's
// right-aligned rows; row_len[b] = clip b's own rows) and switches the collection on -- every row then predicts the id after
// it, but the rows before n_sot, the last one and the padding; conf_end switches it off (always call it) and conf_read copies
// the numbers out: logp[b][i] = log p(row n_sot + 1 + i of clip b), i < row_len[b] - n_sot - 2.  Needs batch <= SKINNY_MAX_M.
int conf_begin(crispy_asr* h, const int* tok_mat, int batch, int n_rows, const int* row_len, int n_sot, hipStream_t s);
void conf_end(crispy_asr* h);
int conf_read(crispy_asr* h, int batch, int n_rows, const int* row_len, int n_sot, hipStream_t s, std::vector<std::vector<float>>* logp);
// The two launchers of whisper_conf.hip (asr_common.h: tok_logprob_f32, lang_probs_f32), reached through a table that file
// installs at static initialisation, as whisper_align.hip installs g_align_round: the host translation units call no launcher
// of it by name, and where the file is not part of the build asking for these numbers is CRISPY_ERR_UNSUPPORTED.
struct ConfKernels {
  hipError_t (*tok_logprob)(const float* logits, long ld, int n_cols, const int* target, float* logp, int ld_t, int P, int pos,
                            int rows, hipStream_t s);
  hipError_t (*lang_probs)(const float* logits, long ld, int lang0, int n_lang, float* probs, int rows, hipStream_t s);
};
extern const ConfKernels* g_conf_kernels;

// ---- whisper_full.cpp ----
int build_ts_masks(crispy_asr* h);
// Word alignment of one round of the seek loop: rows[c] = clip c's token rows (sot sequence of n_sot ids, <|notimestamps|>,
// text tokens, <|endoftext|>), d_enc = the clips' encoder outputs in order, n_frames[c] = mel frames of its window;
// time_idx[c] receives the warping path's entry column of every row after the sot sequence but the last (10 ms x 2 each);
// logp[c] (nullable) the teacher-forced log-probability of every text token of the clip, from the same pass.
// Installed by whisper_align.hip at static initialisation; null where that file is not part of the build.
using AlignRoundFn = int (*)(crispy_asr* h, const float* d_enc, const std::vector<std::vector<int>>& rows, int n_sot,
                             const std::vector<int>& n_frames, const std::vector<int>& heads, std::vector<std::vector<int>>& time_idx,
                             std::vector<std::vector<float>>* logp);
extern AlignRoundFn g_align_round;
// what the DTW kernel takes: its trace at 2 bits per cell, the last two anti-diagonals and the row entries share the LDS
constexpr int kAlignDtwMaxRows = 512, kAlignDtwMaxCols = 4096, kAlignDtwMaxTraceWords = 35000;
inline bool align_dtw_fits(int rows, int cols) {
  return rows >= 1 && rows <= kAlignDtwMaxRows && cols >= 1 && cols <= kAlignDtwMaxCols &&
         (long)rows * ((cols + 15) / 16) <= kAlignDtwMaxTraceWords;
}

}  // namespace asr
}  // namespace crispy

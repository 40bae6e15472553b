// diar_internal.h -- what the host side (diar_api.cpp, diar_front.cpp, diar_seg_api.cpp, diar_emb_api.cpp) and the device side
// (diar_kernels.hip, diar_fbank.hip, diar_seg.hip, diar_emb.hip) of the speaker clustering, its front end and the two networks
// share: the handle, the descriptors the kernels read from device memory and the launch functions.
#pragma once
#include <algorithm>
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/crispy_hip.h"
#include "api_util.h"
#include "diar_jacobi.h"

struct crispy_diar {
  int device = 0;
  hipStream_t stream = nullptr;
  crispy::DevBuf<char> scratch;      // the turn's matrices, grown on demand and kept
  crispy::DevBuf<char> io;           // host-form embeddings and labels; host-form PCM and feature rows
  crispy::DevBuf<char> descs;        // the solver's counter, the non-finite flag (first 256 bytes), EigDesc and ClusterDesc lists
  crispy::DevBuf<char> infos;        // crispy_diar_info of a call's recordings
  crispy::DevBuf<char> fbank_tab;    // FbankTables, built with the first fbank call
  crispy::DevBuf<char> fbank_descs;  // FbankChunk and FbankTile lists of a call
  crispy::DevBuf<float> seg_weights; // the segmentation network as crispy_diar_seg_load laid it out (SegModel); empty until a load
  crispy::DevBuf<float> emb_weights; // the embedding network as crispy_diar_emb_load laid it out (EmbModel); empty until a load
  int emb_dim = 0;                   // its embedding width; 0 until a load
  crispy::DevBuf<char> emb_tab;      // the row, position and segment offsets of a call's chunks, turn by turn
  ~crispy_diar() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace crispy {
namespace diar {

constexpr size_t kScratchCap = (size_t)2000 << 20;      // a turn's scratch, below the 2 GB the header states

// Pieces of the handle's scratch, each on a 256-byte boundary; with p == NULL it only adds up the size.
struct Carve {
  char* p = nullptr;
  size_t used = 0;
  template <class T> T* take(size_t n) {
    T* r = p ? reinterpret_cast<T*>(p + used) : nullptr;
    used += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};

// One matrix of a solve.  A [n][n] is worked on in place (its diagonal ends up holding the eigenvalues, unsorted);
// V [n][n] accumulates the rotations (NULL: values only); cs [3 * rr_pairs(n)] is the global form's rotation list (c, s, t);
// evals [n] and evecs [n][n] (NULL with V) receive the sorted result.  active: 1 being swept, 2 in its last sweep, 0 done (global form);
// status: 1 until the convergence test has passed.
struct EigDesc {
  float* A;
  float* V;
  float* cs;
  float* evals;
  float* evecs;
  int n;
  int active;
  int status;
  int pad;
};

// One recording of a cluster call.
struct ClusterDesc {
  const float* evals;   // [p_max][n] of the sweep
  const float* evecs;   // [n][n] at p*
  float* pts;           // [n][kmax] spectral rows
  float* centers;       // [kmax][kmax]
  int* labels;          // [n], device
  int n, kmax, p_max, index;
};

hipError_t launch_affinity(const float* d_emb, int n, int dim, float* d_aff, hipStream_t st);
hipError_t launch_nonfinite(const float* d_x, size_t count, int* d_flag, hipStream_t st);
hipError_t launch_rank(const float* d_aff, int n, unsigned short* d_rank, unsigned short* d_sym, hipStream_t st);
// `count` Laplacians for p = p0 ... p0 + count - 1
hipError_t launch_laplacians(const float* d_aff, const unsigned short* d_sym, int n, int p0, int count,
                             float* d_dinv, float* d_lap, hipStream_t st);
hipError_t launch_eig_init(EigDesc* d_descs, int count, hipStream_t st);
hipError_t launch_eig_lds(EigDesc* d_descs, int count, hipStream_t st);
hipError_t launch_eig_norm(EigDesc* d_descs, int count, int* d_n_active, hipStream_t st);
hipError_t launch_eig_step(EigDesc* d_descs, int count, int max_n, bool vectors, int t, hipStream_t st);
hipError_t launch_eig_sort(EigDesc* d_descs, int count, hipStream_t st);
hipError_t launch_decide(const ClusterDesc* d_recs, int count, crispy_diar_info* d_infos, hipStream_t st);
hipError_t launch_kmeans(const ClusterDesc* d_recs, int count, const crispy_diar_info* d_infos, hipStream_t st);

// ---- Kaldi fbank (diar_fbank.hip) -----------------------------------------------------------------------------------
constexpr int kFbankBins = 80, kFbankLen = 400, kFbankHop = 160, kFbankFft = 512;
constexpr int kFbankTaps = 501;          // non-zero filter weights of the 80 triangles over FFT bins 0 ... 255
constexpr int kFbankWaveFrames = 8;      // consecutive frames one wave transforms
constexpr int kFbankTileFrames = 32;     // frames of one workgroup (4 waves)

// What the frame kernel copies into LDS once per workgroup.
struct FbankTables {
  float2 w512[512];          // exp(-2 pi i k / 512)
  float window[kFbankLen];   // Povey
  float taps[kFbankTaps + 3];
  int meta[kFbankBins];      // first FFT bin | taps << 8 | offset into taps << 16
};
// Chunk c of a call: where its samples start in the PCM buffer, where its rows start, how many rows.
struct FbankChunk {
  long first;
  long row0;
  int n_frames;
  int pad;
};
// One workgroup's frames: kFbankTileFrames from frame0 of chunk.
struct FbankTile {
  int chunk;
  int frame0;
};

bool fbank_tables(FbankTables& t);      // host; false if the filters do not have kFbankTaps taps
// raw rows [rows][80] of every tile's frames (before the mean subtraction)
hipError_t launch_fbank_frames(const FbankTables* d_tab, const void* d_pcm, int pcm_format, float scale, const FbankChunk* d_chunks,
                               const FbankTile* d_tiles, int n_tiles, float* d_raw, hipStream_t st);
// feats = raw - column mean over the chunk's frames (in place where d_feats == d_raw)
hipError_t launch_fbank_means(const FbankChunk* d_chunks, int n_chunks, const float* d_raw, float* d_feats, hipStream_t st);

// ---- segmentation network (diar_seg.hip) ----------------------------------------------------------------------------
constexpr int kSegWindow = 160000, kSegMinLen = 991, kSegClasses = 7;
constexpr int kSegTaps0 = 251, kSegStride0 = 10, kSegC0 = 80, kSegC1 = 60, kSegTaps = 5;
constexpr int kSegHidden = 128, kSegLayers = 4, kSegGates = 4 * kSegHidden;

// Positions after each stage for a window of len samples (integer division throughout); frames is p2.
struct SegShape {
  int c0, p0, c1, p1, c2, frames;
};
inline SegShape seg_shape(long len) {
  SegShape s{0, 0, 0, 0, 0, 0};
  if (len < kSegMinLen) return s;
  s.c0 = (int)((len - kSegTaps0) / kSegStride0 + 1);
  s.p0 = s.c0 / 3;
  s.c1 = s.p0 - (kSegTaps - 1);
  s.p1 = s.c1 / 3;
  s.c2 = s.p1 - (kSegTaps - 1);
  s.frames = s.c2 / 3;
  return s;
}

// Where each tensor sits in the handle's device copy, as the kernels read it (offsets in floats from the base).
// Convolution weights are [(ci * taps + k)][co] (the output channel contiguous), the LSTM's input weights of a layer are the
// forward rows then the reverse rows [1024][in] with bias_ih + bias_hh [1024] behind them, weight_hh is [2][512][128], the
// two hidden linear layers are [in][out].
struct SegModel {
  const float *wav_g, *wav_b;                      // [1]
  const float *f0, *w1, *b1, *w2, *b2;             // [251][80]; [400][60], [60]; [300][60], [60]
  const float *n_g[3], *n_b[3];                    // [80], [60], [60]
  const float *w_ih[kSegLayers], *b[kSegLayers], *w_hh[kSegLayers];
  const float *l0, *l0_b, *l1, *l1_b, *cls, *cls_b;      // [256][128], [128]; [128][128], [128]; [7][128], [7]
};

// float windows [n_win][kSegWindow] from window w0 on of a recording of n samples: i16 (f32: through f32_to_i16) / 32768, zeros behind the end
hipError_t launch_seg_windows(const void* d_pcm, int pcm_format, long n, long w0, int n_win, float* d_x, hipStream_t st);
// mean and 1 / sqrt(biased variance + 1e-5) of every channel of x [n_win][P][C] over P -> stats [n_win][C]; C <= 1024
hipError_t launch_seg_stats(const float* d_x, int n_win, int P, int C, float2* d_stats, hipStream_t st);
// stage s (0, 1, 2) of the SincNet: the input normalised with `d_stats` (and leaky_relu from stage 1 on) in the load,
// convolution, abs (stage 0) or bias, max over 3 -> out [n_win][n_pool][co]
hipError_t launch_seg_conv(int stage, const SegModel& m, const float* d_in, int n_win, int n_in, const float2* d_stats, float* d_out,
                           int n_pool, hipStream_t st);
// leaky_relu(instance norm) of the last stage's rows -> [n_win][frames][60]
hipError_t launch_seg_norm(const SegModel& m, const float* d_in, int n_win, int frames, const float2* d_stats, float* d_out, hipStream_t st);
// xproj [rows][1024] = x [rows][in] . w_ih^T + b
hipError_t launch_seg_proj(const float* d_x, long rows, int in, const float* d_w, const float* d_b, float* d_xproj, hipStream_t st);
// the recurrence of one layer, both directions of every window -> y [n_win][frames][256]
hipError_t launch_seg_lstm(const float* d_xproj, const float* d_whh, int n_win, int frames, float* d_y, hipStream_t st);
// linear + leaky_relu twice, classifier, log_softmax -> scores [rows][7]
hipError_t launch_seg_head(const SegModel& m, const float* d_y, long rows, float* d_scores, hipStream_t st);

// ---- embedding network (diar_emb.hip) -------------------------------------------------------------------------------
// WeSpeaker CAMPPlus.  Every constant of the network on the device side is here, once.
constexpr int kEmbFeat = kFbankBins, kEmbHeadCh = 32, kEmbHeadOut = 320, kEmbHeadConvs = 12;
constexpr int kEmbTdnnTaps = 5, kEmbTdnnStride = 2, kEmbInit = 128, kEmbGrowth = 32, kEmbBn = 128, kEmbGate = 64 /* 128 / reduction 2 */;
constexpr int kEmbSegLen = 100, kEmbBlocks = 3, kEmbLayers = 52, kEmbXvec = 512, kEmbStats = 2 * kEmbXvec, kEmbMaxDim = 1024;
constexpr int kEmbBlockLayers[kEmbBlocks] = {12, 24, 16}, kEmbBlockDilation[kEmbBlocks] = {1, 2, 2};
constexpr int kEmbBlockWidth[kEmbBlocks] = {512, 1024, 1024};      // channels of a block's buffer once its last layer has appended
constexpr double kEmbBnEps = 1e-5;
constexpr float kEmbPoolEps = 1e-7f;
constexpr int kEmbMinRows = 3, kEmbMaxRows = 30000;

inline long emb_frames(long rows) { return rows < 1 ? 0 : (rows - 1) / kEmbTdnnStride + 1; }
inline long emb_segments(long t2) { return (t2 + kEmbSegLen - 1) / kEmbSegLen; }

// Where each tensor sits in the handle's device copy, as the kernels read it.  Every BatchNorm is a (scale, shift) pair folded
// at load; convolution weights have the output channel contiguous: the head's [(kf * 3 + kt) * ci_n + ci][32], the tdnn's
// [(k * 320 + ci)][128], linear1 [ci][128], linear_local [(k * 128 + ci)][32], the gate's [128][64] and [64][32], a transit's
// [ci][ci / 2], the last dense [1024][dim].
struct EmbConv {
  const float *w, *scale, *shift;
};
struct EmbDense {
  const float *s1, *h1, *w1, *s2, *h2, *wl, *g1, *b1, *g2, *b2;
  int c_in, dilation;
};
struct EmbTransit {
  const float *s, *h, *w;
  int c_in;
};
struct EmbModel {
  EmbConv head[kEmbHeadConvs];      // conv1; layer1.0 conv1, conv2, shortcut; layer1.1 conv1, conv2; layer2 likewise; conv2
  EmbConv tdnn;
  EmbDense layer[kEmbLayers];
  EmbTransit transit[kEmbBlocks];
  const float *out_s, *out_h;       // out_nonlinear, applied in the last transit's store
  EmbConv dense;
  int dim;
};
// A turn's chunks: chunk c has rows row_off[c] ... row_off[c + 1] of the input, positions t2_off[c] ... after the tdnn and
// context segments seg_off[c] ... (all relative to the turn's buffers, in device memory).
struct EmbTables {
  const int *row_off, *t2_off, *seg_off;
  int n_chunks, max_rows, max_t2;
};

// head convolution `idx` (the order of EmbModel::head) on rows [rows][f_in][c_in] -> [rows][f_out][32]; `res` (nullable) is added
// before the ReLU; the last one stores [rows][320] with channel c * 10 + f
hipError_t launch_emb_head_conv(int idx, const EmbModel& m, const EmbTables& t, const float* d_in, const float* d_res, float* d_out, hipStream_t st);
// [rows][320] -> columns 0 ... 127 of the first block's buffer [t2][512]
hipError_t launch_emb_tdnn(const EmbModel& m, const EmbTables& t, const float* d_head, float* d_blk, hipStream_t st);
// C [M][N] (row stride ldc) = epilogue(relu(A [M][K] (row stride lda) * in_s + in_h) . Bt [K][N]) on the f32 matrix instruction;
// epilogue: relu(v * out_s + out_h), or plain with out_s NULL.  K is a multiple of 32, N of 128.
hipError_t launch_emb_gemm(const float* d_a, int lda, int K, const float* in_s, const float* in_h, const float* d_bt, int N, const float* out_s,
                           const float* out_h, float* d_c, int ldc, long M, hipStream_t st);
// the gate vectors [segments][32] of every chunk from h [t2][128]; d_segsum [segments][128] is scratch
hipError_t launch_emb_gates(const EmbDense& l, const EmbTables& t, const float* d_h, float* d_segsum, float* d_gates, hipStream_t st);
// linear_local of h times the gate -> columns c_in ... c_in + 31 of the block's buffer (row stride ldc)
hipError_t launch_emb_local(const EmbDense& l, const EmbTables& t, const float* d_h, const float* d_gates, float* d_blk, int ldc, hipStream_t st);
// xvec [t2][512] -> stats [n_chunks][1024]: mean, then sqrt(unbiased variance + 1e-7)
hipError_t launch_emb_pool(const EmbTables& t, const float* d_xvec, float* d_stats, hipStream_t st);
hipError_t launch_emb_dense(const EmbModel& m, const EmbTables& t, const float* d_stats, float* d_emb, hipStream_t st);

}  // namespace diar
}  // namespace crispy

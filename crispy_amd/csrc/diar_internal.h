// diar_internal.h -- what the host side (diar_api.cpp, diar_front.cpp) and the device side (diar_kernels.hip,
// diar_fbank.hip) of the speaker clustering and its front end share: the handle, the descriptors the kernels read from
// device memory and the launch functions.
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
  ~crispy_diar() {
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace crispy {
namespace diar {

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

}  // namespace diar
}  // namespace crispy

// diar_internal.h -- what diar_api.cpp (host side) and diar_kernels.hip (device side) of the speaker clustering share:
// the descriptors the kernels read from device memory and the launch functions.
#pragma once
#include <algorithm>
#include <cstddef>

#include <hip/hip_runtime.h>

#include "../../include/crispy_hip.h"
#include "diar_jacobi.h"

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

}  // namespace diar
}  // namespace crispy

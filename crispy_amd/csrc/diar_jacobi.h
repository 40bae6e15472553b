// diar_jacobi.h -- the arithmetic the two forms of the symmetric eigensolver share (diar_kernels.hip): the round-robin
// ordering of a cyclic Jacobi sweep, one rotation's cosine and sine, and the update of one 2x2 block.  Plain functions of
// their arguments, usable from host code too.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DIAR_HD __host__ __device__
#else
#define DIAR_HD
#endif

namespace crispy {
namespace diar {

constexpr int kMaxN = 2048;       // chunks of one recording / order of a matrix
constexpr int kMaxDim = 1024;
constexpr int kMaxBatch = 64;
constexpr int kLdsN = 192;        // largest order of the one-workgroup form: 192 * 192 * 4 = 147 456 bytes of LDS
constexpr int kMaxSweeps = 40;    // sweep cap of both forms (a sweep = every pair once); 6 - 12 are what it takes
constexpr float kEps = 5.9604644775390625e-08f;      // 2^-24

// Round-robin ordering (the circle method).  m = n for odd n, n - 1 for even n: the indices 0 ... m-1 sit on a circle, and
// in step t (0 ... m-1) index i meets j where i + j = 2t (mod m).  Index t meets itself: it sits out (odd n) or meets
// the index off the circle, m (even n).  K = (m + 1) / 2 pairs per step, pair 0 being the one of index t; every pair of
// indices meets exactly once in m steps.
DIAR_HD inline int rr_steps(int n) { return (n & 1) ? n : n - 1; }
DIAR_HD inline int rr_pairs(int n) { return (rr_steps(n) + 1) / 2; }
// pair l of step t: (*p, *q), with *q = -1 for the index that sits out
DIAR_HD inline void rr_pair(int n, int t, int l, int* p, int* q) {
  const int m = rr_steps(n);
  if (l == 0) {
    *p = t;
    *q = (n & 1) ? -1 : m;
    return;
  }
  int a = t + l, b = t - l;
  if (a >= m) a -= m;
  if (b < 0) b += m;
  *p = a;
  *q = b;
}

// The rotation J = [[c, s], [-s, c]] on (p, q) that zeroes a_pq in J^T A J (the smaller of the two angles), and
// t = s / c.  Worked out in double and rounded once: c^2 + s^2 is then 1 to the rounding of c and s alone, which is what
// keeps the accumulated vectors orthogonal to a few ulps over the hundreds of rotations a column goes through.
// An a_pq that changes neither diagonal element when added to it a hundredfold is dropped without a rotation (the
// classical rule): turning two vectors by 45 degrees for an off-diagonal of 1e-30 between equal diagonals of 1e-3 would
// gain nothing and cost their last bit.
DIAR_HD inline void jacobi_cs(float app, float aqq, float apq, float* c, float* s, float* t) {
  const float g = 100.0f * fabsf(apq);
  if (apq == 0.0f || (fabsf(app) + g == fabsf(app) && fabsf(aqq) + g == fabsf(aqq))) {
    *c = 1.0f;
    *s = 0.0f;
    *t = 0.0f;
    return;
  }
  const double tau = ((double)aqq - (double)app) / (2.0 * (double)apq);
  double td = 1.0 / (fabs(tau) + sqrt(1.0 + tau * tau));
  if (tau < 0.0) td = -td;
  const double cd = 1.0 / sqrt(1.0 + td * td);
  *c = (float)cd;
  *s = (float)(td * cd);
  *t = (float)td;
}

// One 2x2 block [[x_pr, x_ps], [x_qr, x_qs]] of J_k^T A J_l: rows (p, q) turned by pair k's rotation, then columns (r, s) by
// pair l's.  For the index that sits out pass zeros and (1, 0).  Fused multiply-adds are welcome here.
DIAR_HD inline void rot_block(float& x_pr, float& x_ps, float& x_qr, float& x_qs, float ck, float sk, float cl, float sl) {
#pragma clang fp contract(fast)
  const float b_pr = ck * x_pr - sk * x_qr, b_qr = sk * x_pr + ck * x_qr;
  const float b_ps = ck * x_ps - sk * x_qs, b_qs = sk * x_ps + ck * x_qs;
  x_pr = cl * b_pr - sl * b_ps;
  x_ps = sl * b_pr + cl * b_ps;
  x_qr = cl * b_qr - sl * b_qs;
  x_qs = sl * b_qr + cl * b_qs;
}
// The pair's own block: a'_pp = a_pp - t a_pq, a'_qq = a_qq + t a_pq, and the element the rotation removes is zero --
// the update of the diagonal by a small correction, which loses nothing of a_pp and a_qq (Rutishauser's form).
DIAR_HD inline void rot_diag(float& a_pp, float& a_pq, float& a_qp, float& a_qq, float t) {
#pragma clang fp contract(fast)
  const float h = t * a_pq;
  a_pp = a_pp - h;
  a_qq = a_qq + h;
  a_pq = 0.0f;
  a_qp = 0.0f;
}
// Two entries of a row of the vectors, V J.
DIAR_HD inline void rot_vec(float& x, float& y, float c, float s) {
#pragma clang fp contract(fast)
  const float nx = c * x - s * y, ny = s * x + c * y;
  x = nx;
  y = ny;
}

}  // namespace diar
}  // namespace crispy

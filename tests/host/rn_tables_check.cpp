// Host check of the two table builders the RNNoise frame kernel's host side calls (tests/test_rn_tables_host.py compiles
// and runs this): crispy_amd/csrc/rn_twiddle_rows.h (RnTables::tw8 / tw3 / tw5) and crispy_amd/csrc/rn_band_piece.h
// (RnTables::band_piece).  Exit status 0: every entry is what the index formulas it replaces give.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rn_band_piece.h"
#include "rn_twiddle_rows.h"

namespace {

struct C2 {
  float x, y;
};
bool same(C2 a, C2 b) { return std::memcmp(&a, &b, sizeof(C2)) == 0; }
bool same(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

constexpr int WAVE = 64;
C2 w960[960], tw8[4][8], tw3[32][2], tw5[96][4];

// One pass of the kernel's fft_pass_n: radix R, stride NS, NSIG signals.  For all 64 lanes and every trip, the row the
// lane reads -- by the kernel's own expression for k -- holds w960[k r (960 / (NS R))], the entry the pass indexed before.
template <int R, int NS, int RL>
int check_pass(const C2 (*rows)[RL], int nrows, int first_r, int nsig) {
  constexpr int M = 480 / R, NBF = (M + WAVE - 1) / WAVE;
  const bool joint = nsig == 2 && NBF > 1 && M % WAVE == WAVE / 2;
  int bad = 0;
  for (int lane = 0; lane < WAVE; ++lane)
    for (int nb = 0; nb < NBF; ++nb) {
      const int jm = M - WAVE / 2 + (lane & (WAVE / 2 - 1));
      const bool jt = joint && nb == NBF - 1;
      const int j = jt ? jm : lane + WAVE * nb;                                   // the lane's butterfly, if j < M
      // what the lane loads for: the clamped butterfly index of the trip (the joint trip: jm) -- and where NS divides
      // the wave one set, trip 0's, for every trip
      const int nbk = WAVE % NS == 0 ? 0 : nb;
      const int jk = jt && nbk == nb ? jm : (lane + WAVE * nbk < M - 1 ? lane + WAVE * nbk : M - 1);
      const int k = jk % NS;
      if (k < 0 || k >= nrows) { std::printf("radix %d lane %d trip %d: row %d outside the table\n", R, lane, nb, k); ++bad; continue; }
      if (j < M && j % NS != k) { std::printf("radix %d lane %d trip %d: row %d for butterfly %d\n", R, lane, nb, k, j); ++bad; }
      for (int r = 1; r < R; ++r) {
        const int idx = k * (r * (960 / (NS * R)));
        if (idx >= 960 || !same(rows[k][r - first_r], w960[idx])) {
          std::printf("radix %d lane %d trip %d r %d: row entry is not w960[%d]\n", R, lane, nb, r, idx);
          ++bad;
        }
      }
    }
  return bad;
}

int check_twiddle_rows() {
  const double pi = 3.14159265358979323846;
  int bad = 0;
  for (int fill = 0; fill < 2; ++fill) {
    // once with the table's real values, once with every entry tagged by its own index (equal cosines cannot hide a wrong index)
    for (int k = 0; k < 960; ++k)
      w960[k] = fill == 0 ? C2{(float)std::cos(-2.0 * pi * k / 960), (float)std::sin(-2.0 * pi * k / 960)} : C2{(float)k, (float)-k};
    std::memset(tw8, 0xff, sizeof(tw8));
    std::memset(tw3, 0xff, sizeof(tw3));
    std::memset(tw5, 0xff, sizeof(tw5));
    crispy::rn_build_twiddle_rows(w960, tw8, tw3, tw5);
    for (int nsig = 1; nsig <= 2; ++nsig) {
      bad += check_pass<8, 4, 8>(tw8, 4, 0, nsig);
      bad += check_pass<3, 32, 2>(tw3, 32, 1, nsig);
      bad += check_pass<5, 96, 4>(tw5, 96, 1, nsig);
    }
  }
  static_assert(crispy::rn_twiddle_step(8, 4) == 30 && crispy::rn_twiddle_step(3, 32) == 10 && crispy::rn_twiddle_step(5, 96) == 2, "");
  return bad;
}

// band_piece.  The piece structure is stated again here from the band edges (which lane holds which chunks of which half,
// in the order the builder documents), with the flags in their FIRST form: `take1` in the lane that adds lane + 1 (piece p
// with p + 1 < np), `take2` in the lane that then adds lane + 2 (piece 0 of a half of more than two pieces).  The table's
// flags sit in the giving lane and must be those shifted by one and two lanes; the sums of both forms are then run on the
// 64 lanes for random partials and must agree bit for bit, and with the band sums in double precision.
int check_band_piece() {
  using crispy::kRnEband;
  constexpr int NB = crispy::RN_BANDS;
  int tab[64];
  int bad = 0;
  if (!crispy::rn_build_band_piece(tab)) { std::printf("band_piece: builder refused the band table\n"); return 1; }
  int first[64] = {0}, count[64] = {0}, lo[64] = {0}, take1[64] = {0}, take2[64] = {0}, head[2][NB] = {{0}};
  int lane = 1;
  for (int side = 0; side < 2; ++side)
    for (int b = 0; b < NB; ++b) {
      const int c0 = side == 0 ? (b > 0 ? kRnEband[b - 1] : 0) : kRnEband[b];
      const int c1 = side == 0 ? kRnEband[b] : (b < NB - 1 ? kRnEband[b + 1] : kRnEband[b]);
      const int w = (side == 0 && b == 0) ? 0 : c1 - c0;
      if (w <= 0) continue;
      const int np = (w + 5) / 6;
      if ((lane & 15) + np > 16) lane = (lane + 15) & ~15;
      head[side][b] = lane;
      for (int p = 0, c = c0; p < np; ++p) {
        const int n = (w - (c - c0) + (np - p) - 1) / (np - p);
        first[lane + p] = c; count[lane + p] = n; lo[lane + p] = side;
        take1[lane + p] = p + 1 < np;
        take2[lane + p] = p == 0 && np > 2;
        c += n;
      }
      lane += np;
    }
  if (lane > 64) { std::printf("band_piece: %d lanes\n", lane); ++bad; }
  for (int l = 0; l < 64; ++l) {
    const int bd = tab[l];
    const int give1 = (bd >> 11) & 1, give2 = (bd >> 12) & 1;
    const int want1 = (l & 15) >= 1 ? take1[l - 1] : 0, want2 = (l & 15) >= 2 ? take2[l - 2] : 0;
    if ((bd & 127) != first[l] || ((bd >> 7) & 7) != count[l] || ((bd >> 10) & 1) != lo[l] || count[l] > 6) {
      std::printf("band_piece lane %d: chunks %d+%d side %d, expected %d+%d side %d\n", l, bd & 127, (bd >> 7) & 7, (bd >> 10) & 1, first[l], count[l], lo[l]);
      ++bad;
    }
    if (give1 != want1 || give2 != want2) { std::printf("band_piece lane %d: gives %d %d, expected %d %d\n", l, give1, give2, want1, want2); ++bad; }
    if ((l & 15) == 15 && take1[l]) { std::printf("band_piece lane %d: takes across a row\n", l); ++bad; }
    if ((l & 15) >= 14 && take2[l]) { std::printf("band_piece lane %d: takes across a row\n", l); ++bad; }
    if (l < NB && (((bd >> 13) & 63) != head[0][l] || ((bd >> 19) & 63) != head[1][l])) { std::printf("band_piece lane %d: heads\n", l); ++bad; }
    if (bd >> 25) { std::printf("band_piece lane %d: bits above 24\n", l); ++bad; }
  }
  unsigned rng = 12345u;
  for (int trial = 0; trial < 200; ++trial) {
    float part_lo[100], part_hi[100];
    for (int c = 0; c < 100; ++c) {
      rng = rng * 1664525u + 1013904223u; part_lo[c] = (float)(rng >> 8) * (1.f / 16777216.f) * (trial % 3 == 0 ? 1e-3f : 1.f);
      rng = rng * 1664525u + 1013904223u; part_hi[c] = (float)(rng >> 8) * (1.f / 16777216.f);
    }
    float s[64], a[64], g[64];
    for (int l = 0; l < 64; ++l) {
      const int bd = tab[l], n = (bd >> 7) & 7;
      const float* p = ((bd >> 10) & 1 ? part_lo : part_hi) + (bd & 127);
      float v = 0.f;
      for (int k = 0; k < 6; ++k) v += k < n ? p[k] : 0.f;
      s[l] = v;
    }
    auto shl = [](const float* v, int l, int d) { return (l & 15) + d < 16 ? v[l + d] : 0.f; };   // row_shl:d, 0 past the row's end
    // first form: the taking lane selects
    float t[64];
    for (int l = 0; l < 64; ++l) t[l] = s[l] + (take1[l] ? shl(s, l, 1) : 0.f);
    for (int l = 0; l < 64; ++l) a[l] = t[l] + (take2[l] ? shl(t, l, 2) : 0.f);
    // the kernel's form: the giving lane masks
    float u[64];
    for (int l = 0; l < 64; ++l) u[l] = (tab[l] >> 11) & 1 ? s[l] : 0.f;
    for (int l = 0; l < 64; ++l) t[l] = s[l] + shl(u, l, 1);
    for (int l = 0; l < 64; ++l) u[l] = (tab[l] >> 12) & 1 ? t[l] : 0.f;
    for (int l = 0; l < 64; ++l) g[l] = t[l] + shl(u, l, 2);
    for (int b = 0; b < NB; ++b) {
      const float tot_a = a[(tab[b] >> 13) & 63] + a[(tab[b] >> 19) & 63], tot_g = g[(tab[b] >> 13) & 63] + g[(tab[b] >> 19) & 63];
      double ref = 0.0;
      for (int c = b > 0 ? kRnEband[b - 1] : 0; c < (b > 0 ? kRnEband[b] : 0); ++c) ref += part_hi[c];
      for (int c = kRnEband[b]; c < (b < NB - 1 ? kRnEband[b + 1] : kRnEband[b]); ++c) ref += part_lo[c];
      // (<= 44 positive terms: the f32 tree is within 44 * 2^-24 of the exact sum, relative)
      if (!same(tot_a, tot_g) || std::fabs((double)tot_g - ref) > 44.0 * std::ldexp(1.0, -24) * ref + 1e-30) {
        std::printf("trial %d band %d: taking form %.9g, giving form %.9g, exact %.9g\n", trial, b, tot_a, tot_g, ref);
        ++bad;
      }
    }
  }
  return bad;
}

}  // namespace

int main() {
  const int bad_tw = check_twiddle_rows(), bad_bp = check_band_piece();
  std::printf("rn twiddle rows: %s\n", bad_tw ? "FAILED" : "ok");
  std::printf("rn band pieces: %s\n", bad_bp ? "FAILED" : "ok");
  return bad_tw || bad_bp ? 1 : 0;
}

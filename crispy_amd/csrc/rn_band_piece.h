// rn_band_piece.h -- RnTables::band_piece (rn_common.h), built on the host.  Plain C++ with no HIP in it:
// tests/host/rn_band_piece_check.cpp compiles this text into a host program and holds the table to the band sums it stands for.
#pragma once

namespace crispy {

constexpr int RN_BANDS = 22;
// Opus band edges in 4-bin chunks
constexpr int kRnEband[RN_BANDS] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100};

// The 42 non-empty half-bands -- rising half of band b = chunk partials part_hi[e(b-1) .. e(b)), falling half =
// part_lo[e(b) .. e(b+1)) -- cut into pieces of <= 6 chunks, one piece per lane, the <= 4 pieces of a half on neighbouring
// lanes of one 16-lane row.  Lane 0 stays idle = the "zero" source of the two half-bands that do not exist (rising half of
// band 0, falling half of band 21).  out[lane] packs
//   bits 0-6 first chunk | 7-9 chunks (0: idle lane) | 10 part_lo (else part_hi)
//   | 11 this lane's sum is added into lane - 1 | 12 then this lane's sum is added into lane - 2
//   | 13-18 lane holding the total of the rising half of band `lane` | 19-24 ... of the falling half (lanes < 22)
// The two flags sit in the lane that GIVES (band_sum masks the value it sends and adds with one shifted DPP add): piece
// p >= 1 gives to piece p - 1, and piece 2 of a half of three or four pieces -- by then the sum of pieces 2 and 3 --
// gives to piece 0.  Returns false if the band table does not fit the scheme (it does).
inline bool rn_build_band_piece(int (&out)[64]) {
  int piece[64] = {0}, head[2][RN_BANDS];
  for (int b = 0; b < RN_BANDS; ++b) head[0][b] = head[1][b] = 0;
  int lane = 1;
  for (int side = 0; side < 2; ++side)          // 0: rising halves (part_hi), 1: falling halves (part_lo)
    for (int b = 0; b < RN_BANDS; ++b) {
      const int c0 = side == 0 ? (b > 0 ? kRnEband[b - 1] : 0) : kRnEband[b];
      const int c1 = side == 0 ? kRnEband[b] : (b < RN_BANDS - 1 ? kRnEband[b + 1] : kRnEband[b]);
      const int w = (side == 0 && b == 0) ? 0 : c1 - c0;
      if (w <= 0) continue;
      const int np = (w + 5) / 6;                                  // <= 4 pieces (w <= 22)
      if ((lane & 15) + np > 16) lane = (lane + 15) & ~15;         // a half's pieces stay inside one DPP row
      if (np > 4 || lane + np > 64) return false;
      head[side][b] = lane;
      for (int p = 0, c = c0; p < np; ++p) {
        const int n = (w - (c - c0) + (np - p) - 1) / (np - p);    // balanced: 22 -> 6, 6, 5, 5
        piece[lane + p] = c | (n << 7) | (side << 10) | ((p >= 1 ? 1 : 0) << 11) | ((p == 2 ? 1 : 0) << 12);
        c += n;
      }
      lane += np;
    }
  for (int l = 0; l < 64; ++l) {
    const int b = l < RN_BANDS ? l : 0;
    out[l] = piece[l] | (head[0][b] << 13) | (head[1][b] << 19);
  }
  return true;
}

}  // namespace crispy

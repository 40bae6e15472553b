// rn_twiddle_rows.h -- RnTables::tw8 / tw3 / tw5 (rn_common.h), built on the host.  Plain C++ with no HIP in it:
// tests/host/rn_twiddle_rows_check.cpp compiles this text into a host program and compares every entry with the index
// formula of the frame kernel's Stockham passes.
//
// Butterfly j of a radix-R pass with stride NS multiplies its input r by w960[k r (960 / (NS R))], k = j % NS.  Taken from
// w960 that is one index product and one 8-byte load per r; here the R - 1 values of one k stand side by side, so a lane
// forms one row address and the values come as 16-byte loads at immediate offsets.  The entries are COPIES of w960's: the
// transform multiplies by the same bits.
#pragma once

namespace crispy {

constexpr int rn_twiddle_step(int R, int NS) { return 960 / (NS * R); }

template <class C>
inline void rn_build_twiddle_rows(const C (&w960)[960], C (&tw8)[4][8], C (&tw3)[32][2], C (&tw5)[96][4]) {
  for (int k = 0; k < 4; ++k)
    for (int r = 0; r < 8; ++r) tw8[k][r] = w960[k * r * rn_twiddle_step(8, 4)];        // (r = 0: w960[0], never read)
  for (int k = 0; k < 32; ++k)
    for (int r = 1; r < 3; ++r) tw3[k][r - 1] = w960[k * r * rn_twiddle_step(3, 32)];
  for (int k = 0; k < 96; ++k)
    for (int r = 1; r < 5; ++r) tw5[k][r - 1] = w960[k * r * rn_twiddle_step(5, 96)];
}

}  // namespace crispy

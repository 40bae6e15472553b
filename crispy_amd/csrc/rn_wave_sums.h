// rn_wave_sums.h -- several wave-wide sums for the price of one (gfx950, wave64).
//
// A lone wave sum is six dependent cross-lane steps (wave_sum1 below) and the frame kernel takes ~62 of them per
// frame (the lag inner products of the pitch search, the LPC autocorrelation): ~560 VALU instructions, 7 % of the frame.
// Here N values are reduced TOGETHER: v_permlane32_swap puts the lower halves of two values into one register and their
// upper halves into another -- one add folds both values to 32 lanes --, v_permlane16_swap does the same with the odd /
// even 16-lane rows of two such registers, and four DPP steps (row_sum16, wave_ops.h) finish the four rows at once.  Four sums: 3 swaps + 3 adds +
// 4 DPP adds + 4 v_readlane instead of 4 x (6 steps + v_readlane).  The association of the additions differs from the
// single form (lanes l and l + 32 first); both are trees, neither is the reference's sequential order.
// Lane semantics checked on the hardware by tools/micro/wave_sum4_test.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_ops.h"

namespace crispy {

// The two steps that join the 16-lane rows: v += lane 15 of the row before (rows 1 and 3), then v += lane 31 (rows 2 and
// 3); the rows a step does not name keep v.  Written as `v += dpp_mov<0x142, 0xa>(v)` a step was three instructions -- a
// copy of zero for the rows that are masked off, v_mov_b32_dpp, v_add_f32: the DPP combiner folds a move with disabled
// rows into its user only for integer operations.  v_add_f32_dpp with the destination as its own `old` is the same
// sum in the rows that count (what leaves the reduction is read from lanes 31 and 63) in one instruction.  Inline
// assembly stands outside the compiler's hazard bookkeeping, so the wait states are spelled out: five in front (a VALU
// write of EXEC before a DPP instruction; a VALU write of the register itself needs two), one before the v_readlane
// that follows.
__device__ __forceinline__ float ws_join_rows(float v) {
  asm("s_nop 4\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 0" : "+v"(v));
  return v;
}
__device__ __forceinline__ float ws_join_row_pairs(float v) {      // rows 0 + 1 in lane 31, rows 2 + 3 in lane 63
  asm("s_nop 4\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 0" : "+v"(v));
  return v;
}
// first := [first.lanes 0-31 | second.lanes 0-31], second := [first.lanes 32-63 | second.lanes 32-63]
__device__ __forceinline__ void ws_swap32(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
// rows of 16 lanes: first := [f0, s0, f2, s2], second := [f1, s1, f3, s3]
__device__ __forceinline__ void ws_swap16(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}
__device__ __forceinline__ float ws_lane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ void wave_sum4(float& a, float& b, float& c, float& d) {
  ws_swap32(a, b);
  float ab = a + b;             // lanes 0-31: a folded to 32 lanes, lanes 32-63: b
  ws_swap32(c, d);
  float cd = c + d;
  ws_swap16(ab, cd);
  const float q = row_sum16(ab + cd);     // row 0: a, row 1: c, row 2: b, row 3: d
  a = ws_lane(q, 0);
  c = ws_lane(q, 16);
  b = ws_lane(q, 32);
  d = ws_lane(q, 48);
}
__device__ __forceinline__ void wave_sum2(float& a, float& b) {
  ws_swap32(a, b);
  const float q = ws_join_row_pairs(row_sum16(a + b));      // rows 0, 1: a; rows 2, 3: b
  a = ws_lane(q, 31);
  b = ws_lane(q, 63);
}
__device__ __forceinline__ float wave_sum1(float v) {
  return ws_lane(ws_join_rows(row_sum16(v)), 63);
}
// v[i] := sum over the 64 lanes of v[i], wave-uniform, for all i < N
template <int N>
__device__ __forceinline__ void wave_sums(float (&v)[N]) {
  int i = 0;
#pragma unroll
  for (; i + 4 <= N; i += 4) wave_sum4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  if (N - i == 3) {
    float z = 0.f;
    wave_sum4(v[i], v[i + 1], v[i + 2], z);
  } else if (N - i == 2) {
    wave_sum2(v[i], v[i + 1]);
  } else if (N - i == 1) {
    v[i] = wave_sum1(v[i]);
  }
}

}  // namespace crispy

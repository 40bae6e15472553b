// wave_ops.h -- the wave-level idioms every kernel file shares (gfx950, wave64), each defined once: LDS synchronisation
// of a wave and of a workgroup, DPP lane permutations and the row sums built on them, __shfl_xor reductions, and the
// f16 vector types.  Everything is __device__ __forceinline__ and straight-line: a call compiles to the instructions the
// idiom had when it was written out (tools/isa_same.py is the check).
#pragma once
#include <hip/hip_runtime.h>

namespace crispy {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

// "This wave's LDS traffic has landed": a barrier for the LDS traffic of ONE wave, also inside a multi-wave workgroup.
// The wave runs in lockstep and its LDS operations complete in order, so a wait for them is all the hardware needs; the
// fences keep the compiler from moving LDS accesses across the point.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier for LDS traffic ONLY: __syncthreads() waits for every outstanding vector-memory operation first
// (s_waitcnt vmcnt(0)), i.e. the first barrier of a kernel would wait for all the weights and keys requested at its top
// and serialise exactly the overlap the fused decode kernels are built on (measured: a row's pass through the MLP block
// cost ~3 us with the next row's residual stream "in flight").  Only for kernels that hand no GLOBAL data from wave to wave.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// DPP lane permutations (gfx9 family): no LDS crossbar round trip, one VALU op per step.  CTRL: 0xB1 quad_perm [1,0,3,2],
// 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror, 0x140 row_mirror, 0x101 / 0x102 row_shl:1 / 2.
// (`old` = 0: passing the value itself -- legal for the quad / mirror permutations, whose every lane has a valid source --
// ties the destination to the source register and cost 83 more copies than the zero-initialising moves it removed.  With
// all rows and banks enabled the combiner folds the move into its user; for an integer maximum it can do so only with
// old = 0 -- x is not the identity of the operation -- and each step was a copy, a DPP move and the maximum.)
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_mov(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_mov(float v) {
  return __int_as_float(dpp_mov<CTRL, ROW_MASK>(__float_as_int(v)));
}
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) { return v + dpp_mov<CTRL>(v); }
// v + (v of the permuted lane) as ONE v_add_f32_dpp: the DPP combiner only folds a v_mov_b32_dpp into its user inside one
// basic block, and the compiler likes to sink the add into a following `if (lane ...) store` -- then the move, its
// zero-initialised destination and the add are three instructions.  Pinning the sum (an empty asm that "uses" it) keeps
// the add where the move is.
template <int CTRL>
__device__ __forceinline__ float dpp_add_pinned(float v) {
  float r = v + dpp_mov<CTRL>(v);
  asm volatile("" : "+v"(r));
  return r;
}
// v + (u of the permuted lane; 0 where the pattern has no source lane), pinned like dpp_add_pinned
template <int CTRL>
__device__ __forceinline__ float dpp_add_of_pinned(float v, float u) {
  float r = v + dpp_mov<CTRL>(u);
  asm volatile("" : "+v"(r));
  return r;
}
// sum over the 8 / 16 lanes that share a DPP row (every one of them ends up with the total)
__device__ __forceinline__ float row_sum8(float v) { return dpp_add<0x141>(dpp_add<0x4E>(dpp_add<0xB1>(v))); }
__device__ __forceinline__ float row_sum16(float v) { return dpp_add<0x140>(row_sum8(v)); }

// Butterfly reductions on __shfl_xor over the lane distances FROM, ..., TO (powers of two, halving or doubling); every
// lane that takes part ends up with the result.  <32, 1>: all 64 lanes; <8, 32>: across the 8-lane groups (lanes with
// equal lane % 8); <16, 32>: across the 16-lane rows.  The order of the steps is part of a sum's bits.
template <int FROM = 32, int TO = 1>
__device__ __forceinline__ float shfl_sum(float v) {
#pragma unroll
  for (int off = FROM; FROM > TO ? off >= TO : off <= TO; off = FROM > TO ? off >> 1 : off << 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int FROM = 32, int TO = 1>
__device__ __forceinline__ float shfl_max(float v) {
#pragma unroll
  for (int off = FROM; FROM > TO ? off >= TO : off <= TO; off = FROM > TO ? off >> 1 : off << 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

}  // namespace crispy

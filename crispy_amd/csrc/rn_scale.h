// rn_scale.h -- the power-of-two scale pair of the gain network's fixed-point digit images (rn_kernels.hip: image_i8,
// dotn_i), kept apart from the kernels so that a host program can compile the same text: tests/test_rn_scale_host.py runs
// scale_of and scale_shift over every exponent, the clamp's ends included, against the multiplications they stand for.
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
#define RN_SCALE_FN __device__ __forceinline__
// keeps a wave-uniform value in a scalar register (an empty statement for the code generator to route the value through)
#define RN_PIN_SCALAR(x) asm volatile("" : "+s"(x))
#define RN_PIN_SCALAR2(x, y) asm volatile("" : "+s"(x), "+s"(y))
#elif defined(__HIPCC__)
#define RN_SCALE_FN __device__ __forceinline__
#define RN_PIN_SCALAR(x) ((void)0)
#define RN_PIN_SCALAR2(x, y) ((void)0)
#else
#define RN_SCALE_FN inline
#define RN_PIN_SCALAR(x) ((void)0)
#define RN_PIN_SCALAR2(x, y) ((void)0)
#endif

namespace crispy {

// scale pair of a vector whose largest magnitude is m (wave-uniform): up = 2^s, dn = 2^-s
struct RnScale { float up, dn; };
// m is wave-uniform and arrives in a scalar register (wave_max), but instruction selection follows the consumer (v * up)
// and took the whole exponent arithmetic, and wave_max's last two maxima, onto the vector unit: the bit pattern is pinned
// to the scalar unit on the way in and the pair on the way out.
RN_SCALE_FN RnScale scale_of(float m) {
  int mi = __builtin_bit_cast(int, m);
  RN_PIN_SCALAR(mi);
  int eb = (mi >> 23) & 0xff;                      // m < 2^(eb - 126)
  eb = eb > 64 ? eb : 64;
  RN_PIN_SCALAR(eb);                               // (min of max would become a v_med3_u32)
  eb = eb < 250 ? eb : 250;
  int up = (283 - eb) << 23, dn = (eb - 29) << 23; // 2^(30 - (eb - 126)) and its inverse
  RN_PIN_SCALAR2(up, dn);
  return RnScale{__builtin_bit_cast(float, up), __builtin_bit_cast(float, dn)};
}
// s 2^E for a power of two s from scale_of and E <= 24: the exponent field of dn is at most 221 (eb <= 250), so adding E to
// it stays in the normal range and gives the float that the multiplication by 2^E rounds to -- on the scalar unit
template <int E>
RN_SCALE_FN float scale_shift(float s) {
  return __builtin_bit_cast(float, __builtin_bit_cast(int, s) + (E << 23));
}

}  // namespace crispy

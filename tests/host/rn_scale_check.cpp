// Host check of crispy_amd/csrc/rn_scale.h (built and run by tests/test_rn_scale_host.py): the header's own scale_of and
// scale_shift, compiled for the host, over every exponent byte -- below, at and above both ends of the clamp [64, 250] --
// several mantissas, both signs' magnitudes being what the kernel passes (non-negative bit patterns), NaN and infinity
// patterns included.  References: the parent's min(max()) form of the pair, and the float multiplications by 2^8, 2^16 and
// 2^24 that scale_shift replaced.  Prints the ranges it covered and exits non-zero at the first difference.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "rn_scale.h"

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static float from_bits(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }

int main() {
  const unsigned mant[] = {0u, 1u, 0x400000u, 0x7fffffu};
  int n = 0, eb_lo = 999, eb_hi = -1;
  for (unsigned e = 0; e < 256; ++e) {
    for (unsigned mt : mant) {
      const float m = from_bits((e << 23) | mt);
      const crispy::RnScale sc = crispy::scale_of(m);
      // the parent's form
      int eb = (int)((bits(m) >> 23) & 0xff);
      eb = eb < 64 ? 64 : (eb > 250 ? 250 : eb);
      const float up = from_bits((unsigned)(283 - eb) << 23), dn = from_bits((unsigned)(eb - 29) << 23);
      if (bits(sc.up) != bits(up) || bits(sc.dn) != bits(dn)) { std::printf("scale_of differs at exponent %u mantissa %#x\n", e, mt); return 1; }
      // what the pair means: up = 2^(30 - (eb - 126)), dn its inverse, both normal; m up < 2^30 for every m inside the clamp
      if (sc.up != std::ldexp(1.f, 30 - (eb - 126)) || sc.dn != std::ldexp(1.f, (eb - 126) - 30) || sc.up * sc.dn != 1.f) { std::printf("pair is not 2^s, 2^-s at exponent %u\n", e); return 1; }
      if (!std::isnormal(sc.up) || !std::isnormal(sc.dn)) { std::printf("pair leaves the normal range at exponent %u\n", e); return 1; }
      if (e >= 64 && e <= 250 && !(m * sc.up < 1073741824.f)) { std::printf("m up >= 2^30 at exponent %u mantissa %#x\n", e, mt); return 1; }
      // scale_shift against the multiplications of fold
      const float s8 = crispy::scale_shift<8>(sc.dn), s16 = crispy::scale_shift<16>(sc.dn), s24 = crispy::scale_shift<24>(sc.dn);
      if (bits(s8) != bits(sc.dn * 256.f) || bits(s16) != bits(sc.dn * 65536.f) || bits(s24) != bits(sc.dn * 16777216.f)) { std::printf("scale_shift differs from the product at exponent %u\n", e); return 1; }
      if (!std::isnormal(s24)) { std::printf("dn 2^24 leaves the normal range at exponent %u\n", e); return 1; }
      eb_lo = eb < eb_lo ? eb : eb_lo;
      eb_hi = eb > eb_hi ? eb : eb_hi;
      ++n;
    }
  }
  std::printf("rn_scale ok: %d inputs, clamped exponent %d .. %d\n", n, eb_lo, eb_hi);
  return 0;
}

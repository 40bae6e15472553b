// Host check of crispy_amd/csrc/rn_prio.h, the rule by which a wave of the one-wave RNNoise frame kernel picks its issue
// priority (tests/test_rn_prio_host.py compiles and runs this).  Exit status 0: every property holds for the mode the
// header ships (or the one given with -DRN_PRIO_MODE=n).
#include <cstdio>

#include "rn_prio.h"

using crispy::kRnPrioMode;
using crispy::rn_prio_at;
using crispy::rn_prio_of;

static_assert(rn_prio_of(0, 0) >= 0, "usable in constant expressions");

int main() {
  int bad = 0;
  const int T = 12;   // frames of a launch, for the last-frame rule of mode 3
  // values stay in 0 .. 3 for every slot a SIMD has, at every frame
  for (unsigned slot = 0; slot < 16; ++slot)
    for (int t = 0; t < 64; ++t) {
      const int p = rn_prio_of(slot, t), q = rn_prio_at(slot, t, T);
      if (p < 0 || p > 3 || q < 0 || q > 3) { std::printf("slot %u frame %d: priority %d / %d out of range\n", slot, t, p, q); ++bad; }
    }
  if (kRnPrioMode >= 1) {
    // four neighbouring slots hold four distinct priorities at every frame
    for (unsigned s0 = 0; s0 < 16; s0 += 4)
      for (int t = 0; t < 64; ++t) {
        unsigned seen = 0;
        for (unsigned s = s0; s < s0 + 4; ++s) seen |= 1u << rn_prio_of(s, t);
        if (seen != 0xfu) { std::printf("slots %u..%u frame %d: priorities not distinct (mask %x)\n", s0, s0 + 3, t, seen); ++bad; }
      }
  }
  if (kRnPrioMode >= 2) {
    // over any four consecutive frames a slot takes each priority once
    for (unsigned slot = 0; slot < 16; ++slot)
      for (int t = 0; t < 60; ++t) {
        unsigned seen = 0;
        for (int d = 0; d < 4; ++d) seen |= 1u << rn_prio_of(slot, t + d);
        if (seen != 0xfu) { std::printf("slot %u frames %d..%d: not every priority (mask %x)\n", slot, t, t + 3, seen); ++bad; }
      }
  }
  // inside a launch rn_prio_at is rn_prio_of; only mode 3 differs, in the last frame, where all waves are equal
  for (unsigned slot = 0; slot < 16; ++slot)
    for (int t = 0; t < T; ++t) {
      const bool last = kRnPrioMode == 3 && t == T - 1;
      if (!last && rn_prio_at(slot, t, T) != rn_prio_of(slot, t)) { std::printf("slot %u frame %d: rn_prio_at differs\n", slot, t); ++bad; }
      if (last && rn_prio_at(slot, t, T) != rn_prio_at(0, t, T)) { std::printf("slot %u: last frame not level\n", slot); ++bad; }
    }
  std::printf("rn_prio mode %d: %s\n", kRnPrioMode, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

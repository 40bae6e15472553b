// rn_prio.h -- issue priority of a wave of the one-wave RNNoise frame kernel (rn_kernels.hip), as plain integer
// arithmetic so that the rule the kernel compiles can be checked on the host (tests/test_rn_prio_host.py).
//
// Four waves share a SIMD's vector issue port.  Different priorities keep them out of phase without anyone sleeping;
// which wave holds which priority is the rule below.  `slot` is the wave's slot on its SIMD (HW_ID bits 3:0), `t` the
// frame inside the launch.
//   RN_PRIO_MODE 0  none: every wave stays at the priority it was launched with (0)
//                1  fixed per slot for the whole launch: slot & 3
//                2  rotating: (slot + t) & 3 -- at every frame the four slots hold four priorities, and over four
//                   frames every slot holds each once, so no wave lives on leftovers for a whole launch
//                3  mode 2, and every wave at the same priority in the last frame of the launch
#pragma once

#ifndef RN_PRIO_MODE
#define RN_PRIO_MODE 2
#endif

namespace crispy {

constexpr int kRnPrioMode = RN_PRIO_MODE;
static_assert(kRnPrioMode >= 0 && kRnPrioMode <= 3, "RN_PRIO_MODE is 0, 1, 2 or 3");

// Priority (0 .. 3, the operand of s_setprio) of the wave in `slot` during frame `t` of a launch.
constexpr int rn_prio_of(unsigned slot, int t) {
  return kRnPrioMode == 0 ? 0 : kRnPrioMode == 1 ? (int)(slot & 3u) : (int)((slot + (unsigned)t) & 3u);
}
// The same for a launch of T frames: mode 3 levels the waves in its last frame.
constexpr int rn_prio_at(unsigned slot, int t, int T) {
  return (kRnPrioMode == 3 && t == T - 1) ? 0 : rn_prio_of(slot, t);
}

}  // namespace crispy

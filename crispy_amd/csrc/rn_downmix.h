// rn_downmix.h -- the app-audio handlers' downmix (src-tauri/src/commands/recording.rs:260-369), shared by the kernels that
// read app audio: rn_rec_app_kernel (rn_record.hip) and rn_rec_app_at_kernel (rn_capture.hip).  Device code only.  Both files
// switch contraction off before they include anything that computes.
#pragma once
#include <hip/hip_runtime.h>

namespace crispy {

// 1 channel: the sample itself; 2: (f0 + f1) / 2.0; more: `iter().sum::<f32>()`, which starts from 0.0 and adds in order,
// then `/ channels as f32`.  Every add rounds on its own and the division is correctly rounded.
static __device__ __forceinline__ float app_downmix(const float* f, int channels) {
#pragma clang fp contract(off)
  if (channels == 1) return f[0];
  if (channels == 2) return (f[0] + f[1]) / 2.0f;
  float acc = 0.0f;
  for (int c = 0; c < channels; ++c) acc = acc + f[c];
  return acc / (float)channels;
}

}  // namespace crispy

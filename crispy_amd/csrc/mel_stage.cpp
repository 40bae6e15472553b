// mel_stage.cpp -- stage entry point of the log-mel front end for the parity tests (include/crispy_hip.h).  A file of its
// own: the host-logic harness of tests/asan compiles asr_api.cpp against its launcher stand-ins and needs none for this.
#include "../../include/crispy_hip.h"
#include "api_util.h"
#include "asr_common.h"

using namespace crispy;

extern "C" {

int crispy_mel_stage_log10_device(crispy_mel* h, const double* d_s, float* d_y, size_t n, void* hip_stream) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_mel_stage_log10_device: NULL handle");
  if (n == 0) return CRISPY_OK;
  if (!d_s || !d_y) return fail(CRISPY_ERR_INVALID_ARG, "crispy_mel_stage_log10_device: NULL pointer");
  if (n > ((size_t)1 << 40)) return fail(CRISPY_ERR_INVALID_ARG, "crispy_mel_stage_log10_device: n too large");
  HIP_TRY(hipSetDevice(mel_handle_device(h)));
  HIP_TRY(mel_log10_launch(d_s, d_y, (long)n, hip_stream ? (hipStream_t)hip_stream : mel_handle_stream(h)));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_mel_stage_log10_device")

}  // extern "C"

// pk_tdt_harness.cpp -- TEST INFRASTRUCTURE ONLY.  The device-free host logic of Parakeet's TDT decoder under AddressSanitizer +
// UBSan on the CPU box: pk_tdt_api.cpp is compiled HERE, unmodified, against the host-memory HIP stand-in of
// tests/asan/hip/hip_runtime.h; the launchers it calls are the no-ops below.  What runs for real: the config and limit checks,
// crispy_pk_tdt_max_steps, the tensor table, the load's validation and its layout loops (into a "device" buffer that ASan
// watches), the call's checks and workspace carving, and crispy_pk_tdt_words on hostile steps, pieces and buffer sizes.
// Built and driven by tests/test_pk_tdt_sanitizers.py; never linked into the product.  Exit status 0 = every case answered as
// expected; a sanitizer report ends the process.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hip/hip_runtime.h"
static inline hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) { *free_b = *total_b = (size_t)1 << 30; return hipSuccess; }

#include "../../crispy_amd/csrc/api_util.cpp"
#include "../../crispy_amd/csrc/pk_tdt_api.cpp"

namespace crispy {
namespace pk {
hipError_t launch_gemm(GemmEpilogue, const float*, int, const float*, const float*, int, float, const float*, float*, long, hipStream_t) { return hipSuccess; }
hipError_t launch_tdt_init(const TdtModel&, const TdtState& s, hipStream_t) {      // what the init kernel leaves: no steps, every clip finished
  for (int c = 0; c < s.n_clips; ++c) s.n_steps[c] = 0;
  *s.finished = s.n_clips;
  return hipSuccess;
}
hipError_t launch_tdt_predict(const TdtModel&, const TdtState&, hipStream_t) { return hipSuccess; }
hipError_t launch_tdt_joint(const TdtModel&, const TdtState&, hipStream_t) { return hipSuccess; }
hipError_t launch_tdt_advance(const TdtModel&, const TdtState&, hipStream_t) { return hipSuccess; }
}  // namespace pk
}  // namespace crispy

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      std::fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, crispy::last_error_cstr()); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

static crispy_pk_tdt_config tiny() {
  crispy_pk_tdt_config c{};
  c.hidden = 64; c.decoder_hidden = 128; c.decoder_layers = 2; c.vocab = 70; c.blank = 69; c.n_durations = 5; c.max_symbols_per_step = 10;
  for (int i = 0; i < 5; ++i) c.durations[i] = i;
  return c;
}

static void configs_and_budgets() {
  crispy_pk_tdt_config c = tiny();
  EXPECT(crispy_pk_tdt_max_steps(&c, 0) == 0 && crispy_pk_tdt_max_steps(&c, -7) == 0 && crispy_pk_tdt_max_steps(&c, 1) == 9);
  EXPECT(crispy_pk_tdt_max_steps(&c, 5000) == 49999 && crispy_pk_tdt_max_steps(&c, 5001) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_tdt_max_steps(nullptr, 1) == CRISPY_ERR_INVALID_ARG);
  std::mt19937 rng(1);
  int fields[15];
  for (int i = 0; i < 4000; ++i) {      // hostile configs: every answer a count or a status, never a crash
    std::memcpy(fields, &c, sizeof c);
    const int n = 1 + (int)(rng() % 3);
    for (int k = 0; k < n; ++k) {
      const int which = (int)(rng() % 15);
      const unsigned r = rng();
      fields[which] = (r & 3) == 0 ? (int)r : (r & 3) == 1 ? (int)(r % 70000) - 100 : (r & 3) == 2 ? INT32_MAX - (int)(r % 3) : INT32_MIN + (int)(r % 3);
    }
    crispy_pk_tdt_config bad;
    std::memcpy(&bad, fields, sizeof bad);
    const char* name = nullptr;
    long count = 0;
    const int rc = crispy_pk_tdt_tensor_spec(&bad, (int)(rng() % 20) - 2, &name, &count);
    EXPECT(rc == CRISPY_ERR_INVALID_ARG || (rc == 3 + 4 * bad.decoder_layers + 4 && name && count > 0));
    const long steps = crispy_pk_tdt_max_steps(&bad, (long)(rng() % 6000) - 10);
    EXPECT(steps == CRISPY_ERR_INVALID_ARG || (steps >= 0 && steps < 64L * 5000));
  }
}

static void load_and_call() {
  const crispy_pk_tdt_config c = tiny();
  void* h = nullptr;
  EXPECT(crispy_pk_tdt_create(0, &h) == CRISPY_OK && h);
  const char* name = nullptr;
  long count = 0;
  const int n = crispy_pk_tdt_tensor_spec(&c, 0, &name, &count);
  EXPECT(n == 15);
  std::vector<std::string> names;
  std::vector<std::vector<float>> data;
  for (int i = 0; i < n; ++i) {
    EXPECT(crispy_pk_tdt_tensor_spec(&c, i, &name, &count) == n);
    names.push_back(name);
    data.emplace_back((size_t)count, 0.25f);      // exactly `count` floats each: a read past one is a report
  }
  auto load = [&](int drop, int repeat, long off, int at) {
    std::vector<const char*> np;
    std::vector<const float*> dp;
    std::vector<long> cp;
    for (int i = 0; i < n; ++i) {
      if (i == drop) continue;
      np.push_back(names[(size_t)i].c_str());
      dp.push_back(data[(size_t)i].data());
      cp.push_back((long)data[(size_t)i].size() + (i == at ? off : 0));
    }
    if (repeat >= 0) {
      np.push_back(names[(size_t)repeat].c_str());
      dp.push_back(data[(size_t)repeat].data());
      cp.push_back((long)data[(size_t)repeat].size());
    }
    return crispy_pk_tdt_load(h, &c, np.data(), dp.data(), cp.data(), (int)np.size());
  };
  for (int i = 0; i < n; ++i) {
    EXPECT(load(i, -1, 0, -1) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "missing"));
    EXPECT(load(-1, i, 0, -1) == CRISPY_ERR_INVALID_ARG && std::strstr(crispy::last_error_cstr(), "twice"));
    EXPECT(load(-1, -1, 1, i) == CRISPY_ERR_INVALID_ARG && load(-1, -1, -1, i) == CRISPY_ERR_INVALID_ARG);
  }
  EXPECT(crispy_pk_tdt_loaded(h) == 0);
  long off[4] = {0, 3, 3, 10};
  int steps[3 * (29 + 69)] = {0}, n_steps[3] = {-1, -1, -1};
  float frames[10 * 64] = {0};
  EXPECT(crispy_pk_tdt_decode(h, frames, off, 3, steps, n_steps, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);      // before a load
  EXPECT(load(-1, -1, 0, -1) == CRISPY_OK && crispy_pk_tdt_loaded(h) == 1);
  EXPECT(load(-1, -1, 0, -1) == CRISPY_OK);      // a reload lets the first copy go (the leak check is the test)
  crispy_pk_tdt_config back{};
  EXPECT(crispy_pk_tdt_config_of(h, &back) == CRISPY_OK && std::memcmp(&back, &c, sizeof c) == 0);
  std::vector<float> proj(10 * 128), tap((size_t)(29 + 69) * 75);
  EXPECT(crispy_pk_tdt_decode(h, frames, off, 3, steps, n_steps, proj.data(), tap.data()) == CRISPY_OK);      // the buffers and the workspace at their sizes
  EXPECT(n_steps[0] == 0 && n_steps[1] == 0 && n_steps[2] == 0);
  long bad_off[3] = {0, 5001, 5002};
  EXPECT(crispy_pk_tdt_decode(h, frames, bad_off, 2, steps, n_steps, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  long back_off[3] = {0, 4, 2};
  EXPECT(crispy_pk_tdt_decode(h, frames, back_off, 2, steps, n_steps, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_tdt_decode(h, frames, off, 0, steps, n_steps, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  EXPECT(crispy_pk_tdt_decode(h, frames, off, 4097, steps, n_steps, nullptr, nullptr) == CRISPY_ERR_INVALID_ARG);
  crispy_pk_tdt_destroy(h);
}

static void words() {
  const char* pieces[] = {"\xE2\x96\x81he", "llo", "\xE2\x96\x81", "\xE2", "\xE2\x96", "", "\xC3\xA9", "<blank>"};
  const int vocab = 8, blank = 7;
  std::mt19937 rng(2);
  for (int i = 0; i < 3000; ++i) {
    const int n = (int)(rng() % 12);
    std::vector<int> steps((size_t)3 * n);      // exactly 3 n ints
    for (int s = 0; s < n; ++s) {
      const unsigned r = rng();
      steps[(size_t)3 * s] = (r & 15) == 0 ? (int)(r >> 4) - (1 << 27) : (int)(r % vocab);      // now and then a token outside the vocabulary
      steps[(size_t)3 * s + 1] = (r & 0x30) == 0x30 ? INT32_MAX - (int)(r % 3) : (int)((r >> 8) % 40);
      steps[(size_t)3 * s + 2] = (r & 0xc0) == 0xc0 ? INT32_MAX : (int)((r >> 16) % 5);
    }
    long need = -1;
    const long w = crispy_pk_tdt_words(steps.data(), n, 30, blank, pieces, vocab, 0.08, nullptr, nullptr, nullptr, 0, nullptr, 0, &need);
    if (w < 0) continue;      // a hostile token: refused
    EXPECT(w <= n && need >= w);
    std::vector<float> start((size_t)w), end((size_t)w);      // exactly the sizes asked for
    std::vector<long> off((size_t)w);
    std::vector<char> text((size_t)need);
    EXPECT(crispy_pk_tdt_words(steps.data(), n, 30, blank, pieces, vocab, 0.08, start.data(), end.data(), off.data(), (int)w, text.data(), need, nullptr) == w);
    for (long k = 0; k < w; ++k) EXPECT(off[(size_t)k] >= 0 && off[(size_t)k] < need && end[(size_t)k] <= 30 * 0.08f + 1e-6f);
    if (w > 0) {      // one short of either size: the sizes come back and nothing is written
      char canary = 0x5a;
      EXPECT(crispy_pk_tdt_words(steps.data(), n, 30, blank, pieces, vocab, 0.08, start.data(), end.data(), off.data(), (int)w - 1, &canary, 0, &need) == w && canary == 0x5a);
    }
  }
  EXPECT(crispy_pk_tdt_words(nullptr, 0, 0, blank, pieces, vocab, 0.08, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) == 0);
  EXPECT(crispy_pk_tdt_words(nullptr, 3, 0, blank, pieces, vocab, 0.08, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr) == CRISPY_ERR_INVALID_ARG);
}

int main() {
  configs_and_budgets();
  load_and_call();
  words();
  std::printf("pk_tdt_harness: %d failures\n", failures);
  return failures ? 1 : 0;
}

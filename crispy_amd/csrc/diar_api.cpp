// diar_api.cpp -- host side of the speaker clustering (include/crispy_hip.h, "Speaker clustering and diarized text"):
// the crispy_diar handle, the turns and the solver loop of crispy_diar_cluster*, the stage entry points, and the host
// functions that need no device (chunk plan, speaker segments, find speaker, diarized text).
// Reference: src-tauri/src/managers/diarization.rs:276-724.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "api_util.h"
#include "diar_internal.h"

using crispy::DevBuf;
using crispy::fail;
using namespace crispy::diar;

namespace {

int p_max_of(int n) { return std::min(n - 1, std::max((int)std::sqrt((double)n), 2) * 2); }

// Solves every matrix of `descs` (host copies; pointers are device memory) on `st`: the LDS form for n <= kLdsN, the
// global form above, side by side.  Returns after the results are in place.
int solve(crispy_diar* h, std::vector<EigDesc>& descs, hipStream_t st) {
  std::vector<EigDesc> small, large;
  bool vectors = false;
  int max_n = 0;
  for (EigDesc d : descs) {
    d.status = 1;
    d.active = 1;
    if (d.n <= kLdsN) small.push_back(d);
    else { large.push_back(d); max_n = std::max(max_n, d.n); vectors |= d.V != nullptr; }
  }
  const size_t ns = small.size(), nl = large.size();
  HIP_TRY(h->descs.grow(256 + (ns + nl) * sizeof(EigDesc)));
  int* d_counter = h->descs.as<int>();
  EigDesc* d_small = reinterpret_cast<EigDesc*>(h->descs.p + 256);
  EigDesc* d_large = d_small + ns;
  if (ns) HIP_TRY(hipMemcpyAsync(d_small, small.data(), ns * sizeof(EigDesc), hipMemcpyHostToDevice, st));
  if (nl) HIP_TRY(hipMemcpyAsync(d_large, large.data(), nl * sizeof(EigDesc), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_eig_init(d_small, (int)(ns + nl), st));
  if (ns) HIP_TRY(launch_eig_lds(d_small, (int)ns, st));
  if (nl) {
    const int steps = rr_steps(max_n);
    for (int sweep = 0;; ++sweep) {
      int n_active = 0;
      HIP_TRY(hipMemsetAsync(d_counter, 0, sizeof(int), st));
      HIP_TRY(launch_eig_norm(d_large, (int)nl, d_counter, st));
      HIP_TRY(hipMemcpyAsync(&n_active, d_counter, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (n_active == 0) break;
      if (sweep > kMaxSweeps)
        return fail(CRISPY_ERR_INTERNAL, "crispy_diar: %d matrices (order up to %d) not diagonal after %d Jacobi sweeps", n_active,
                    max_n, kMaxSweeps);
      for (int t = 0; t < steps; ++t) HIP_TRY(launch_eig_step(d_large, (int)nl, max_n, vectors, t, st));
    }
  }
  HIP_TRY(launch_eig_sort(d_small, (int)(ns + nl), st));
  if (ns) {
    HIP_TRY(hipMemcpyAsync(small.data(), d_small, ns * sizeof(EigDesc), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (const EigDesc& d : small)
      if (d.status != 0)
        return fail(CRISPY_ERR_INTERNAL, "crispy_diar: a matrix of order %d not diagonal after %d Jacobi sweeps", d.n, kMaxSweeps);
  }
  return CRISPY_OK;
}

struct Rec {
  int index, n, kmax, p_max;
  size_t row0;
  float *aff, *dinv, *laps, *evals, *cs, *V, *evecs, *pts, *centers;
  unsigned short *rank, *sym;
};

void carve_rec(Carve& c, Rec& r) {
  const size_t n = r.n, nn = n * n, pm = r.p_max;
  r.aff = c.take<float>(nn);
  r.rank = c.take<unsigned short>(nn);
  r.sym = c.take<unsigned short>(nn);
  r.dinv = c.take<float>(pm * n);
  r.laps = c.take<float>((pm + 1) * nn);      // the sweep's, then the one at p*
  r.evals = c.take<float>((pm + 1) * n);
  r.cs = c.take<float>((pm + 1) * (3 * (n / 2 + 1)));
  r.V = c.take<float>(nn);
  r.evecs = c.take<float>(nn);
  r.pts = c.take<float>(n * r.kmax);
  r.centers = c.take<float>((size_t)r.kmax * r.kmax);
}

int cluster_turn(crispy_diar* h, std::vector<Rec>& recs, const float* d_emb, int dim, int* d_labels, crispy_diar_info* d_infos,
                 std::vector<crispy_diar_info>& infos, hipStream_t st) {
  Carve size;
  for (Rec r : recs) carve_rec(size, r);
  HIP_TRY(h->scratch.grow(size.used));
  Carve c;
  c.p = h->scratch.p;
  std::vector<EigDesc> eig;
  std::vector<ClusterDesc> cds;
  for (Rec& r : recs) {
    carve_rec(c, r);
    const size_t n = r.n, nn = n * n;
    HIP_TRY(launch_affinity(d_emb + r.row0 * dim, r.n, dim, r.aff, st));
    HIP_TRY(launch_rank(r.aff, r.n, r.rank, r.sym, st));
    HIP_TRY(launch_laplacians(r.aff, r.sym, r.n, 1, r.p_max, r.dinv, r.laps, st));
    for (int p = 1; p <= r.p_max; ++p)
      eig.push_back(EigDesc{r.laps + (p - 1) * nn, nullptr, r.cs + (size_t)(p - 1) * (3 * (n / 2 + 1)), r.evals + (p - 1) * n, nullptr, r.n, 1, 1, 0});
    cds.push_back(ClusterDesc{r.evals, r.evecs, r.pts, r.centers, d_labels + r.row0, r.n, r.kmax, r.p_max, r.index});
  }
  int rc = solve(h, eig, st);
  if (rc != CRISPY_OK) return rc;
  // the descriptors of the recordings live behind the solver's lists
  const size_t off = 256 + ((eig.size() * sizeof(EigDesc) + 255) & ~(size_t)255);
  HIP_TRY(h->descs.grow(off + cds.size() * sizeof(ClusterDesc)));
  ClusterDesc* d_cds = reinterpret_cast<ClusterDesc*>(h->descs.p + off);
  HIP_TRY(hipMemcpyAsync(d_cds, cds.data(), cds.size() * sizeof(ClusterDesc), hipMemcpyHostToDevice, st));
  HIP_TRY(launch_decide(d_cds, (int)cds.size(), d_infos, st));
  for (const Rec& r : recs)
    HIP_TRY(hipMemcpyAsync(&infos[r.index], d_infos + r.index, sizeof(crispy_diar_info), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  eig.clear();
  for (const Rec& r : recs) {
    if (infos[r.index].k <= 1) continue;
    const size_t n = r.n, nn = n * n, pm = r.p_max;
    HIP_TRY(launch_laplacians(r.aff, r.sym, r.n, infos[r.index].p_star, 1, r.dinv, r.laps + pm * nn, st));
    eig.push_back(EigDesc{r.laps + pm * nn, r.V, r.cs + pm * (3 * (n / 2 + 1)), r.evals + pm * n, r.evecs, r.n, 1, 1, 0});
  }
  if (!eig.empty()) {
    rc = solve(h, eig, st);      // (a shorter list than the sweep's: the recordings' descriptors behind it stay)
    if (rc != CRISPY_OK) return rc;
  }
  HIP_TRY(launch_kmeans(d_cds, (int)cds.size(), d_infos, st));
  return CRISPY_OK;
}

int check_cluster_args(const char* who, crispy_diar* h, const float* emb, const int* n, int batch, int dim, int* labels) {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL handle", who);
  if (!n) return fail(CRISPY_ERR_INVALID_ARG, "%s: n is NULL", who);
  if (batch < 1 || batch > kMaxBatch) return fail(CRISPY_ERR_INVALID_ARG, "%s: batch %d outside 1 ... %d", who, batch, kMaxBatch);
  if (dim < 1 || dim > kMaxDim) return fail(CRISPY_ERR_INVALID_ARG, "%s: dim %d outside 1 ... %d", who, dim, kMaxDim);
  size_t total = 0;
  for (int r = 0; r < batch; ++r) {
    if (n[r] < 0 || n[r] > kMaxN) return fail(CRISPY_ERR_INVALID_ARG, "%s: n[%d] = %d outside 0 ... %d", who, r, n[r], kMaxN);
    total += (size_t)n[r];
  }
  if (total > 0 && (!emb || !labels)) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL embeddings or labels", who);
  return CRISPY_OK;
}

// nme_sc of `batch` recordings on device pointers; complete on return.
int cluster_device(crispy_diar* h, const float* d_emb, const int* n, int batch, int dim, int max_speakers, int* d_labels,
                   crispy_diar_info* info, hipStream_t st, bool check_finite) {
  std::vector<crispy_diar_info> infos((size_t)batch);
  std::vector<Rec> all;
  size_t total = 0;
  for (int r = 0; r < batch; ++r) {
    infos[r] = crispy_diar_info{0, n[r] > 0 ? 1 : 0, 0.0f, 0.0f, 0};
    if (n[r] > 2) {
      Rec rec{};
      rec.index = r;
      rec.n = n[r];
      rec.kmax = std::min(std::max(max_speakers, 1), n[r] - 1);
      rec.p_max = p_max_of(n[r]);
      rec.row0 = total;
      all.push_back(rec);
    }
    total += (size_t)n[r];
  }
  if (total == 0) {
    if (info) std::memcpy(info, infos.data(), infos.size() * sizeof(crispy_diar_info));
    return CRISPY_OK;
  }
  HIP_TRY(h->descs.grow(4096));
  if (check_finite) {
    int* d_flag = reinterpret_cast<int*>(h->descs.p + 128);
    int flag = 0;
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), st));
    HIP_TRY(launch_nonfinite(d_emb, total * dim, d_flag, st));
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (flag) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_cluster_device: a non-finite embedding value");
  }
  HIP_TRY(hipMemsetAsync(d_labels, 0, total * sizeof(int), st));
  HIP_TRY(h->infos.grow((size_t)kMaxBatch * sizeof(crispy_diar_info)));
  crispy_diar_info* d_infos = h->infos.as<crispy_diar_info>();
  HIP_TRY(hipMemcpyAsync(d_infos, infos.data(), infos.size() * sizeof(crispy_diar_info), hipMemcpyHostToDevice, st));
  size_t i = 0;
  while (i < all.size()) {      // turns of consecutive recordings whose scratch stays below the cap
    std::vector<Rec> turn;
    Carve size;
    while (i < all.size()) {
      Rec probe = all[i];
      Carve next = size;
      carve_rec(next, probe);
      if (!turn.empty() && next.used > kScratchCap) break;
      size = next;
      turn.push_back(all[i++]);
    }
    const int rc = cluster_turn(h, turn, d_emb, dim, d_labels, d_infos, infos, st);
    if (rc != CRISPY_OK) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (info) std::memcpy(info, infos.data(), infos.size() * sizeof(crispy_diar_info));
  return CRISPY_OK;
}

// ---- host functions -------------------------------------------------------------------------------------------------
std::string speaker_name(int s) { return s == 0 ? std::string("Speaker ?") : "Speaker " + std::to_string(s); }

int find_speaker(double time, const double* s0, const double* s1, const int* who, long n) {
  for (long i = 0; i < n; ++i)
    if (time >= s0[i] && time <= s1[i]) return who[i];
  int closest = 0;
  double min_dist = 1.7976931348623157e308;      // f64::MAX
  for (long i = 0; i < n; ++i) {
    const double dist = time < s0[i] ? s0[i] - time : time - s1[i];
    if (dist < min_dist) { min_dist = dist; closest = who[i]; }
  }
  return closest;
}

// Rust's `{:.1}` of an f64: the exact decimal value rounded half to even, which is what printf's %.1f gives; the
// decimal point is written here, whatever the host's locale.
std::string fmt_1(double v) {
  if (std::isnan(v)) return "NaN";
  if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
  char buf[400];
  const int len = std::snprintf(buf, sizeof buf, "%.1f", v);
  if (len < 3 || len >= (int)sizeof buf) return "NaN";
  buf[len - 2] = '.';
  return std::string(buf, (size_t)len);
}

struct WordRef { double t0, t1; const char* text; };

std::string format_text(const std::vector<WordRef>& words, const double* s0, const double* s1, const int* who, long n_segs) {
  std::string out;
  if (n_segs == 0 || words.empty()) {
    for (size_t i = 0; i < words.size(); ++i) {
      if (i) out += ' ';
      out += words[i].text;
    }
    return out;
  }
  std::vector<std::string> lines;
  bool have = false;
  int current = 0;
  std::string line;
  bool line_has = false;
  for (const WordRef& w : words) {
    const std::string t = crispy::trim_unicode(w.text);
    if (t.empty()) continue;
    const int sp = find_speaker((w.t0 + w.t1) / 2.0, s0, s1, who, n_segs);
    if (!have || sp != current) {
      if (line_has) { lines.push_back(line); line.clear(); line_has = false; }
      have = true;
      current = sp;
      lines.push_back("\n[" + speaker_name(sp) + "|" + fmt_1(w.t0) + "]");
    }
    if (line_has) line += ' ';
    line += t;
    line_has = true;
  }
  if (line_has) lines.push_back(line);
  for (size_t i = 0; i < lines.size(); ++i) {
    if (i) out += '\n';
    out += lines[i];
  }
  return crispy::trim_unicode(out);
}

int give_text(const char* who, const std::string& s, char* out, size_t cap, size_t* needed) {
  if (needed) *needed = s.size() + 1;
  if (!out || cap < s.size() + 1) {
    if (out && cap) out[0] = '\0';
    if (!out && cap == 0 && needed) return CRISPY_OK;      // the sizing call
    return fail(CRISPY_ERR_INVALID_ARG, "%s: the text takes %zu bytes, the buffer has %zu", who, s.size() + 1, out ? cap : (size_t)0);
  }
  std::memcpy(out, s.c_str(), s.size() + 1);
  return CRISPY_OK;
}

int check_segs(const char* who, const double* s0, const double* s1, const int* sp, long n) {
  if (n < 0) return fail(CRISPY_ERR_INVALID_ARG, "%s: n_segments < 0", who);
  if (n > 0 && (!s0 || !s1 || !sp)) return fail(CRISPY_ERR_INVALID_ARG, "%s: NULL speaker segments", who);
  return CRISPY_OK;
}

}  // namespace

extern "C" {

int crispy_diar_create(int device, void** out) try {
  if (!out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_create: out is NULL");
  *out = nullptr;
  const int rc = crispy::check_device(device, "crispy_diar_create");
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  crispy_diar* h = new crispy_diar;
  h->device = device;
  const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    h->stream = nullptr;
    delete h;
    return fail(CRISPY_ERR_HIP, "crispy_diar_create: hipStreamCreate: %s", hipGetErrorString(e));
  }
  *out = h;
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_create")

void crispy_diar_destroy(void* hv) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  delete h;
}
CRISPY_CATCH_VOID("crispy_diar_destroy")

int crispy_diar_cluster_device(void* hv, const float* d_emb, const int* n, int batch, int dim, int max_speakers, int* d_labels,
                               void* info, void* hip_stream) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  const int rc = check_cluster_args("crispy_diar_cluster_device", h, d_emb, n, batch, dim, d_labels);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipSetDevice(h->device));
  return cluster_device(h, d_emb, n, batch, dim, max_speakers, d_labels, static_cast<crispy_diar_info*>(info),
                        hip_stream ? static_cast<hipStream_t>(hip_stream) : h->stream, true);
}
CRISPY_CATCH_RET("crispy_diar_cluster_device")

int crispy_diar_cluster(void* hv, const float* emb, const int* n, int batch, int dim, int max_speakers, int* labels, void* info) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  const int rc = check_cluster_args("crispy_diar_cluster", h, emb, n, batch, dim, labels);
  if (rc != CRISPY_OK) return rc;
  size_t total = 0;
  for (int r = 0; r < batch; ++r) total += (size_t)n[r];
  for (size_t e = 0; e < total * dim; ++e)
    if (!std::isfinite(emb[e]))
      return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_cluster: embedding value %zu of row %zu is not finite", e % dim, e / dim);
  HIP_TRY(hipSetDevice(h->device));
  const size_t emb_bytes = (total * dim * sizeof(float) + 255) & ~(size_t)255;
  HIP_TRY(h->io.grow(emb_bytes + total * sizeof(int) + 256));
  float* d_emb = h->io.as<float>();
  int* d_labels = reinterpret_cast<int*>(h->io.p + emb_bytes);
  if (total) HIP_TRY(hipMemcpyAsync(d_emb, emb, total * dim * sizeof(float), hipMemcpyHostToDevice, h->stream));
  const int rc2 = cluster_device(h, d_emb, n, batch, dim, max_speakers, d_labels, static_cast<crispy_diar_info*>(info), h->stream, false);
  if (rc2 != CRISPY_OK) return rc2;
  if (total) {
    HIP_TRY(hipMemcpyAsync(labels, d_labels, total * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_cluster")

int crispy_diar_affinity_device(void* hv, const float* d_emb, int n, int dim, float* d_aff) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h || !d_emb || !d_aff) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_affinity_device: NULL handle or pointer");
  if (n < 1 || n > kMaxN || dim < 1 || dim > kMaxDim)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_affinity_device: n %d outside 1 ... %d or dim %d outside 1 ... %d", n, kMaxN, dim, kMaxDim);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(launch_affinity(d_emb, n, dim, d_aff, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_affinity_device")

int crispy_diar_laplacian_device(void* hv, const float* d_aff, int n, int p, float* d_lap) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h || !d_aff || !d_lap) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_laplacian_device: NULL handle or pointer");
  if (n < 1 || n > kMaxN || p < 1) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_laplacian_device: n %d outside 1 ... %d or p %d < 1", n, kMaxN, p);
  HIP_TRY(hipSetDevice(h->device));
  Carve c;
  const size_t nn = (size_t)n * n;
  c.take<unsigned short>(nn); c.take<unsigned short>(nn); c.take<float>(n);
  HIP_TRY(h->scratch.grow(c.used));
  c = Carve{h->scratch.p, 0};
  unsigned short* rank = c.take<unsigned short>(nn);
  unsigned short* sym = c.take<unsigned short>(nn);
  float* dinv = c.take<float>(n);
  HIP_TRY(launch_rank(d_aff, n, rank, sym, h->stream));
  HIP_TRY(launch_laplacians(d_aff, sym, n, std::min(p, kMaxN), 1, dinv, d_lap, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_laplacian_device")

int crispy_diar_eigh_device(void* hv, const float* d_mats, int n, int n_mats, float* d_evals, float* d_evecs) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h || !d_mats || !d_evals) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_eigh_device: NULL handle or pointer");
  if (n < 1 || n > kMaxN || n_mats < 1) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_eigh_device: n %d outside 1 ... %d or n_mats %d < 1", n, kMaxN, n_mats);
  const size_t nn = (size_t)n * n, per = nn * sizeof(float) * (d_evecs ? 2 : 1);
  if ((size_t)n_mats > kScratchCap / per)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_eigh_device: %d matrices of order %d take more than the 2 GB of scratch", n_mats, n);
  HIP_TRY(hipSetDevice(h->device));
  Carve c;
  c.take<float>(nn * n_mats); c.take<float>((size_t)(3 * (n / 2 + 1)) * n_mats); if (d_evecs) c.take<float>(nn * n_mats);
  HIP_TRY(h->scratch.grow(c.used));
  c = Carve{h->scratch.p, 0};
  float* A = c.take<float>(nn * n_mats);
  float* cs = c.take<float>((size_t)(3 * (n / 2 + 1)) * n_mats);
  float* V = d_evecs ? c.take<float>(nn * n_mats) : nullptr;
  HIP_TRY(hipMemcpyAsync(A, d_mats, nn * n_mats * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  std::vector<EigDesc> descs;
  for (size_t m = 0; m < (size_t)n_mats; ++m)
    descs.push_back(EigDesc{A + m * nn, V ? V + m * nn : nullptr, cs + m * (3 * (n / 2 + 1)), d_evals + m * n, d_evecs ? d_evecs + m * nn : nullptr, n, 1, 1, 0});
  const int rc = solve(h, descs, h->stream);
  if (rc != CRISPY_OK) { (void)hipStreamSynchronize(h->stream); return rc; }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_eigh_device")

int crispy_diar_decide_device(void* hv, const float* d_evals, int n, int p_max, int max_speakers, void* info) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h || !info) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_decide_device: NULL handle or info");
  if (n < 0 || n > kMaxN || p_max < 0 || p_max > kMaxN)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_decide_device: n %d or p_max %d outside 0 ... %d", n, p_max, kMaxN);
  crispy_diar_info out{0, n > 0 ? 1 : 0, 0.0f, 0.0f, 0};
  if (n > 2 && p_max > 0) {
    if (!d_evals) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_decide_device: NULL eigenvalues");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->descs.grow(4096));
    HIP_TRY(h->infos.grow((size_t)kMaxBatch * sizeof(crispy_diar_info)));
    const ClusterDesc cd{d_evals, nullptr, nullptr, nullptr, nullptr, n, std::min(std::max(max_speakers, 1), n - 1), p_max, 0};
    ClusterDesc* d_cd = reinterpret_cast<ClusterDesc*>(h->descs.p + 256);
    crispy_diar_info* d_infos = h->infos.as<crispy_diar_info>();
    HIP_TRY(hipMemcpyAsync(d_cd, &cd, sizeof cd, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(d_infos, &out, sizeof out, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_decide(d_cd, 1, d_infos, h->stream));
    HIP_TRY(hipMemcpyAsync(&out, d_infos, sizeof out, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  std::memcpy(info, &out, sizeof out);
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_decide_device")

int crispy_diar_kmeans_device(void* hv, const float* d_vecs, int n, int k, int* d_labels, float* d_points, float* d_centers) try {
  crispy_diar* h = static_cast<crispy_diar*>(hv);
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_kmeans_device: NULL handle");
  if (n < 0 || n > kMaxN || k < 1) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_kmeans_device: n %d outside 0 ... %d or k %d < 1", n, kMaxN, k);
  if (n == 0) return CRISPY_OK;
  if (!d_vecs || !d_labels) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_kmeans_device: NULL vectors or labels");
  HIP_TRY(hipSetDevice(h->device));
  const size_t kk = k < n ? (size_t)k : 0;      // k >= n reads no point and keeps no centre
  Carve c;
  c.take<float>((size_t)n * kk); c.take<float>(kk * kk);
  HIP_TRY(h->scratch.grow(c.used));
  c = Carve{h->scratch.p, 0};
  float* pts = c.take<float>((size_t)n * kk);
  float* centers = c.take<float>(kk * kk);
  HIP_TRY(h->descs.grow(4096));
  HIP_TRY(h->infos.grow((size_t)kMaxBatch * sizeof(crispy_diar_info)));
  const ClusterDesc cd{nullptr, d_vecs, d_points ? d_points : pts, d_centers ? d_centers : centers, d_labels, n, k, 0, 0};
  const crispy_diar_info in{0, k, 0.0f, 0.0f, 0};
  ClusterDesc* d_cd = reinterpret_cast<ClusterDesc*>(h->descs.p + 256);
  crispy_diar_info* d_infos = h->infos.as<crispy_diar_info>();
  HIP_TRY(hipMemcpyAsync(d_cd, &cd, sizeof cd, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(d_infos, &in, sizeof in, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(launch_kmeans(d_cd, 1, d_infos, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
}
CRISPY_CATCH_RET("crispy_diar_kmeans_device")

long crispy_diar_chunk_plan(const double* start, const double* end, const long* n_samples, long n_segments, int sample_rate,
                            double* out_start, double* out_end, long* out_segment, long* out_first, long* out_len, long cap) try {
  if (n_segments < 0 || cap < 0 || sample_rate <= 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_chunk_plan: negative count or sample_rate <= 0");
  if (n_segments > 0 && (!start || !end || !n_samples)) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_chunk_plan: NULL segments");
  if (cap > 0 && (!out_start || !out_end || !out_segment || !out_first || !out_len))
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_chunk_plan: NULL output with cap > 0");
  const double max_dur = 4.0, rate = (double)sample_rate;
  long count = 0;
  auto put = [&](double s, double e, long seg, long first, long len) {
    if (count < cap) { out_start[count] = s; out_end[count] = e; out_segment[count] = seg; out_first[count] = first; out_len[count] = len; }
    ++count;
  };
  for (long i = 0; i < n_segments; ++i) {
    if (!std::isfinite(start[i]) || !std::isfinite(end[i]) || n_samples[i] < 0)
      return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_chunk_plan: segment %ld has a non-finite time or a negative length", i);
    const double dur = end[i] - start[i];
    if (dur > max_dur) {
      const double fc = std::ceil(dur / max_dur);
      if (!(fc < 1e9)) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_chunk_plan: segment %ld lasts %g s", i, dur);
      const long chunks = (long)fc, chunk_samples = n_samples[i] / chunks;
      for (long c = 0; c < chunks; ++c) {
        const long a = c * chunk_samples, b = c == chunks - 1 ? n_samples[i] : (c + 1) * chunk_samples;
        put(start[i] + (double)a / rate, start[i] + (double)b / rate, i, a, b - a);
      }
    } else {
      put(start[i], end[i], i, 0, n_samples[i]);
    }
  }
  return count;
}
CRISPY_CATCH_RET("crispy_diar_chunk_plan")

long crispy_diar_speaker_segments(const double* start, const double* end, const int* labels, long n, double merge_gap,
                                  double* out_start, double* out_end, int* out_speaker, long cap) try {
  if (n < 0 || cap < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_speaker_segments: negative count");
  if (n > 0 && (!start || !end || !labels)) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_speaker_segments: NULL segments");
  if (cap > 0 && (!out_start || !out_end || !out_speaker)) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_speaker_segments: NULL output with cap > 0");
  for (long i = 0; i < n; ++i)
    if (std::isnan(start[i])) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_speaker_segments: start[%ld] is NaN", i);
  std::vector<int> order;      // labels in order of first appearance
  struct Seg { double s, e; int who; };
  std::vector<Seg> segs;
  for (long i = 0; i < n; ++i) {
    size_t k = 0;
    while (k < order.size() && order[k] != labels[i]) ++k;
    if (k == order.size()) order.push_back(labels[i]);
    segs.push_back(Seg{start[i], end[i], (int)k + 1});
  }
  std::stable_sort(segs.begin(), segs.end(), [](const Seg& a, const Seg& b) { return a.s < b.s; });
  std::vector<Seg> merged;
  for (const Seg& s : segs) {
    if (!merged.empty()) {
      Seg& last = merged.back();
      const double gap = std::fmax(s.s - last.e, 0.0);
      if (last.who == s.who && gap <= merge_gap) {
        last.e = std::fmax(s.e, last.e);
        continue;
      }
    }
    merged.push_back(s);
  }
  for (size_t i = 0; i < merged.size() && (long)i < cap; ++i) { out_start[i] = merged[i].s; out_end[i] = merged[i].e; out_speaker[i] = merged[i].who; }
  return (long)merged.size();
}
CRISPY_CATCH_RET("crispy_diar_speaker_segments")

int crispy_diar_find_speaker(double time, const double* seg_start, const double* seg_end, const int* seg_speaker, long n_segments) try {
  const int rc = check_segs("crispy_diar_find_speaker", seg_start, seg_end, seg_speaker, n_segments);
  if (rc != CRISPY_OK) return rc;
  return find_speaker(time, seg_start, seg_end, seg_speaker, n_segments);
}
CRISPY_CATCH_RET("crispy_diar_find_speaker")

int crispy_diar_format_text(const double* t0, const double* t1, const char* const* text, long n_words, const double* seg_start,
                            const double* seg_end, const int* seg_speaker, long n_segments, char* out, size_t cap, size_t* needed) try {
  if (n_words < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_format_text: n_words < 0");
  if (n_words > 0 && (!t0 || !t1 || !text)) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_format_text: NULL words");
  const int rc = check_segs("crispy_diar_format_text", seg_start, seg_end, seg_speaker, n_segments);
  if (rc != CRISPY_OK) return rc;
  std::vector<WordRef> words;
  for (long i = 0; i < n_words; ++i) {
    if (!text[i]) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_format_text: text[%ld] is NULL", i);
    words.push_back(WordRef{t0[i], t1[i], text[i]});
  }
  return give_text("crispy_diar_format_text", format_text(words, seg_start, seg_end, seg_speaker, n_segments), out, cap, needed);
}
CRISPY_CATCH_RET("crispy_diar_format_text")

int crispy_diar_format_result(const crispy_asr_result* r, double chunk_offset, const double* seg_start, const double* seg_end,
                              const int* seg_speaker, long n_segments, char* out, size_t cap, size_t* needed) try {
  if (!r) return fail(CRISPY_ERR_INVALID_ARG, "crispy_diar_format_result: NULL result");
  const int rc = check_segs("crispy_diar_format_result", seg_start, seg_end, seg_speaker, n_segments);
  if (rc != CRISPY_OK) return rc;
  const crispy_asr_word* w = static_cast<const crispy_asr_word*>(r->words);
  std::vector<WordRef> words;
  for (int i = 0; w && i < r->n_words; ++i)
    words.push_back(WordRef{chunk_offset + (double)w[i].t0, chunk_offset + (double)w[i].t1, w[i].text ? w[i].text : ""});
  return give_text("crispy_diar_format_result", format_text(words, seg_start, seg_end, seg_speaker, n_segments), out, cap, needed);
}
CRISPY_CATCH_RET("crispy_diar_format_result")

}  // extern "C"

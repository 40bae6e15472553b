// whisper_api.cpp -- the Whisper model container behind include/crispy_hip.h: tensors by their model-file names and the copies
// derived from them (fused rows, LayerNorm folds, f16 operands of precision mode 1, packed operands of the fused decode step),
// the precision modes, the encoder, the workspaces.  Replaces transcribe_rs::whisper_cpp::WhisperEngine::{load, transcribe}
// together with ggml_load.cpp, decode_steps.cpp and whisper_full.cpp (reference: src-tauri/src/managers/transcription.rs:138-141,
// 183-185).
#include "whisper_internal.h"

using namespace crispy;
using namespace crispy::asr;

namespace crispy {
namespace asr {
namespace {

void add_spec(std::map<std::string, size_t>& spec, const std::string& name, size_t n) { spec[name] = n; }

// Every copy the handle derives from its tensors is made here: n bytes of device memory that the handle owns until it is freed
int derived_copy(crispy_asr* h, size_t n, void** out) {
  DevBuf<void> b;
  HIP_TRY(b.alloc(n));
  *out = b.p;
  h->derived.push_back(std::move(b));
  return CRISPY_OK;
}

int upload(crispy_asr* h, const std::vector<float>& host, const float** out) {
  void* d = nullptr;
  const int rc = derived_copy(h, host.size() * sizeof(float), &d);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = static_cast<const float*>(d);
  return CRISPY_OK;
}

// f16 copy of n floats, converted on the handle's stream
int half_copy(crispy_asr* h, const float* w, size_t n, const void** out) {
  void* p = nullptr;
  const int rc = derived_copy(h, n * 2, &p);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(convert_f32_to_f16(w, p, (long)n, h->stream));
  *out = p;
  return CRISPY_OK;
}

// n halves once more in the fused step kernels' operand order
int packed_copy(crispy_asr* h, const void* src, size_t n, int kind, const void** out) {
  void* p = nullptr;
  const int rc = derived_copy(h, n * 2, &p);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(fused_pack_weights(src, p, h->hp.n_text_state, kind, h->stream));
  *out = p;
  return CRISPY_OK;
}

// a tensor by its model-file name; an unknown name is reported, never inserted
Tensor* find_tensor(crispy_asr* h, const std::string& name) {
  const auto it = h->tensors.find(name);
  if (it != h->tensors.end()) return &it->second;
  fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_finalize: unknown tensor '%s'", name.c_str());
  return nullptr;
}

// T(name): the tensor's device pointer; the first unknown name stays in rc, which the caller returns after its look-ups
struct Resolver {
  crispy_asr* h;
  int rc = CRISPY_OK;
  const float* operator()(const std::string& name) {
    const Tensor* t = rc == CRISPY_OK ? find_tensor(h, name) : nullptr;
    if (!t) { if (rc == CRISPY_OK) rc = CRISPY_ERR_BAD_MODEL; return nullptr; }
    return t->d;
  }
};

int download(crispy_asr* h, const std::string& name, std::vector<float>& host) {
  const Tensor* t = find_tensor(h, name);
  if (!t) return CRISPY_ERR_BAD_MODEL;
  host.resize(t->n);
  HIP_TRY(hipMemcpy(host.data(), t->d, t->n * sizeof(float), hipMemcpyDeviceToHost));
  return CRISPY_OK;
}

// [co][ci][3] -> [co][kk*ci_n + ci]: K order (tap, channel) matches three consecutive frame-major rows
int reorder_conv(crispy_asr* h, const std::string& name, int co_n, int ci_n, const float** out) {
  std::vector<float> src, dst((size_t)co_n * ci_n * 3);
  int rc = download(h, name, src);
  if (rc != CRISPY_OK) return rc;
  for (int co = 0; co < co_n; ++co)
    for (int ci = 0; ci < ci_n; ++ci)
      for (int kk = 0; kk < 3; ++kk) dst[((size_t)co * 3 + kk) * ci_n + ci] = src[((size_t)co * ci_n + ci) * 3 + kk];
  return upload(h, dst, out);
}

QRef qref(crispy_asr* h, std::initializer_list<std::string> names) {
  QRef r;
  for (const std::string& n : names) r.t[r.n++] = &h->qtensors[n];
  return r;
}

// concatenated biases of row-fused weights (a missing bias is zeros)
int fuse_bias(crispy_asr* h, const std::vector<std::string>& bnames, int d, const float** b_out) {
  std::vector<float> Bv;
  for (const std::string& b : bnames) {
    if (!b.empty()) {
      std::vector<float> t;
      const int rc = download(h, b, t);
      if (rc != CRISPY_OK) return rc;
      Bv.insert(Bv.end(), t.begin(), t.end());
    } else {
      Bv.insert(Bv.end(), (size_t)d, 0.f);
    }
  }
  return upload(h, Bv, b_out);
}

// concatenate row blocks of [d][d] weights (and biases: fuse_bias)
int fuse_rows(crispy_asr* h, const std::vector<std::string>& wnames, const std::vector<std::string>& bnames, int d,
              const float** w_out, const float** b_out) {
  std::vector<float> W;
  for (const std::string& w : wnames) {
    std::vector<float> t;
    const int rc = download(h, w, t);
    if (rc != CRISPY_OK) return rc;
    W.insert(W.end(), t.begin(), t.end());
  }
  const int rc = upload(h, W, w_out);
  if (rc != CRISPY_OK) return rc;
  return fuse_bias(h, bnames, d, b_out);
}

// LayerNorm (gamma, beta over K) folded into W [N][K] (+ bias [N], may be null): see GemmArgs::ln_s
int fold_ln(crispy_asr* h, const float* d_w, const float* d_bias, const float* d_gamma, const float* d_beta, size_t N,
            size_t K, const float** lw, const float** ls, const float** lc) {
  std::vector<float> W(N * K), b(N, 0.f), g(K), be(K);
  HIP_TRY(hipMemcpy(W.data(), d_w, W.size() * sizeof(float), hipMemcpyDeviceToHost));
  if (d_bias) HIP_TRY(hipMemcpy(b.data(), d_bias, N * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(g.data(), d_gamma, K * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(be.data(), d_beta, K * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> s(N), c(N);
  for (size_t n = 0; n < N; ++n) {
    double ss = 0.0, cc = (double)b[n];
    float* row = W.data() + n * K;
    for (size_t k = 0; k < K; ++k) {
      cc += (double)be[k] * (double)row[k];
      row[k] *= g[k];
      ss += (double)row[k];
    }
    s[n] = (float)ss;
    c[n] = (float)cc;
  }
  int rc = upload(h, W, lw);
  if (rc == CRISPY_OK) rc = upload(h, s, ls);
  if (rc == CRISPY_OK) rc = upload(h, c, lc);
  return rc;
}
}  // namespace

std::map<std::string, size_t> expected_tensors(const crispy_asr_hparams& hp) {
  std::map<std::string, size_t> s;
  const size_t d = hp.n_audio_state, dt = hp.n_text_state;
  add_spec(s, "encoder.conv1.weight", d * hp.n_mels * 3);
  add_spec(s, "encoder.conv1.bias", d);
  add_spec(s, "encoder.conv2.weight", d * d * 3);
  add_spec(s, "encoder.conv2.bias", d);
  add_spec(s, "encoder.positional_embedding", (size_t)hp.n_audio_ctx * d);
  for (int i = 0; i < hp.n_audio_layer; ++i) {
    const std::string p = "encoder.blocks." + std::to_string(i) + ".";
    add_spec(s, p + "attn_ln.weight", d); add_spec(s, p + "attn_ln.bias", d);
    add_spec(s, p + "attn.query.weight", d * d); add_spec(s, p + "attn.query.bias", d);
    add_spec(s, p + "attn.key.weight", d * d);
    add_spec(s, p + "attn.value.weight", d * d); add_spec(s, p + "attn.value.bias", d);
    add_spec(s, p + "attn.out.weight", d * d); add_spec(s, p + "attn.out.bias", d);
    add_spec(s, p + "mlp_ln.weight", d); add_spec(s, p + "mlp_ln.bias", d);
    add_spec(s, p + "mlp.0.weight", 4 * d * d); add_spec(s, p + "mlp.0.bias", 4 * d);
    add_spec(s, p + "mlp.2.weight", 4 * d * d); add_spec(s, p + "mlp.2.bias", d);
  }
  add_spec(s, "encoder.ln_post.weight", d); add_spec(s, "encoder.ln_post.bias", d);
  add_spec(s, "decoder.token_embedding.weight", (size_t)hp.n_vocab * dt);
  add_spec(s, "decoder.positional_embedding", (size_t)hp.n_text_ctx * dt);
  for (int i = 0; i < hp.n_text_layer; ++i) {
    const std::string p = "decoder.blocks." + std::to_string(i) + ".";
    for (const char* a : {"attn", "cross_attn"}) {
      const std::string q = p + a;
      add_spec(s, q + "_ln.weight", dt); add_spec(s, q + "_ln.bias", dt);
      add_spec(s, q + ".query.weight", dt * dt); add_spec(s, q + ".query.bias", dt);
      add_spec(s, q + ".key.weight", dt * dt);
      add_spec(s, q + ".value.weight", dt * dt); add_spec(s, q + ".value.bias", dt);
      add_spec(s, q + ".out.weight", dt * dt); add_spec(s, q + ".out.bias", dt);
    }
    add_spec(s, p + "mlp_ln.weight", dt); add_spec(s, p + "mlp_ln.bias", dt);
    add_spec(s, p + "mlp.0.weight", 4 * dt * dt); add_spec(s, p + "mlp.0.bias", 4 * dt);
    add_spec(s, p + "mlp.2.weight", 4 * dt * dt); add_spec(s, p + "mlp.2.bias", dt);
  }
  add_spec(s, "decoder.ln.weight", dt); add_spec(s, "decoder.ln.bias", dt);
  return s;
}

// ---- resident quantised tensors (asr_quant.h) -----------------------------------------------------------------
// Dense copy of a (row-concatenated) resident tensor in the handle's scratch slot, enqueued on `s` right in front of
// its consumer: f16 (the operands of precision mode 1), f32, or f32 x gamma[k] (the LayerNorm-folded decode projections).
int dq(crispy_asr* h, const QRef& r, bool f16, const float* gamma, hipStream_t s, const void** out) {
  const size_t esz = f16 ? 2 : 4;
  if (r.n <= 0 || r.elems() * esz > h->q_scratch.bytes)
    return fail(CRISPY_ERR_INVALID_ARG, "resident model: tensor of %zu elements does not fit the de-quantisation slot", r.elems());
  char* dst = h->q_scratch.as<char>();
  for (int i = 0; i < r.n; ++i) {
    const QTensor& t = *r.t[i];
    HIP_TRY(dequant_blocks(t.d, t.ttype, (long)(t.n / 32), t.cols, dst, f16 ? 1 : 0, gamma, s));
    dst += t.n * esz;
  }
  *out = h->q_scratch.p;
  return CRISPY_OK;
}

// the captured steps hold the workspace's addresses: they go first
void free_dec_ws(crispy_asr* h) {
  h->drop_graphs();
  h->dw = DecWs{};
}

int upload_mask(DevBuf<unsigned char>& mask, const std::vector<unsigned char>& host) {
  HIP_TRY(mask.grow(host.size()));
  HIP_TRY(hipMemcpy(mask, host.data(), host.size(), hipMemcpyHostToDevice));
  return CRISPY_OK;
}

int reserve_enc(crispy_asr* h, int batch) {
  EncWs& w = h->ew;
  if (batch <= w.cap_batch) return CRISPY_OK;
  w = EncWs{};
  const size_t B = batch, d = h->hp.n_audio_state, Tn = h->hp.n_audio_ctx;
  HIP_TRY(w.melt.alloc(B * (MEL_FRAMES + 2) * h->hp.n_mels * sizeof(float)));
  HIP_TRY(w.h1.alloc(B * (MEL_FRAMES + 1) * d * sizeof(float)));
  HIP_TRY(w.x.alloc(B * Tn * d * sizeof(float)));
  HIP_TRY(w.xn.alloc(B * Tn * d * sizeof(float)));
  HIP_TRY(w.qkv.alloc(B * Tn * 3 * d * sizeof(float)));
  HIP_TRY(w.att.alloc(B * Tn * d * sizeof(float)));
  HIP_TRY(w.h.alloc(B * Tn * 4 * d * sizeof(float)));
  HIP_TRY(w.enc.alloc(B * Tn * d * sizeof(float)));
  // zero padding rows of the frame-major buffers are written once
  HIP_TRY(hipMemset(w.melt, 0, w.melt.bytes));
  HIP_TRY(hipMemset(w.h1, 0, w.h1.bytes));
  // hipMemset on device memory does not wait on the host, and it runs on the NULL stream, which the handle's
  // non-blocking stream is not ordered against: without this the 1.5 GB memset of a 256-clip workspace was still
  // clearing h1 while the first call's conv1 had already written the first clips (wrong encoder output for clips
  // 0..7 of the first 256-clip call, intermittently: tests/test_gpu_pipeline.py cfg5)
  HIP_TRY(hipDeviceSynchronize());
  w.cap_batch = batch;
  return CRISPY_OK;
}

// the PCM rows of the encoder workspace [cap_batch][stride] (after reserve_enc), regrown when a call's rows are longer
int reserve_pcm(crispy_asr* h, long stride) {
  EncWs& w = h->ew;
  if (w.pcm && stride <= w.cap_pcm_stride) return CRISPY_OK;
  HIP_TRY(w.pcm.alloc((size_t)w.cap_batch * stride * sizeof(float)));
  w.cap_pcm_stride = stride;
  return CRISPY_OK;
}

GemmArgs gemm(const float* A, long lda, const float* W, long ldw, float* C, long ldc, const float* bias, int M, int N,
              int K) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.bias = bias;
  g.M = M; g.N = N; g.K = K;
  return g;
}

}  // namespace asr
}  // namespace crispy

extern "C" {

int crispy_asr_create(const crispy_asr_hparams* hp, const float* mel_filters, int device, crispy_asr** out) try {
  if (!out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_create: out is NULL");
  *out = nullptr;
  if (!hp || !mel_filters) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_create: NULL argument");
  if (hp->n_audio_ctx != 1500 || !whisper_width_ok(hp->n_audio_state) || !whisper_width_ok(hp->n_text_state) ||
      // (divisions, not products: a hostile head count from a model file must not overflow -- found by the sanitizer
      // harness, tests/test_host_sanitizers.py)
      hp->n_audio_state % 64 != 0 || hp->n_audio_head != hp->n_audio_state / 64 || hp->n_text_head != hp->n_text_state / 64 ||
      hp->n_audio_layer <= 0 || hp->n_audio_layer > 64 || hp->n_text_layer <= 0 || hp->n_text_layer > 64 ||
      hp->n_text_ctx <= 0 || hp->n_text_ctx > 448 || hp->n_vocab <= 0 || (hp->n_mels != 80 && hp->n_mels != 128) ||
      (hp->n_mels * 3) % 16)
    return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_create: unsupported hyper-parameters (widths 384/512/768/1024/1280, head dim 64, ctx 1500/<=448)");
  int rc = check_device(device, "crispy_asr_create");
  if (rc != CRISPY_OK) return rc;
  crispy_asr* h = new (std::nothrow) crispy_asr();
  if (!h) return fail(CRISPY_ERR_OOM, "crispy_asr_create: host allocation failed");
  h->device = device;
  h->hp = *hp;
  h->audio_ctx = hp->n_audio_ctx;
  h->eot = hp->n_vocab >= 51865 ? 50257 : 50256;   // multilingual vocabularies shift the specials by one
  if (const char* e = dev_env("CRISPY_ASR_XCD")) h->xcd_swizzle = std::atoi(e) != 0;
  auto body = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    int r = crispy_mel_create(mel_filters, hp->n_mels, device, &h->mel);
    if (r != CRISPY_OK) return r;
    for (const auto& kv : expected_tensors(*hp)) {     // device memory is taken when a tensor is set: a resident
      h->tensors[kv.first].n = kv.second;               // quantised model never holds its matrices as f32
    }
    return CRISPY_OK;
  };
  rc = body();
  if (rc != CRISPY_OK) {
    const std::string keep = last_error_cstr();
    crispy_asr_free(h);
    return fail(rc, "%s", keep.c_str());
  }
  *out = h;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_create")

void crispy_asr_free(crispy_asr* h) try {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->drop_graphs();                        // the captured steps hold the workspaces' addresses: they go first
  crispy_mel* const mel = h->mel;
  const hipEvent_t ev_scratch = h->ev_scratch;
  const hipStream_t stream = h->stream;
  delete h;                                // every device buffer is a member: let go here, on the handle's device, after the sync
  if (mel) crispy_mel_destroy(mel);
  if (ev_scratch) (void)hipEventDestroy(ev_scratch);
  if (stream) (void)hipStreamDestroy(stream);
} CRISPY_CATCH_VOID("crispy_asr_free")

int crispy_asr_set_tensor(crispy_asr* h, const char* name, const float* data, size_t n_elems) try {
  if (!h || !name || !data) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_set_tensor: NULL argument");
  if (h->finalized) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_set_tensor: model already finalized");
  auto it = h->tensors.find(name);
  if (it == h->tensors.end()) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_set_tensor: unknown tensor '%s'", name);
  if (it->second.n != n_elems)
    return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_set_tensor: '%s' has %zu elements, expected %zu", name, n_elems,
                it->second.n);
  HIP_TRY(hipSetDevice(h->device));
  if (!it->second.d) HIP_TRY(it->second.d.alloc(n_elems * sizeof(float)));
  HIP_TRY(hipMemcpy(it->second.d, data, n_elems * sizeof(float), hipMemcpyHostToDevice));
  it->second.set = true;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_set_tensor")

}  // extern "C"

namespace crispy {
namespace asr {
namespace {

int finalize_tail(crispy_asr* h) {
  const std::vector<unsigned char> none(h->hp.n_vocab, 0);
  int rc = upload_mask(h->d_suppress, none);
  if (rc == CRISPY_OK) rc = upload_mask(h->d_suppress_first, none);
  if (rc == CRISPY_OK) rc = build_ts_masks(h);
  if (rc != CRISPY_OK) return rc;
  h->finalized = true;
  return CRISPY_OK;
}

// f16 copies of the two convolution kernels (precision mode 1; conv1's rows [3 n_mels] zero-padded to a multiple of 32
// columns, 3 * 80 = 240 -> 256: the padded operand columns of A read on into the next frames -- finite values -- and meet
// zeros here)
int make_conv_halves(crispy_asr* h) {
  const size_t d = h->hp.n_audio_state;
  int rc = half_copy(h, h->conv2_w, d * 3 * d, &h->conv2_wh);
  if (rc != CRISPY_OK) return rc;
  const int k1 = 3 * h->hp.n_mels, k1p = (k1 + 31) / 32 * 32;
  void* p = nullptr;
  if ((rc = derived_copy(h, d * k1p * 2, &p)) != CRISPY_OK) return rc;
  HIP_TRY(hipMemsetAsync(p, 0, d * k1p * 2, h->stream));
  HIP_TRY(convert_rows_f32_to_f16(h->conv1_w, k1, p, k1p, k1, (long)d, h->stream));
  h->conv1_wh = p;
  h->conv1_kp = k1p;
  return CRISPY_OK;
}

// What both finalize paths resolve alike: the reordered convolution kernels and every vector the kernels read as the model
// file holds it -- conv biases, positional embeddings, every LayerNorm, the biases that are not row-fused.  The dense path
// adds the matrices (fuse_rows / fold_ln), the resident path the block references (QRef) and fuse_bias.
int resolve_shared(crispy_asr* h) {
  const int d = h->hp.n_audio_state;
  int rc;
  if ((rc = reorder_conv(h, "encoder.conv1.weight", d, h->hp.n_mels, &h->conv1_w)) != CRISPY_OK) return rc;
  if ((rc = reorder_conv(h, "encoder.conv2.weight", d, d, &h->conv2_w)) != CRISPY_OK) return rc;
  Resolver T{h};
  h->conv1_b = T("encoder.conv1.bias");
  h->conv2_b = T("encoder.conv2.bias");
  h->enc_pos = T("encoder.positional_embedding");
  h->ln_post_w = T("encoder.ln_post.weight");
  h->ln_post_b = T("encoder.ln_post.bias");
  h->enc.resize(h->hp.n_audio_layer);
  for (int i = 0; i < h->hp.n_audio_layer; ++i) {
    const std::string p = "encoder.blocks." + std::to_string(i) + ".";
    EncLayer& L = h->enc[i];
    L.ln1_w = T(p + "attn_ln.weight"); L.ln1_b = T(p + "attn_ln.bias");
    L.ln2_w = T(p + "mlp_ln.weight"); L.ln2_b = T(p + "mlp_ln.bias");
    L.out_b = T(p + "attn.out.bias"); L.fc1_b = T(p + "mlp.0.bias"); L.fc2_b = T(p + "mlp.2.bias");
    L.qkv_w = L.out_w = L.fc1_w = L.fc2_w = nullptr;
  }
  h->dec.resize(h->hp.n_text_layer);
  for (int i = 0; i < h->hp.n_text_layer; ++i) {
    const std::string p = "decoder.blocks." + std::to_string(i) + ".";
    DecLayer& L = h->dec[i];
    L.ln1_w = T(p + "attn_ln.weight"); L.ln1_b = T(p + "attn_ln.bias");
    L.lnx_w = T(p + "cross_attn_ln.weight"); L.lnx_b = T(p + "cross_attn_ln.bias");
    L.ln2_w = T(p + "mlp_ln.weight"); L.ln2_b = T(p + "mlp_ln.bias");
    L.out_b = T(p + "attn.out.bias"); L.xq_b = T(p + "cross_attn.query.bias");
    L.xout_b = T(p + "cross_attn.out.bias"); L.fc1_b = T(p + "mlp.0.bias"); L.fc2_b = T(p + "mlp.2.bias");
    L.qkv_w = L.out_w = L.xq_w = L.xkv_w = L.xout_w = L.fc1_w = L.fc2_w = nullptr;
    L.qkv_lw = L.xq_lw = L.fc1_lw = nullptr;
  }
  h->tok_emb = nullptr;
  h->dec_pos = T("decoder.positional_embedding");
  h->dec_ln_w = T("decoder.ln.weight");
  h->dec_ln_b = T("decoder.ln.bias");
  return T.rc;
}

// crispy_asr_finalize of a dense model: every matrix is an f32 tensor; q | k | v and the cross k | v are fused by rows, the
// LayerNorm in front of q | k | v, cross-q and fc1 is folded into the decode projections
int finalize_dense(crispy_asr* h) {
  const int d = h->hp.n_audio_state, dt = h->hp.n_text_state;
  int rc = resolve_shared(h);
  if (rc != CRISPY_OK) return rc;
  Resolver T{h};
  for (int i = 0; i < h->hp.n_audio_layer; ++i) {
    const std::string p = "encoder.blocks." + std::to_string(i) + ".";
    EncLayer& L = h->enc[i];
    rc = fuse_rows(h, {p + "attn.query.weight", p + "attn.key.weight", p + "attn.value.weight"},
                   {p + "attn.query.bias", "", p + "attn.value.bias"}, d, &L.qkv_w, &L.qkv_b);
    if (rc != CRISPY_OK) return rc;
    L.out_w = T(p + "attn.out.weight"); L.fc1_w = T(p + "mlp.0.weight"); L.fc2_w = T(p + "mlp.2.weight");
  }
  h->tok_emb = T("decoder.token_embedding.weight");
  for (int i = 0; i < h->hp.n_text_layer; ++i) {
    const std::string p = "decoder.blocks." + std::to_string(i) + ".";
    DecLayer& L = h->dec[i];
    rc = fuse_rows(h, {p + "attn.query.weight", p + "attn.key.weight", p + "attn.value.weight"},
                   {p + "attn.query.bias", "", p + "attn.value.bias"}, dt, &L.qkv_w, &L.qkv_b);
    if (rc != CRISPY_OK) return rc;
    L.out_w = T(p + "attn.out.weight"); L.xq_w = T(p + "cross_attn.query.weight");
    rc = fuse_rows(h, {p + "cross_attn.key.weight", p + "cross_attn.value.weight"}, {"", p + "cross_attn.value.bias"},
                   dt, &L.xkv_w, &L.xkv_b);
    if (rc != CRISPY_OK) return rc;
    L.xout_w = T(p + "cross_attn.out.weight"); L.fc1_w = T(p + "mlp.0.weight"); L.fc2_w = T(p + "mlp.2.weight");
    if (T.rc != CRISPY_OK) return T.rc;
    rc = fold_ln(h, L.qkv_w, L.qkv_b, L.ln1_w, L.ln1_b, 3 * (size_t)dt, dt, &L.qkv_lw, &L.qkv_ls, &L.qkv_lc);
    if (rc == CRISPY_OK) rc = fold_ln(h, L.xq_w, L.xq_b, L.lnx_w, L.lnx_b, dt, dt, &L.xq_lw, &L.xq_ls, &L.xq_lc);
    if (rc == CRISPY_OK) rc = fold_ln(h, L.fc1_w, L.fc1_b, L.ln2_w, L.ln2_b, 4 * (size_t)dt, dt, &L.fc1_lw, &L.fc1_ls, &L.fc1_lc);
    if (rc != CRISPY_OK) return rc;
  }
  if (T.rc != CRISPY_OK) return T.rc;
  return finalize_tail(h);
}

// The resident token embedding for the logits: f16, packed in MFMA operand order, from a dense copy that lives for this
// function only (pack, stream sync, then release)
int pack_resident_tok_emb(crispy_asr* h) {
  const int dt = h->hp.n_text_state, V = h->hp.n_vocab;
  DevBuf<float> tmp;
  HIP_TRY(tmp.alloc((size_t)V * dt * sizeof(float)));
  HIP_TRY(dequant_blocks(h->q_tok_emb->d, h->q_tok_emb->ttype, (long)((size_t)V * dt / 32), dt, tmp, 0, nullptr, h->stream));
  void* packed = nullptr;
  const int rc = derived_copy(h, vocab_f16_packed_bytes(V, dt), &packed);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(pack_vocab_f16(tmp, packed, V, dt, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->tok_emb_hp = packed;
  return CRISPY_OK;
}

// crispy_asr_load_resident: the 2-D tensors stay as the file's ggml blocks (h->qtensors); what is made here is small --
// fused biases, the LayerNorm-fold vectors of the decode projections, the two convolution kernels (f16 / f32 in every
// ggml file) -- plus the token embedding packed in MFMA operand order for the logits (f16: the one matrix kept dense;
// its quantised form stays resident too and serves the embedding look-ups).  Precision mode 1 only: the operands of
// every matrix product are de-quantised to f16 (f32 x gamma for the folded projections) right in front of the product.
int finalize_resident(crispy_asr* h) {
  const int d = h->hp.n_audio_state, dt = h->hp.n_text_state;
  if (!whisper_width_ok(dt))
    return fail(CRISPY_ERR_UNSUPPORTED, "crispy_asr_load_resident: width %d has no f16 logits kernel", dt);
  int rc = resolve_shared(h);
  if (rc != CRISPY_OK) return rc;
  // a matrix the file holds dense (f32 / f16: mixed files) takes part as a QT_F32 "block" tensor aliasing its dense copy
  auto matrix = [&](const std::string& name, int cols) -> int {
    if (h->qtensors.count(name)) return CRISPY_OK;
    const Tensor* t = find_tensor(h, name);
    if (!t) return CRISPY_ERR_BAD_MODEL;
    if (!t->d) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_load_resident: tensor '%s' missing", name.c_str());
    QTensor& q = h->qtensors[name];
    q.d = reinterpret_cast<const unsigned char*>(t->d.p); q.ttype = QT_F32; q.n = t->n; q.cols = cols; q.nbytes = t->n * 4;
    return CRISPY_OK;
  };
  size_t max_elems = 0;
  auto ref = [&](std::initializer_list<std::string> names, int cols, QRef* out) -> int {
    for (const std::string& n : names) { const int r = matrix(n, cols); if (r != CRISPY_OK) return r; }
    *out = qref(h, names);
    if (out->elems() > max_elems) max_elems = out->elems();
    return CRISPY_OK;
  };
  for (int i = 0; i < h->hp.n_audio_layer; ++i) {
    const std::string p = "encoder.blocks." + std::to_string(i) + ".";
    EncLayer& L = h->enc[i];
    if ((rc = ref({p + "attn.query.weight", p + "attn.key.weight", p + "attn.value.weight"}, d, &L.r_qkv)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "attn.out.weight"}, d, &L.r_out)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "mlp.0.weight"}, d, &L.r_fc1)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "mlp.2.weight"}, 4 * d, &L.r_fc2)) != CRISPY_OK) return rc;
    if ((rc = fuse_bias(h, {p + "attn.query.bias", "", p + "attn.value.bias"}, d, &L.qkv_b)) != CRISPY_OK) return rc;
  }
  for (int i = 0; i < h->hp.n_text_layer; ++i) {
    const std::string p = "decoder.blocks." + std::to_string(i) + ".";
    DecLayer& L = h->dec[i];
    if ((rc = ref({p + "attn.query.weight", p + "attn.key.weight", p + "attn.value.weight"}, dt, &L.r_qkv)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "attn.out.weight"}, dt, &L.r_out)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "cross_attn.query.weight"}, dt, &L.r_xq)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "cross_attn.key.weight", p + "cross_attn.value.weight"}, dt, &L.r_xkv)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "cross_attn.out.weight"}, dt, &L.r_xout)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "mlp.0.weight"}, dt, &L.r_fc1)) != CRISPY_OK) return rc;
    if ((rc = ref({p + "mlp.2.weight"}, 4 * dt, &L.r_fc2)) != CRISPY_OK) return rc;
    if ((rc = fuse_bias(h, {p + "attn.query.bias", "", p + "attn.value.bias"}, dt, &L.qkv_b)) != CRISPY_OK) return rc;
    if ((rc = fuse_bias(h, {"", p + "cross_attn.value.bias"}, dt, &L.xkv_b)) != CRISPY_OK) return rc;
  }
  if ((rc = matrix("decoder.token_embedding.weight", dt)) != CRISPY_OK) return rc;
  h->q_tok_emb = &h->qtensors["decoder.token_embedding.weight"];
  // the one scratch slot: the largest (fused) matrix as f32
  HIP_TRY(h->q_scratch.alloc(max_elems * sizeof(float)));
  if ((rc = pack_resident_tok_emb(h)) != CRISPY_OK) return rc;
  if ((rc = make_conv_halves(h)) != CRISPY_OK) return rc;
  // One matrix per decoder layer is kept de-quantised as well: the cross-q projection, as f16 (the values the blocks
  // de-quantise to at the point of use: same bits).  The matrix-vector decode step computes a head's query in every one of the
  // workgroups that share the head's keys (whisper_dec_gemv.hip: gv_xattn_kernel), and de-quantising it four times over cost
  // large-v3-q5_0 more than the launch the fusion saves (1.78 -> 1.92 ms per token); 1 / 14 of the decoder's weights, + 7 % memory.
  if (gemv_dec_supported(dt, 1)) {
    for (DecLayer& L : h->dec) {
      if (!gemv_ref_ok(L.r_xq)) continue;
      void* p = nullptr;
      if ((rc = derived_copy(h, (size_t)dt * dt * 2, &p)) != CRISPY_OK) return rc;
      HIP_TRY(dequant_blocks(L.r_xq.t[0]->d, L.r_xq.t[0]->ttype, (long)((size_t)dt * dt / 32), dt, p, 1, nullptr, h->stream));
      L.xq_wh = p;
    }
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->half_ready = true;
  h->enc_precision = 1;
  h->dec_ln16 = true;                        // mode 1: f16 LayerNorm outputs against the blocks de-quantised to f16 (gemm_skinny_q, WH forms)
  return finalize_tail(h);
}

// Precision mode 1: f16 copies of the encoder GEMM weights and of the decoder's plain projections, made on the device once
int make_mode1_halves(crispy_asr* h) {
  const size_t d = h->hp.n_audio_state, dtt = h->hp.n_text_state;
  int rc = make_conv_halves(h);
  for (EncLayer& L : h->enc) {
    if (rc == CRISPY_OK) rc = half_copy(h, L.qkv_w, 3 * d * d, &L.qkv_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.out_w, d * d, &L.out_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.fc1_w, 4 * d * d, &L.fc1_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.fc2_w, 4 * d * d, &L.fc2_wh);
  }
  for (DecLayer& L : h->dec) {
    if (rc == CRISPY_OK) rc = half_copy(h, L.xkv_w, 2 * dtt * dtt, &L.xkv_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.out_w, dtt * dtt, &L.out_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.xout_w, dtt * dtt, &L.xout_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.fc2_w, 4 * dtt * dtt, &L.fc2_wh);
  }
  if (rc != CRISPY_OK) return rc;
  const int dt = h->hp.n_text_state;
  if (whisper_width_ok(dt)) {    // the widths the f16 logits kernel is built for
    // token embedding for the logits: f16 (as the model file holds it), packed in MFMA operand order
    void* p = nullptr;
    if ((rc = derived_copy(h, vocab_f16_packed_bytes(h->hp.n_vocab, dt), &p)) != CRISPY_OK) return rc;
    HIP_TRY(pack_vocab_f16(h->tok_emb, p, h->hp.n_vocab, dt, h->stream));
    h->tok_emb_hp = p;
  }
  return CRISPY_OK;
}

// Precision modes 1 and 2: f16 copies of the decoder's q | k | v, cross-q and fc1 weights (un-folded: the LayerNorm runs as
// a launch of its own), and the fused step kernels' operand order (same bytes once more)
int make_ln16_halves(crispy_asr* h) {
  const size_t dtt = h->hp.n_text_state;
  const bool fused = fused_decode_supported((int)dtt, 1, h->hp.n_audio_ctx);
  int rc = CRISPY_OK;
  for (DecLayer& L : h->dec) {
    if (rc == CRISPY_OK) rc = half_copy(h, L.qkv_w, 3 * dtt * dtt, &L.qkv_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.xq_w, dtt * dtt, &L.xq_wh);
    if (rc == CRISPY_OK) rc = half_copy(h, L.fc1_w, 4 * dtt * dtt, &L.fc1_wh);
    if (!fused) continue;
    if (rc == CRISPY_OK) rc = packed_copy(h, L.qkv_wh, 3 * dtt * dtt, 0, &L.qkv_p);
    if (rc == CRISPY_OK) rc = packed_copy(h, L.out_wh, dtt * dtt, 1, &L.out_p);
    if (rc == CRISPY_OK) rc = packed_copy(h, L.fc1_wh, 4 * dtt * dtt, 2, &L.fc1_p);
    if (rc == CRISPY_OK) rc = packed_copy(h, L.fc2_wh, 4 * dtt * dtt, 3, &L.fc2_p);
  }
  return rc;
}

}  // namespace
}  // namespace asr
}  // namespace crispy

extern "C" {

int crispy_asr_finalize(crispy_asr* h) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_finalize: NULL handle");
  if (h->finalized) return CRISPY_OK;
  for (const auto& kv : h->tensors)
    if (!kv.second.set) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_finalize: tensor '%s' was never set", kv.first.c_str());
  HIP_TRY(hipSetDevice(h->device));
  return h->resident ? finalize_resident(h) : finalize_dense(h);
} CRISPY_CATCH_RET("crispy_asr_finalize")

int crispy_asr_hparams_get(const crispy_asr* h, crispy_asr_hparams* out) try {
  if (!h || !out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_hparams_get: NULL argument");
  *out = h->hp;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_hparams_get")

int crispy_asr_set_precision(crispy_asr* h, int mode) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_set_precision: NULL handle");
  if (!h->finalized) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_set_precision: model not finalized");
  if (mode < 0 || mode > 2)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_set_precision: mode must be 0 (f32 operands), 1 (whisper.cpp's arithmetic: f16 operands of every product, f16 LayerNorm outputs and caches) "
                "or 2 (1 + the query and the normalised probabilities rounded to f16 inside the attentions)");
  HIP_TRY(hipSetDevice(h->device));
  const bool want_attn16 = mode == 2;
  if (mode == 2) mode = 1;
  const bool want_ln16 = mode == 1;
  if (h->resident && (mode != 1 || want_attn16))
    return fail(CRISPY_ERR_UNSUPPORTED, "crispy_asr_set_precision: a resident quantised model runs in precision mode 1 only "
                "(its matrices exist as f16 operands at the point of use, never as f32 tensors)");
  // `half_ready` / `ln16_ready` are only set after the last copy and a stream sync: an allocation failing part-way (OOM on
  // a large model) leaves the mode unchanged and a retry starts over (the partial copies stay owned by `derived` until the
  // handle is freed) -- ADVICE r2.
  if (mode == 1 && !h->half_ready) {
    const int rc = make_mode1_halves(h);
    if (rc != CRISPY_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->half_ready = true;
  }
  if (want_ln16 && !h->resident && !h->ln16_ready) {
    const int rc = make_ln16_halves(h);
    if (rc != CRISPY_OK) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->ln16_ready = true;
  }
  if (h->enc_precision != mode || h->dec_ln16 != want_ln16 || h->dec_attn16 != want_attn16) {   // the captured decode steps bake the kernels in
    h->drop_graphs();
  }
  h->enc_precision = mode;
  h->dec_ln16 = want_ln16;
  h->dec_attn16 = want_attn16;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_set_precision")

// whisper.cpp's whisper_full_params.audio_ctx [UPSTREAM-RECALL].  Every call builds its encoder output and cross K | V from
// h->audio_ctx, so nothing of an earlier layout is read after a switch; what bakes the value in are the captured decode
// steps (key count, strides, stream_kv of their launches): they go, after everything in flight on the handle has finished.
int crispy_asr_set_audio_ctx(crispy_asr* h, int n) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_set_audio_ctx: NULL handle");
  if (!h->finalized) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_set_audio_ctx: model not finalized");
  if (n < 0 || n > h->hp.n_audio_ctx)
    return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_set_audio_ctx: n = %d (0 = the model's own, or 1 ... %d)", n, h->hp.n_audio_ctx);
  const int want = n == 0 ? h->hp.n_audio_ctx : n;
  if (want == h->audio_ctx) return CRISPY_OK;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->drop_graphs();
  h->audio_ctx = want;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_set_audio_ctx")

int crispy_asr_audio_ctx(const crispy_asr* h, int* n) try {
  if (!h || !n) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_audio_ctx: NULL argument");
  if (!h->finalized) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_audio_ctx: model not finalized");
  *n = h->audio_ctx;
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_audio_ctx")

}  // extern "C"

namespace crispy {
namespace asr {
namespace {

// the convolution stem: padded frame-major mel -> residual stream h->ew.x [batch * Tn][d] (GELU, positional embedding added).
// Tn = the handle's audio context.  Below the model's own, conv1 runs over the first 2 Tn frames and must see its own zero
// padding at frame 2 Tn [UPSTREAM-RECALL: whisper.cpp builds the graph over a 2 * audio_ctx view of the mel], where the
// caller's buffer holds the real frame: `cut` clears padded row 2 Tn + 1 in a copy (mode 1 has one anyway: the f16 mel).
int encode_stem(crispy_asr* h, const float* d_mel_t, int batch, hipStream_t s) {
  const int d = h->hp.n_audio_state, Tn = h->audio_ctx, nm = h->hp.n_mels;
  const bool cut = Tn < h->hp.n_audio_ctx;
  const int M1 = 2 * Tn;                                      // conv1's frames
  if (h->enc_precision == 1) {
    // The convolution stem on the f16 matrix cores too (ggml runs a convolution as im2col in f16 x f16 kernel): the
    // frame-major mel is rounded to f16 once, conv1 writes GELU(h1) as f16 (it only feeds conv2), conv2 reads it as
    // a strided view and writes the f32 residual stream.  The f16 buffers alias the hidden-layer / h1 workspace.
    _Float16* mel_h = h->ew.h.as<_Float16>();                 // [batch][3002][n_mels] (+ padding)
    _Float16* h1_h = h->ew.h1.as<_Float16>();                 // [batch][3001][d], row 0 of a clip = zeros
    const long mel_n = (long)batch * (MEL_FRAMES + 2) * nm;
    HIP_TRY(convert_f32_to_f16(d_mel_t, mel_h, mel_n, s));
    HIP_TRY(hipMemsetAsync(mel_h + mel_n, 0, 64 * sizeof(_Float16), s));  // what the last row's padded columns read
    if (cut) HIP_TRY(hipMemset2DAsync(mel_h + (size_t)(M1 + 1) * nm, (size_t)(MEL_FRAMES + 2) * nm * 2, 0, (size_t)nm * 2, batch, s));
    HIP_TRY(hipMemset2DAsync(h1_h, (size_t)(MEL_FRAMES + 1) * d * 2, 0, (size_t)d * 2, batch, s));
    {
      HGemmArgs g{};
      g.A = mel_h; g.lda = nm; g.strideA = (long)(MEL_FRAMES + 2) * nm;
      g.W = reinterpret_cast<const _Float16*>(h->conv1_wh); g.ldw = h->conv1_kp;
      g.C = h1_h + d; g.ldc = d; g.strideC = (long)(MEL_FRAMES + 1) * d;
      g.bias = h->conv1_b; g.M = M1; g.N = d; g.K = h->conv1_kp; g.gelu = 1;
      HIP_TRY(gemm_hh(g, HGEMM_F16, batch, s));
    }
    {
      HGemmArgs g{};
      g.A = h1_h; g.lda = 2L * d; g.strideA = (long)(MEL_FRAMES + 1) * d;
      g.W = reinterpret_cast<const _Float16*>(h->conv2_wh); g.ldw = 3L * d;
      g.C = h->ew.x; g.ldc = d; g.strideC = (long)Tn * d;
      g.bias = h->conv2_b; g.M = Tn; g.N = d; g.K = 3 * d;
      g.rowtab = h->enc_pos; g.rowtab_period = Tn;
      HIP_TRY(gemm_hh(g, HGEMM_TAB, batch, s));
    }
  } else {
    // conv1 (k3, p1) + GELU: rows t of the padded frame-major mel are 3*n_mels contiguous floats
    // (the zero row in front of every clip's h1 is rewritten each call: precision mode 1 uses the same workspace as f16)
    HIP_TRY(hipMemset2DAsync(h->ew.h1, (size_t)(MEL_FRAMES + 1) * d * sizeof(float), 0, (size_t)d * sizeof(float), batch, s));
    if (cut) {      // rows 0 .. 2 Tn of every clip into the hidden-layer workspace (free until fc1), row 2 Tn + 1 cleared
      const size_t pitch = (size_t)(MEL_FRAMES + 2) * nm * sizeof(float);
      HIP_TRY(hipMemcpy2DAsync(h->ew.h, pitch, d_mel_t, pitch, (size_t)(M1 + 1) * nm * sizeof(float), batch, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemset2DAsync(h->ew.h + (size_t)(M1 + 1) * nm, pitch, 0, (size_t)nm * sizeof(float), batch, s));
      d_mel_t = h->ew.h;
    }
    {
      GemmArgs g = gemm(d_mel_t, nm, h->conv1_w, 3L * nm, h->ew.h1 + d, d, h->conv1_b, M1, d, 3 * nm);
      g.strideA = (long)(MEL_FRAMES + 2) * nm;
      g.strideC = (long)(MEL_FRAMES + 1) * d;
      g.gelu = 1;
      HIP_TRY(gemm_f32_nt(g, batch, s));
    }
    // conv2 (k3, s2, p1) + GELU + positional embedding: row t' = frames 2t'-1 .. 2t'+1 of h1 (one zero row in front)
    {
      GemmArgs g = gemm(h->ew.h1, 2L * d, h->conv2_w, 3L * d, h->ew.x, d, h->conv2_b, Tn, d, 3 * d);
      g.strideA = (long)(MEL_FRAMES + 1) * d;
      g.strideC = (long)Tn * d;
      g.gelu = 1;
      g.rowtab = h->enc_pos;
      g.rowtab_period = Tn;
      HIP_TRY(gemm_f32_nt(g, batch, s));
    }
  }
  return CRISPY_OK;
}

// the encoder layers over h->ew.x in precision mode 1
int encode_layers_f16(crispy_asr* h, int batch, hipStream_t s) {
  const int d = h->hp.n_audio_state, Tn = h->audio_ctx, H = h->hp.n_audio_head;
  const long rows = (long)batch * Tn;
  int rc = CRISPY_OK;
  // whisper.cpp's numerics with the bytes halved: every activation that only feeds a matrix product is stored as the
  // f16 value the product would round it to anyway (LayerNorm output, q | k, V^T, attention output, MLP hidden
  // layer); the residual stream stays f32.  The f16 buffers alias the f32 workspace of the default mode.
  void* xn_h = h->ew.xn;                                                   // [rows][d] f16
  void* qk_h = h->ew.qkv;                                                  // [rows][2 d] f16
  void* vt_h = h->ew.qkv.as<_Float16>() + rows * 2L * d;     // [batch][d][ENC_TP] f16
  void* att_h = h->ew.att;                                                 // [rows][d] f16
  void* hid_h = h->ew.h;                                                   // [rows][4 d] f16
  const int swz = h->xcd_swizzle;
  auto hg = [&](const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias, int N, int K) {
    HGemmArgs g{};
    g.A = reinterpret_cast<const _Float16*>(A); g.lda = lda; g.W = reinterpret_cast<const _Float16*>(W); g.ldw = ldw;
    g.C = C; g.ldc = ldc; g.bias = bias; g.M = (int)rows; g.N = N; g.K = K; g.vt_T = Tn; g.xcd_swizzle = swz;
    return g;
  };
  // f16 weights of a product: the resident copy, or -- resident quantised model -- the blocks de-quantised into the
  // scratch slot right here (the previous product has finished with the slot: same stream)
  auto w16 = [&](const void* dense, const QRef& r, const void** out) -> int {
    if (!h->resident) { *out = dense; return CRISPY_OK; }
    return dq(h, r, true, nullptr, s, out);
  };
  for (const EncLayer& L : h->enc) {
    const void* w = nullptr;
    HIP_TRY(layernorm_f16out(h->ew.x, L.ln1_w, L.ln1_b, xn_h, rows, d, s));
    if ((rc = w16(L.qkv_wh, L.r_qkv, &w)) != CRISPY_OK) return rc;
    HIP_TRY(gemm_hh(hg(xn_h, d, w, d, qk_h, 2L * d, L.qkv_b, 2 * d, d), HGEMM_F16, 1, s));
    HIP_TRY(gemm_hh(hg(xn_h, d, reinterpret_cast<const _Float16*>(w) + 2L * d * d, d, vt_h, 0, L.qkv_b + 2 * d, d, d),
                    HGEMM_VT, 1, s));
    HIP_TRY(attn_encoder_h(qk_h, vt_h, att_h, batch, Tn, d, H, s, h->dec_attn16 ? 1 : 0));     // mode 2: ggml's rounding points inside the attention
    {
      if ((rc = w16(L.out_wh, L.r_out, &w)) != CRISPY_OK) return rc;
      HGemmArgs g = hg(att_h, d, w, d, h->ew.x, d, L.out_b, d, d);
      g.residual = h->ew.x; g.ldr = d;
      HIP_TRY(gemm_hh(g, HGEMM_RES, 1, s));
    }
    HIP_TRY(layernorm_f16out(h->ew.x, L.ln2_w, L.ln2_b, xn_h, rows, d, s));
    {
      if ((rc = w16(L.fc1_wh, L.r_fc1, &w)) != CRISPY_OK) return rc;
      HGemmArgs g = hg(xn_h, d, w, d, hid_h, 4L * d, L.fc1_b, 4 * d, d);
      g.gelu = 1;
      HIP_TRY(gemm_hh(g, HGEMM_F16, 1, s));
    }
    {
      if ((rc = w16(L.fc2_wh, L.r_fc2, &w)) != CRISPY_OK) return rc;
      HGemmArgs g = hg(hid_h, 4L * d, w, 4L * d, h->ew.x, d, L.fc2_b, d, 4 * d);
      g.residual = h->ew.x; g.ldr = d;
      HIP_TRY(gemm_hh(g, HGEMM_RES, 1, s));
    }
  }
  return CRISPY_OK;
}

// ... and in precision mode 0 (f32 operands)
int encode_layers_f32(crispy_asr* h, int batch, hipStream_t s) {
  const int d = h->hp.n_audio_state, Tn = h->audio_ctx, H = h->hp.n_audio_head;
  const long rows = (long)batch * Tn;
  // g.tiled: the 128 x 128 kernel at every row count.  At a small audio context batch x Tn falls into the skinny kernel's
  // range (a decode step's shape), whose sums run in another order: a clip's bits would depend on the batch it is encoded in.
  for (const EncLayer& L : h->enc) {
    HIP_TRY(layernorm_f32(h->ew.x, L.ln1_w, L.ln1_b, h->ew.xn, rows, d, s));
    {
      GemmArgs g = gemm(h->ew.xn, d, L.qkv_w, d, h->ew.qkv, 3L * d, L.qkv_b, (int)rows, 3 * d, d);
      g.tiled = 1;
      HIP_TRY(gemm_f32_nt(g, 1, s));
    }
    HIP_TRY(attn_encoder_f32(h->ew.qkv, h->ew.att, batch, Tn, d, H, s));
    {
      GemmArgs g = gemm(h->ew.att, d, L.out_w, d, h->ew.x, d, L.out_b, (int)rows, d, d);
      g.tiled = 1;
      g.residual = h->ew.x; g.ldr = d;
      HIP_TRY(gemm_f32_nt(g, 1, s));
    }
    HIP_TRY(layernorm_f32(h->ew.x, L.ln2_w, L.ln2_b, h->ew.xn, rows, d, s));
    {
      GemmArgs g = gemm(h->ew.xn, d, L.fc1_w, d, h->ew.h, 4L * d, L.fc1_b, (int)rows, 4 * d, d);
      g.tiled = 1;
      g.gelu = 1;
      HIP_TRY(gemm_f32_nt(g, 1, s));
    }
    {
      GemmArgs g = gemm(h->ew.h, 4L * d, L.fc2_w, 4L * d, h->ew.x, d, L.fc2_b, (int)rows, d, 4 * d);
      g.tiled = 1;
      g.residual = h->ew.x; g.ldr = d;
      HIP_TRY(gemm_f32_nt(g, 1, s));
    }
  }
  return CRISPY_OK;
}

}  // namespace
}  // namespace asr
}  // namespace crispy

extern "C" {

int crispy_asr_encode_device(crispy_asr* h, const float* d_mel_t, int batch, float* d_out, void* hip_stream) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_encode_device: NULL handle");
  if (!h->finalized) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_encode_device: model not finalized");
  if (batch < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_encode_device: batch < 0");
  if (batch == 0) return CRISPY_OK;
  if (!d_mel_t || !d_out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_encode_device: NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  int rc = reserve_enc(h, batch);
  if (rc != CRISPY_OK) return rc;
  // A resident quantised model de-quantises every weight into ONE scratch slot in front of its product; decode, cross K|V
  // and the LayerNorm folding fill it on the handle's own stream.  A caller's stream is not ordered against that one, so
  // an encode enqueued here while a decode of the same handle is still in flight would overwrite weights in use
  // (ADVICE r3): order the two explicitly -- this encode starts after everything enqueued on the handle's stream so far,
  // and the handle's stream continues after it.
  struct ScratchOrder {
    crispy_asr* h; hipStream_t s; bool on;
    ~ScratchOrder() {
      if (on && hipEventRecord(h->ev_scratch, s) == hipSuccess) (void)hipStreamWaitEvent(h->stream, h->ev_scratch, 0);
    }
  } scratch_order{h, s, false};
  if (h->resident && s != h->stream) {
    if (!h->ev_scratch) HIP_TRY(hipEventCreateWithFlags(&h->ev_scratch, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(h->ev_scratch, h->stream));
    HIP_TRY(hipStreamWaitEvent(s, h->ev_scratch, 0));
    scratch_order.on = true;
  }
  rc = encode_stem(h, d_mel_t, batch, s);
  if (rc == CRISPY_OK) rc = h->enc_precision == 1 ? encode_layers_f16(h, batch, s) : encode_layers_f32(h, batch, s);
  if (rc != CRISPY_OK) return rc;
  const long rows = (long)batch * h->audio_ctx;
  const int d = h->hp.n_audio_state;
  HIP_TRY(layernorm_f32(h->ew.x, h->ln_post_w, h->ln_post_b, d_out, rows, d, s));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_encode_device")

// PCM (host) -> log-mel -> encoder output (host); one call per batch of <= 30 s clips
int crispy_asr_encode(crispy_asr* h, const float* pcm, long pcm_stride, const int* n_samples, int batch, float* out) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_encode: NULL handle");
  if (!h->finalized) return fail(CRISPY_ERR_BAD_MODEL, "crispy_asr_encode: model not finalized");
  if (batch < 0) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_encode: batch < 0");
  if (batch == 0) return CRISPY_OK;
  if (!pcm || !n_samples || !out) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_encode: NULL argument");
  HIP_TRY(hipSetDevice(h->device));
  int rc = reserve_enc(h, batch);
  if (rc != CRISPY_OK) return rc;
  rc = reserve_pcm(h, pcm_stride);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(h->ew.pcm, pcm, (size_t)batch * pcm_stride * sizeof(float), hipMemcpyHostToDevice, h->stream));
  rc = crispy_mel_compute_device(h->mel, h->ew.pcm, pcm_stride, n_samples, batch, nullptr, h->ew.melt, h->stream);
  if (rc != CRISPY_OK) return rc;
  rc = crispy_asr_encode_device(h, h->ew.melt, batch, h->ew.enc, h->stream);
  if (rc != CRISPY_OK) return rc;
  HIP_TRY(hipMemcpyAsync(out, h->ew.enc, (size_t)batch * h->audio_ctx * h->hp.n_audio_state * sizeof(float),
                         hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_encode")

int crispy_asr_synchronize(crispy_asr* h) try {
  if (!h) return fail(CRISPY_ERR_INVALID_ARG, "crispy_asr_synchronize: NULL handle");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return CRISPY_OK;
} CRISPY_CATCH_RET("crispy_asr_synchronize")

}  // extern "C"

// diar_fbank.hip -- the features the embedding network of the diarization path reads, for MI355X (gfx950): an 80-bin
// Kaldi fbank with per-chunk mean subtraction, what EmbeddingExtractor::compute gets from knf_rs::compute_fbank
// (src-tauri/src/managers/diarization.rs:53-75), for all chunks of a recording in one launch pair.
//
//   fbank_frames_kernel  grid (tiles of all chunks): a workgroup of 4 waves takes kFbankTileFrames consecutive frames of
//                        one chunk, a wave kFbankWaveFrames of them, FB_NF at a time.  Per frame: 400 samples at hop 160,
//                        i16 (or f32 through f32_to_i16) / 32768 * scale, frame mean removed, pre-emphasis 0.97,
//                        Povey window, zero padding to 512, the real FFT as a 256-point complex Stockham transform in
//                        LDS (radices 4.4.4.4) plus the real-input pass, power spectrum in place, 501 sparse filter
//                        taps summed in f32 in tap order, log(max(e, FLT_EPSILON)).  Tables (8 KB) sit in LDS once per
//                        workgroup; 42 KB of LDS per workgroup.
//   fbank_means_kernel   one thread per (chunk, bin): the f32 sum of the column in frame order / the frame count,
//                        subtracted from every row.  A chunk's bytes depend on its own samples alone.
#include <cmath>

#include "diar_internal.h"
#include "fft_lds.h"

namespace crispy {
namespace diar {
namespace {

using namespace fftx;

constexpr int FB_NF = 4;         // frames a wave transforms at once
constexpr int FB_BS = 264;       // complex numbers between two frames' buffers (257 used: bin 256 keeps its power there)
constexpr size_t FB_LDS_BUF = 4 * FB_NF * FB_BS * sizeof(float2);
constexpr size_t FB_LDS = FB_LDS_BUF + sizeof(FbankTables);
static_assert(kFbankWaveFrames % FB_NF == 0 && kFbankTileFrames == 4 * kFbankWaveFrames, "a tile is 4 waves of whole batches");
static_assert(sizeof(FbankTables) % 4 == 0, "copied into LDS as 32-bit words");

// One sample as the reference hands it to the fbank: the i16 (f32: through f32_to_i16, (s.clamp(-1, 1) * 32767.0) as i16,
// truncating, NaN -> 0) as f32 / 32768, times scale.
template <bool F32>
__device__ __forceinline__ float sample(const void* __restrict__ pcm, long s, float scale) {
  int q;
  if (F32) {
    const float x = static_cast<const float*>(pcm)[s];
    const float c = fminf(fmaxf(x, -1.0f), 1.0f);
    q = x != x ? 0 : (int)(c * 32767.0f);
  } else {
    q = static_cast<const short*>(pcm)[s];
  }
  return ((float)q / 32768.0f) * scale;
}

template <bool F32>
__global__ __launch_bounds__(256) void fbank_frames_kernel(const FbankTables* __restrict__ tab, const void* __restrict__ pcm, float scale,
                                                           const FbankChunk* __restrict__ chunks, const FbankTile* __restrict__ tiles,
                                                           float* __restrict__ raw) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // per wave: FB_NF transform buffers (the power of bin k replaces the real part of element k); per workgroup: the tables
  float2* buf = reinterpret_cast<float2*>(smem) + wave * (FB_NF * FB_BS);
  float* fl = reinterpret_cast<float*>(buf);
  const FbankTables* lt = reinterpret_cast<const FbankTables*>(smem + FB_LDS_BUF);
  {
    const int* __restrict__ src = reinterpret_cast<const int*>(tab);
    int* dst = reinterpret_cast<int*>(smem + FB_LDS_BUF);
    for (int i = threadIdx.x; i < (int)(sizeof(FbankTables) / 4); i += 256) dst[i] = src[i];
    __syncthreads();
  }
  const FbankTile tile = tiles[blockIdx.x];
  const FbankChunk ch = chunks[tile.chunk];

  for (int fb = 0; fb < kFbankWaveFrames; fb += FB_NF) {
    const int f0 = tile.frame0 + wave * kFbankWaveFrames + fb;
    if (f0 >= ch.n_frames) break;      // the same for the whole wave; only wave-level synchronisation below
    // samples, frame mean, pre-emphasis from the back, window; frames past the chunk's last redo it (their rows are not stored)
    {
      float v[FB_NF][7];
#pragma unroll
      for (int f = 0; f < FB_NF; ++f) {
        const long s0 = ch.first + (long)min(f0 + f, ch.n_frames - 1) * kFbankHop;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int i = lane + 64 * j;
          v[f][j] = i < kFbankLen ? sample<F32>(pcm, s0 + i, scale) : 0.0f;
        }
      }
#pragma unroll
      for (int f = 0; f < FB_NF; ++f) {
        float p = v[f][0];
#pragma unroll
        for (int j = 1; j < 7; ++j) p += v[f][j];
        const float mean = shfl_sum(p) / (float)kFbankLen;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int i = lane + 64 * j;
          v[f][j] = i < kFbankLen ? v[f][j] - mean : 0.0f;
          fl[f * 2 * FB_BS + i] = v[f][j];
        }
        fl[f * 2 * FB_BS + 448 + lane] = 0.0f;
      }
      wave_lds_sync();
      float y[FB_NF][7];
#pragma unroll
      for (int f = 0; f < FB_NF; ++f)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int i = lane + 64 * j;
          if (i < kFbankLen) {
            const float prev = fl[f * 2 * FB_BS + max(i - 1, 0)];
            y[f][j] = (v[f][j] - 0.97f * prev) * lt->window[i];
          }
        }
      wave_lds_sync();
#pragma unroll
      for (int f = 0; f < FB_NF; ++f)
#pragma unroll
        for (int j = 0; j < 7; ++j) {
          const int i = lane + 64 * j;
          if (i < kFbankLen) fl[f * 2 * FB_BS + i] = y[f][j];
        }
    }
    wave_lds_sync();
    // z[m] = (y[2m], y[2m+1]) is the float array itself
    pass_batched<256, 4, 1, 512, FB_NF, FB_BS>(buf, lt->w512, lane);
    pass_batched<256, 4, 4, 512, FB_NF, FB_BS>(buf, lt->w512, lane);
    pass_batched<256, 4, 16, 512, FB_NF, FB_BS>(buf, lt->w512, lane);
    pass_batched<256, 4, 64, 512, FB_NF, FB_BS>(buf, lt->w512, lane);
    // real-input pass of the pair (k, 256 - k) and power spectrum
    {
      constexpr int TOT = FB_NF * 129, NT = (TOT + 63) / 64;
#pragma unroll
      for (int it = 0; it < NT; ++it) {
        const int idx = lane + 64 * it;
        if (idx < TOT) {
          const int f = idx / 129, k = idx - f * 129;
          const float2* bf = buf + f * FB_BS;
          const float2 zk = bf[k];
          const float2 zn = (k == 0) ? zk : bf[256 - k];
          float2 zc = cconj(zn);
          float2 fe = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
          float2 d = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
          float2 tt = cmul(lt->w512[k], make_float2(d.y, -d.x));
          const float2 xk = cadd(fe, tt);
          zc = cconj(zk);
          fe = make_float2(0.5f * (zn.x + zc.x), 0.5f * (zn.y + zc.y));
          d = make_float2(0.5f * (zn.x - zc.x), 0.5f * (zn.y - zc.y));
          tt = cmul(lt->w512[256 - k], make_float2(d.y, -d.x));
          const float2 xn = cadd(fe, tt);
          // in place: elements k and 256 - k belong to this work item alone, and both were read above
          fl[2 * (f * FB_BS + k)] = xk.x * xk.x + xk.y * xk.y;
          fl[2 * (f * FB_BS + 256 - k)] = xn.x * xn.x + xn.y * xn.y;
        }
      }
    }
    wave_lds_sync();
    // sparse triangular filters, f32 in tap order, log with the floor: one (frame, bin) per lane and step, rows stored whole
    {
      constexpr int TOT = FB_NF * kFbankBins, NT = (TOT + 63) / 64;
      static_assert(TOT % 64 == 0, "every lane has a (frame, bin)");
#pragma unroll
      for (int it = 0; it < NT; ++it) {
        const int idx = lane + 64 * it;
        const int f = idx / kFbankBins, m = idx - f * kFbankBins;
        const int meta = lt->meta[m];
        const int k0 = meta & 0xff, len = (meta >> 8) & 0xff;
        const float* w = lt->taps + (meta >> 16);
        const float* p = fl + 2 * (f * FB_BS + k0);
        float e = 0.0f;
        for (int q = 0; q < len; ++q) e += p[2 * q] * w[q];
        if (f0 + f < ch.n_frames) raw[(ch.row0 + f0 + f) * kFbankBins + m] = logf(fmaxf(e, 1.1920929e-07f));
      }
    }
    wave_lds_sync();
  }
}

__global__ __launch_bounds__(256) void fbank_means_kernel(const FbankChunk* __restrict__ chunks, int n_chunks, const float* raw, float* feats) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int c = idx / kFbankBins, m = idx - c * kFbankBins;
  if (c >= n_chunks) return;
  const FbankChunk ch = chunks[c];
  if (ch.n_frames < 1) return;
  const float* r = raw + ch.row0 * kFbankBins + m;
  float* o = feats + ch.row0 * kFbankBins + m;
  float sum = 0.0f;
  for (int t = 0; t < ch.n_frames; ++t) sum += r[(long)t * kFbankBins];
  const float mean = sum / (float)ch.n_frames;
  for (int t = 0; t < ch.n_frames; ++t) o[(long)t * kFbankBins] = r[(long)t * kFbankBins] - mean;
}

}  // namespace

// Window, twiddles and filters, worked out in double and rounded once.  The filters are kaldi-native-fbank's
// (mel-computations.cc): 80 triangles in mel space (1127 ln(1 + f / 700)) between 20 Hz and the Nyquist frequency over
// the FFT bins 0 ... 255.
bool fbank_tables(FbankTables& t) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 512; ++k) t.w512[k] = make_float2((float)std::cos(2.0 * pi * k / 512.0), (float)-std::sin(2.0 * pi * k / 512.0));
  for (int i = 0; i < kFbankLen; ++i) t.window[i] = (float)std::pow(0.5 - 0.5 * std::cos(2.0 * pi * i / (kFbankLen - 1)), 0.85);
  auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
  const double lo = mel(20.0), hi = mel(8000.0), delta = (hi - lo) / (kFbankBins + 1);
  int n_taps = 0;
  for (int i = 0; i < kFbankTaps + 3; ++i) t.taps[i] = 0.0f;
  for (int b = 0; b < kFbankBins; ++b) {
    const double left = lo + b * delta, center = left + delta, right = center + delta;
    int k0 = -1, len = 0;
    const int off = n_taps;
    for (int i = 0; i < kFbankFft / 2; ++i) {
      const double m = mel(16000.0 / kFbankFft * i);
      if (m > left && m < right) {
        const double w = m <= center ? (m - left) / (center - left) : (right - m) / (right - center);
        if (k0 < 0) k0 = i;
        if (n_taps < kFbankTaps) t.taps[n_taps] = (float)w;
        ++n_taps;
        len = i - k0 + 1;
      }
    }
    t.meta[b] = (k0 < 0 ? 0 : k0) | (len << 8) | (off << 16);
  }
  return n_taps == kFbankTaps;      // a property of the constants above
}

hipError_t launch_fbank_frames(const FbankTables* d_tab, const void* d_pcm, int pcm_format, float scale, const FbankChunk* d_chunks,
                               const FbankTile* d_tiles, int n_tiles, float* d_raw, hipStream_t st) {
  static_assert(FB_LDS <= 64 * 1024, "above the default dynamic-LDS limit");
  if (n_tiles < 1) return hipSuccess;
  if (pcm_format == CRISPY_PCM_F32)
    hipLaunchKernelGGL(fbank_frames_kernel<true>, dim3(n_tiles), dim3(256), FB_LDS, st, d_tab, d_pcm, scale, d_chunks, d_tiles, d_raw);
  else
    hipLaunchKernelGGL(fbank_frames_kernel<false>, dim3(n_tiles), dim3(256), FB_LDS, st, d_tab, d_pcm, scale, d_chunks, d_tiles, d_raw);
  return hipGetLastError();
}

hipError_t launch_fbank_means(const FbankChunk* d_chunks, int n_chunks, const float* d_raw, float* d_feats, hipStream_t st) {
  const int total = n_chunks * kFbankBins;
  hipLaunchKernelGGL(fbank_means_kernel, dim3((total + 255) / 256), dim3(256), 0, st, d_chunks, n_chunks, d_raw, d_feats);
  return hipGetLastError();
}

}  // namespace diar
}  // namespace crispy

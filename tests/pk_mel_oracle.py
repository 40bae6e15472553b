"""Parakeet's log-mel front end restated in torch (include/crispy_hip.h, "Parakeet front end"), in float64 or float32: what
transformers' ParakeetFeatureExtractor computes for one clip of 16 kHz mono f32 samples.  tests/test_pk_mel_oracle.py pins it against
the installed class and against tests/golden/parakeet_mel_golden.npz.

  pre-emphasis   y[0] = x[0], y[i] = x[i] - c x[i - 1] with c = f32(0.97), 0 for i >= n
  frames         rows = n // 160; frame t is 512 points from sample 160 t - 256 (zeros outside [0, n)) under a symmetric 400-point Hann
                 window at positions 56 ... 455, a real 512-point transform, re^2 + im^2 over bins 0 ... 256
  mel            the filters [M][257] over the bins, log(e + 2^-24)
  normalisation  per bin over the clip's rows: mean, std with the divisor rows - 1, (v - mean) / (std + f32(1e-5))

In float32 every step is f32 arithmetic, as the library's; in float64 the same operands (the f32 samples, the f32 filters, c and the
f32 constants) go through exact-enough arithmetic."""
import numpy as np
import torch

HOP, WIN, FFT, SPEC = 160, 400, 512, 257
COEF = float(np.float32(0.97))
GUARD = 2.0 ** -24
EPS = float(np.float32(1e-5))


def rows(samples: int) -> int:
    return max(int(samples), 0) // HOP


def slaney_filters(mel_bins: int) -> np.ndarray:
    """[M][257] f32: transformers.audio_utils.mel_filter_bank's Slaney filters restated in numpy float64, rounded once"""
    def to_mel(f):
        return 15.0 + np.log(f / 1000.0) * (27.0 / np.log(6.4)) if f >= 1000.0 else 3.0 * f / 200.0

    def to_hz(m):
        return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)

    edges = to_hz(np.linspace(to_mel(0.0), to_mel(8000.0), mel_bins + 2))
    freqs = np.linspace(0, 8000, SPEC)
    slopes = edges[None, :] - freqs[:, None]
    diff = np.diff(edges)
    fb = np.maximum(0, np.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]))
    fb = fb * (2.0 / (edges[2:mel_bins + 2] - edges[:mel_bins]))[None, :]
    return np.ascontiguousarray(fb.T.astype(np.float32))


def raw_rows(pcm, fb, dtype=torch.float64) -> torch.Tensor:
    """[rows][M] before the normalisation"""
    x = torch.from_numpy(np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)).to(dtype)
    n = x.shape[0]
    y = torch.cat([x[:1], x[1:] - COEF * x[:-1]])
    t = rows(n)
    padded = torch.cat([torch.zeros(FFT // 2, dtype=dtype), y, torch.zeros(FFT // 2 + HOP, dtype=dtype)])
    frames = padded.unfold(0, FFT, HOP)[:t]
    window = torch.zeros(FFT, dtype=dtype)
    window[(FFT - WIN) // 2:(FFT + WIN) // 2] = torch.hann_window(WIN, periodic=False, dtype=dtype)
    spec = torch.fft.rfft(frames * window, dim=-1)
    power = spec.real ** 2 + spec.imag ** 2
    mel = power @ torch.from_numpy(np.ascontiguousarray(fb, dtype=np.float32)).to(dtype).T
    return torch.log(mel + GUARD)


def normalise(raw: torch.Tensor):
    """rows [rows][M] of either dtype -> (normalised rows, mean [M], std [M]) in that dtype"""
    t = raw.shape[0]
    mean = raw.sum(0) / t
    std = torch.sqrt(((raw - mean) ** 2).sum(0) / (t - 1))
    return (raw - mean) / (std + EPS), mean, std


def features(pcm, fb, dtype=torch.float64):
    """one clip -> (rows [rows][M], rows before normalisation, mean [M], std [M]) as numpy arrays of `dtype`"""
    raw = raw_rows(pcm, fb, dtype)
    out, mean, std = normalise(raw)
    return out.numpy(), raw.numpy(), mean.numpy(), std.numpy()


def noise(samples: int, seed: int, amplitude: float = 0.1) -> np.ndarray:
    """seeded white noise: broadband, every bin's std well above rounding"""
    return (np.random.default_rng(seed).standard_normal(samples) * amplitude).astype(np.float32)


def ramped(samples: int, seed: int) -> np.ndarray:
    """white noise whose amplitude grows 30-fold over the clip (0.01 ... 0.3): broadband at every instant, and the two or three rows of
    a very short clip differ in every bin, so that no bin's std is rounding error alone"""
    gain = 0.01 * 30.0 ** (np.arange(samples) / max(samples - 1, 1))
    return (np.random.default_rng(seed).standard_normal(samples) * gain).astype(np.float32)


def speechlike(samples: int, seed: int) -> np.ndarray:
    """a cumulative sum of noise (a 1 / f^2 spectrum) with a slow envelope, on a broadband floor of 1e-2 of its peak"""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.standard_normal(samples))
    walk -= np.linspace(walk[0], walk[-1], samples)
    walk *= 0.5 + 0.5 * np.sin(np.arange(samples) * (2 * np.pi / 3200.0)) ** 2
    walk *= 0.5 / max(float(np.abs(walk).max()), 1e-9)
    return (walk + 5e-3 * rng.standard_normal(samples)).astype(np.float32)


def hf_extractor(mel_bins: int):
    """transformers' ParakeetFeatureExtractor without its constructor (which needs librosa): the module imported directly, the object
    built with __new__ plus SequenceFeatureExtractor.__init__, the filters from transformers.audio_utils.mel_filter_bank as f32"""
    import importlib

    from transformers.audio_utils import mel_filter_bank
    from transformers.feature_extraction_sequence_utils import SequenceFeatureExtractor
    mod = importlib.import_module("transformers.models.parakeet.feature_extraction_parakeet")
    cls = mod.ParakeetFeatureExtractor
    fe = cls.__new__(cls)
    SequenceFeatureExtractor.__init__(fe, feature_size=mel_bins, sampling_rate=16000, padding_value=0.0)
    fe.hop_length, fe.n_fft, fe.win_length, fe.preemphasis = HOP, FFT, WIN, 0.97
    fb = mel_filter_bank(SPEC, mel_bins, 0, 8000, 16000, norm="slaney", mel_scale="slaney")
    fe.mel_filters = torch.from_numpy(np.ascontiguousarray(fb.T)).to(torch.float32)
    return fe


def hf_features(fe, pcm) -> np.ndarray:
    """one clip through the library's class -> its rows [rows][M] f32"""
    out = fe([np.ascontiguousarray(pcm, dtype=np.float32)], sampling_rate=16000, return_tensors="pt")
    return out["input_features"][0, :rows(len(pcm))].numpy().astype(np.float32)

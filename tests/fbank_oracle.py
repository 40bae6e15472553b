"""Oracles of the diarization front end (include/crispy_hip.h, "Diarization front end"), written from the definitions:

* `fbank_raw` / `fbank`: the 80-bin Kaldi fbank of crispy_diar_fbank in numpy, every step in the dtype asked for
  (float64: the reference the GPU is measured against; float32: the stand-in for an f32 CPU implementation, whose own
  distance from float64 sets the tolerance of the GPU test).
* `speech_segments`: pyannote_get_segments_fixed (managers/diarization.rs:146-271) from the network's scores on, line
  by line in Python integers.
"""
import math

import numpy as np

N_BINS, FRAME, HOP, NFFT = 80, 400, 160, 512
EPS = 1.1920929e-07      # the mel floor: f32 machine epsilon, absolute


def f32_to_i16(x):
    """(s.clamp(-1, 1) * 32767.0) as i16: truncating, NaN -> 0"""
    x = np.asarray(x, np.float32)
    v = np.clip(x, np.float32(-1), np.float32(1)) * np.float32(32767.0)
    return np.where(np.isnan(v), np.float32(0), v).astype(np.int16)


def n_frames(n):
    return 0 if n < FRAME else 1 + (n - FRAME) // HOP


def povey(dtype=np.float64):
    i = np.arange(FRAME, dtype=np.float64)
    return ((0.5 - 0.5 * np.cos(2 * np.pi * i / (FRAME - 1))) ** 0.85).astype(dtype)


def mel_scale(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_filters(dtype=np.float64):
    """[80][257]: triangles in mel space between 20 Hz and 8000 Hz over the FFT bins 0 ... 255 (bin 256 has no weight)"""
    lo, hi = float(mel_scale(20.0)), float(mel_scale(8000.0))
    delta = (hi - lo) / (N_BINS + 1)
    mel = mel_scale(16000.0 / NFFT * np.arange(NFFT // 2))
    w = np.zeros((N_BINS, NFFT // 2 + 1))
    for b in range(N_BINS):
        left, center, right = lo + b * delta, lo + (b + 1) * delta, lo + (b + 2) * delta
        up, down = (mel - left) / (center - left), (right - mel) / (right - center)
        inside = (mel > left) & (mel < right)
        w[b, :NFFT // 2] = np.where(inside, np.where(mel <= center, up, down), 0.0)
    return w.astype(dtype)


def mel_energies(pcm_i16, scale, dtype=np.float64):
    """[frames][80] mel energies of one chunk before the floor and the log, every step in `dtype`"""
    t = dtype
    x = np.asarray(pcm_i16, np.int16).astype(t) / t(32768.0) * t(scale)
    nf = n_frames(len(x))
    if nf == 0:
        return np.zeros((0, N_BINS), t)
    idx = np.arange(nf)[:, None] * HOP + np.arange(FRAME)[None, :]
    fr = x[idx]
    fr = fr - (fr.sum(1, dtype=t) / t(FRAME))[:, None]
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], 1)
    fr = (fr - t(0.97) * prev) * povey(t)[None, :]
    pad = np.zeros((nf, NFFT), t)
    pad[:, :FRAME] = fr
    spec = np.fft.rfft(pad, axis=1)
    assert spec.dtype == (np.complex64 if t is np.float32 else np.complex128)
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(t)
    w = mel_filters(t)
    out = np.zeros((nf, N_BINS), t)
    for b in range(N_BINS):      # the taps of a bin in order, as a dot product over its support
        k = np.nonzero(w[b])[0]
        acc = np.zeros(nf, t)
        for q in k:
            acc = acc + power[:, q] * w[b, q]
        out[:, b] = acc
    return out


def fbank_raw(pcm_i16, scale, dtype=np.float64):
    return np.log(np.maximum(mel_energies(pcm_i16, scale, dtype), dtype(EPS)))


def subtract_mean(raw):
    """the per-chunk step in f32: the column sums in frame order / the frame count"""
    raw = np.asarray(raw, np.float32)
    if len(raw) == 0:
        return raw
    return raw - (np.add.accumulate(raw, 0)[-1] / np.float32(len(raw)))


def fbank(pcm_i16, scale, dtype=np.float64):
    raw = fbank_raw(pcm_i16, scale, dtype)
    return raw - raw.mean(0) if len(raw) else raw


# ---- speech segments ------------------------------------------------------------------------------------------------
def p_silence(scores):
    """float64 soft-max probability of class 0 per frame"""
    s = np.asarray(scores, np.float64)
    e = np.exp(s - s.max(-1, keepdims=True))
    return e[..., 0] / e.sum(-1)


def _as_usize(v):
    return 0 if not v > 0 else int(v)


def speech_segments(scores, n_samples, merge_gap, sample_rate=16000):
    """scores [n_windows][n_frames][n_classes] -> [(start s, end s, first sample, n samples)]"""
    scores = np.asarray(scores, np.float32)
    if n_samples == 0 or scores.shape[0] == 0:
        return []
    window_size, frame_step, frame_start = sample_rate * 10, 270, 721
    raw = []
    speech, start = False, 0
    for w in range(scores.shape[0]):
        labels = []
        for probs in scores[w]:
            mx = np.float32(-np.inf)
            for v in probs:
                mx = max(mx, v)
            sum_exp, p_sil = np.float32(0), np.float32(0)
            for i, v in enumerate(probs):
                e = np.exp(np.float32(v - mx))
                if i == 0:
                    p_sil = e
                sum_exp = np.float32(sum_exp + e)
            p_sil = np.float32(p_sil / sum_exp)
            labels.append(0 if p_sil > 0.5 else 1)
        smoothed = []
        for i in range(len(labels)):
            part = labels[max(i - 5, 0):min(i + 6, len(labels))]
            smoothed.append(1 if sum(part) > len(part) // 2 else 0)
        for i, lb in enumerate(smoothed):
            is_speech = lb == 1
            if is_speech != speech:
                idx = w * window_size + frame_start + i * frame_step
                if is_speech:
                    start = 0 if idx < 1600 else idx
                else:
                    s, e = min(start, n_samples), min(idx, n_samples)
                    if e > s:
                        raw.append((s, e))
                speech = is_speech
    if speech:
        s = min(start, n_samples)
        if n_samples > s:
            raw.append((s, n_samples))
    raw.sort(key=lambda x: x[0])      # stable
    gap, min_dur = _as_usize(sample_rate * merge_gap), _as_usize(sample_rate * 1.5)
    merged = []
    for s, e in raw:
        if merged and s <= merged[-1][1] + gap:
            merged[-1] = (merged[-1][0], max(merged[-1][1], e))
        else:
            merged.append((s, e))
    out = [(s, e) for s, e in merged if max(e - s, 0) >= min_dur]
    if not out and merged:
        best = merged[0]
        for m in merged[1:]:      # max_by_key: the last of equal maxima
            if m[1] - m[0] >= best[1] - best[0]:
                best = m
        out = [best]
    return [(s / sample_rate, e / sample_rate, s, e - s) for s, e in out]


def segmentation_windows(pcm_i16):
    x = np.asarray(pcm_i16, np.int16)
    if x.size == 0:
        return np.zeros((0, 160000), np.float32)
    n = math.ceil(x.size / 160000) + 1
    out = np.zeros(n * 160000, np.float32)
    out[:x.size] = x.astype(np.float32) / np.float32(32768.0)
    return out.reshape(n, 160000)

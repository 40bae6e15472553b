"""whisper.cpp's log-mel for a recording of ANY length, in float64 numpy: the formula of
tests/test_oracle_logmel.py::test_oracle_matches_numpy_stft, generalised.  whisper.cpp computes the log-mel of the whole
recording once -- reflect 200 in front, 30 s of zeros + 200 behind, (n + 480000) / 160 frames, ONE maximum -- and every
window of whisper_full's seek loop is frames [seek, seek + 3000) of it, clamped to max - 8, then (x + 4) / 4.
oracle/logmel_oracle.c is the same for n <= 480000; tests/test_long_logmel_oracle.py pins this form to it.

    raw(x)            -> [n_mel, (n + 480000) // 160] float64, log10 before normalisation
    window(raw, seek) -> [n_mel, 3000] float64
"""
from __future__ import annotations

import numpy as np

from crispy_amd.mel_filters import whisper_mel_filters

N_FRAMES = 3000
FLOOR = -10.0          # log10(1e-10): every frame that lies wholly in the zero padding


def n_len_org(n: int) -> int:
    """whisper.cpp's mel.n_len_org: the frames of the audio itself, the last seek a window may start at."""
    return 1 + (n + 200 - 400) // 160


def raw(x: np.ndarray, n_mel: int = 80, filters: np.ndarray | None = None) -> np.ndarray:
    F = (whisper_mel_filters(n_mel) if filters is None else np.asarray(filters)).astype(np.float64)
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    xp = np.concatenate([x[1:201][::-1], x, np.zeros(480000 + 200, np.float32)]).astype(np.float64)
    hann = 0.5 * (1 - np.cos(2 * np.pi * np.arange(400) / 400))
    n_len = (xp.size - 400) // 160
    assert n_len == (n + 480000) // 160
    out = np.full((F.shape[0], n_len), FLOOR)
    live = min(n_len, (n + 200 + 159) // 160)          # later frames see zeros only
    frames = np.lib.stride_tricks.sliding_window_view(xp, 400)[::160]
    for t0 in range(0, live, 8192):                    # in blocks: a 10 min clip would otherwise hold 0.4 GB at once
        t1 = min(live, t0 + 8192)
        P = np.abs(np.fft.rfft(frames[t0:t1] * hann, axis=1)) ** 2
        out[:, t0:t1] = np.log10(np.maximum(P @ F.T, 1e-10)).T
    return out


def window(r: np.ndarray, seek: int) -> np.ndarray:
    """Frames [seek, seek + 3000) of `r`, normalised with the maximum of the whole recording."""
    assert 0 <= seek
    w = r[:, seek:seek + N_FRAMES]
    if w.shape[1] < N_FRAMES:                          # past (n + 480000) / 160 (a seek beyond n_len_org): more zero padding
        w = np.concatenate([w, np.full((r.shape[0], N_FRAMES - w.shape[1]), FLOOR)], axis=1)
    return (np.maximum(w, r.max() - 8.0) + 4.0) / 4.0


def window_t(r: np.ndarray, seek: int) -> np.ndarray:
    """The frame-major layout the encoder reads: [3002, n_mel], one zero frame on either side."""
    w = window(r, seek)
    out = np.zeros((N_FRAMES + 2, w.shape[0]))
    out[1:-1] = w.T
    return out

"""Writes tests/golden/fbank_golden.npz: three 0.75 s signals (noise, a voiced harmonic stack plus noise, a pure tone)
quantised by f32_to_i16, and their Kaldi fbank rows (before the mean subtraction) at scale 1 and scale 32768 from an
implementation independent of this project: transformers.audio_utils.  Run from the repository root:

    python tests/golden/make_fbank_golden.py
"""
import os
import sys

import numpy as np
from transformers.audio_utils import mel_filter_bank, spectrogram, window_function

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests.fbank_oracle import f32_to_i16  # noqa: E402

N = 12000


def signals():
    rng = np.random.default_rng(20)
    t = np.arange(N) / 16000.0
    noise = 0.1 * rng.standard_normal(N)
    voiced = sum(0.3 / h * np.sin(2 * np.pi * 140.0 * h * t + h) for h in range(1, 20)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    voiced = voiced + 0.01 * rng.standard_normal(N)
    tone = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    return {"noise": noise, "voiced": voiced, "tone": tone}


def features(pcm_i16, scale):
    window = window_function(400, "povey", periodic=False)
    filters = mel_filter_bank(257, 80, 20, 8000, 16000, norm=None, mel_scale="kaldi", triangularize_in_mel_space=True)
    x = pcm_i16.astype(np.float64) / 32768.0 * scale
    out = spectrogram(x, window, frame_length=400, hop_length=160, fft_length=512, power=2.0, center=False, preemphasis=0.97,
                      mel_filters=filters, log_mel="log", mel_floor=1.192092955078125e-07, remove_dc_offset=True, dtype=np.float64)
    return np.ascontiguousarray(out.T)      # [frames][80]


def main():
    out = {}
    for name, sig in signals().items():
        q = f32_to_i16(sig.astype(np.float32))
        out[f"{name}_pcm"] = q
        out[f"{name}_scale1"] = features(q, 1.0)
        out[f"{name}_scale32768"] = features(q, 32768.0)
    path = os.path.join(HERE, "fbank_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

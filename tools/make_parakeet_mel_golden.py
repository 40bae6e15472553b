#!/usr/bin/env python3
"""Writes tests/golden/parakeet_mel_golden.npz: the rows transformers' ParakeetFeatureExtractor gives for three short clips (2, 3 and
36 rows) at 80 and 128 mel bins, with the clips themselves.  Recorded inputs and outputs only; tests/test_pk_mel_oracle.py holds
tests/pk_mel_oracle.py to them where transformers is not installed.

The object is built as tests/pk_mel_oracle.hf_extractor builds it (the constructor needs librosa): the filters are
transformers.audio_utils.mel_filter_bank's, as f32.  Needs transformers and torch; no device.

    python tools/make_parakeet_mel_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pk_mel_oracle as MO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "parakeet_mel_golden.npz")
CLIPS = (("rows2", MO.ramped, 337, 5), ("rows3", MO.ramped, 497, 5), ("rows36", MO.noise, 5800, 3))
BINS = (80, 128)


def main():
    import transformers
    data = {"transformers_version": np.array(transformers.__version__)}
    clips = {name: make(n, seed) for name, make, n, seed in CLIPS}
    for name, x in clips.items():
        data[f"pcm_{name}"] = x
    for M in BINS:
        fe = MO.hf_extractor(M)
        for name, x in clips.items():
            rows = MO.hf_features(fe, x)
            assert rows.shape == (MO.rows(len(x)), M) and np.isfinite(rows).all()
            data[f"rows_{M}_{name}"] = rows
    np.savez(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")


if __name__ == "__main__":
    main()

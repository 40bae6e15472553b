"""tests/long_logmel_oracle.py -- the float64 numpy log-mel for a recording of any length, the reference of
tests/test_gpu_long_audio.py -- pinned to the committed C oracle (oracle/logmel_oracle.c, n <= 480000 and seek <= 3000):
(a) directly, on clips the C oracle takes; (b) a long clip against the C oracle on 30 s slices of it, where both sides
are off their clamp floors (the two maxima differ: the clip's, and the slice's).  The bar is the project's own for this
pair, 2e-5 (tests/test_oracle_logmel.py::test_oracle_matches_numpy_stft)."""
import numpy as np
import pytest

BAR = 2e-5


@pytest.fixture(scope="module")
def F():
    from crispy_amd.mel_filters import whisper_mel_filters
    return whisper_mel_filters(80)


@pytest.mark.parametrize("n", [50000, 480000])
def test_numpy_long_form_equals_the_c_oracle_within_30_s(oracle, F, n):
    from crispy_amd import synth_audio
    from tests import long_logmel_oracle as LO
    x = synth_audio.clip16k_np(5, n)
    r = LO.raw(x, 80, F)
    assert r.shape == (80, (n + 480000) // 160)
    for seek in (0, 200, 1234, 2990, 3000):
        d = np.abs(LO.window(r, seek) - oracle.oracle_logmel(x, F, seek)).max()
        print(f"n {n} seek {seek}: max difference {d:.2e}")
        assert d < BAR, (n, seek, d)


def test_long_clip_equals_the_c_oracle_on_its_slices(oracle, F):
    from crispy_amd import synth_audio
    from tests import long_logmel_oracle as LO
    from tests.long_audio_cases import N_LONG
    x = synth_audio.clip16k_np(7, N_LONG)
    r = LO.raw(x, 80, F)
    assert r.shape == (80, (N_LONG + 480000) // 160)
    floor_long = (r.max() - 8.0 + 4.0) / 4.0
    for seek in (3000, 3008, 4400, 6600):
        sl = x[160 * seek:160 * seek + 480000]
        k = min(2998, (sl.size - 200) // 160)
        # frames [2, k): frame 0 and 1 of the slice reflect at ITS start, frames from k on see ITS zero padding
        a = LO.window(r, seek)[:, 2:k]
        full = oracle.oracle_logmel(sl, F, 0).astype(np.float64)
        b = full[:, 2:k]
        ok = (a > floor_long + 1e-6) & (b > full.max() - 2.0 + 1e-6)     # neither side on its clamp floor, (max - 8 + 4) / 4
        share = ok.mean()
        d = np.abs(a - b)[ok].max()
        print(f"seek {seek}: {k - 2} frames, {100 * share:.2f} % comparable, max difference {d:.2e}")
        assert share >= 0.99, (seek, share)
        assert d < BAR, (seek, d)


def test_silence_and_padding_are_the_floor():
    from tests import long_logmel_oracle as LO
    r = LO.raw(np.zeros(500000, np.float32))
    assert np.all(r == LO.FLOOR) and np.all(LO.window(r, LO.n_len_org(500000)) == (LO.FLOOR + 4.0) / 4.0)
    assert LO.n_len_org(480000) == 2999 and LO.n_len_org(1123457) == 7021


def test_real_clip_oracle_result_is_committed_with_todays_fingerprint():
    """tests/golden/oracle_cache/long_audio_real.json (written by `python -m tests.long_audio_cases`): tens of seconds of
    float64 encoder that the GPU suite must not recompute."""
    import json
    import os
    from tests import long_audio_cases as LC
    from tests.oracle_cache import CACHE_DIR
    path = os.path.join(CACHE_DIR, "long_audio_real.json")
    assert os.path.exists(path), "run python -m tests.long_audio_cases"
    blob = json.load(open(path))
    assert blob["fingerprint"] == LC.real_fingerprint()
    assert len(blob["value"]["wins"]) >= 2 and "wrong_last_avg_logprob" in blob["value"]

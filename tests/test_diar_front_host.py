"""CPU tests of the diarization front end (include/crispy_hip.h, "Diarization front end"): the new symbols on every layer, the
argument checks that need no device, crispy_diar_speech_segments against the line-by-line oracle of tests/fbank_oracle.py
on every edge of pyannote_get_segments_fixed (managers/diarization.rs:146-271), and the float64 fbank oracle against the
transformers.audio_utils fixture tests/golden/fbank_golden.npz."""
import ctypes as C
import os
import re

import numpy as np

from tests import fbank_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crispy_diar_fbank_frames", "crispy_diar_speech_segments", "crispy_diar_fbank_device", "crispy_diar_fbank")
N_FRAMES, N_CLASSES = 589, 7      # what segmentation-3.0 gives for a 10 s window
WIN = 160000


def _lib():
    from crispy_amd import _native as N
    return N, N.lib()


# ---- symbols and ABI ------------------------------------------------------------------------------------------------
def test_new_symbols_on_every_layer_and_abi_unchanged():
    N, L = _lib()
    assert N.DIAR_FRONT_SYMBOLS == NEW and set(NEW) <= set(N.ALL_SYMBOLS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crispy_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(L, s).argtypes is not None, s
        assert re.search(r"pub fn %s\(" % s, rust), s
    assert L.crispy_diar_fbank_frames.restype is C.c_long and L.crispy_diar_speech_segments.restype is C.c_long
    assert L.crispy_abi_version() == 6 == N.ABI_VERSION
    assert "#define CRISPY_ABI_VERSION 6" in hdr


def test_fbank_frames():
    from crispy_amd.diarize import fbank_frames
    assert [fbank_frames(n) for n in (0, 399, 400, 559, 560)] == [0, 0, 1, 1, 2]
    assert [O.n_frames(n) for n in (0, 399, 400, 559, 560, 64000)] == [0, 0, 1, 1, 2, 398]
    assert fbank_frames(64000) == 398


# ---- validation without a device ------------------------------------------------------------------------------------
def test_fbank_entry_points_validate_before_touching_a_device():
    N, L = _lib()
    first, ln, off = np.zeros(2, np.int64), np.array([400, 560], np.int64), np.zeros(3, np.int64)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_long))      # noqa: E731
    fake = C.c_void_p(1)      # never dereferenced: every case below fails (or ends) before the handle is used
    for dev in (True, False):
        def call(h, fmt, f, l, n, scale, o):
            if dev:
                return L.crispy_diar_fbank_device(h, None, fmt, f, l, n, scale, None, None, o, None)
            return L.crispy_diar_fbank(h, None, fmt, f, l, n, scale, None, o)
        assert call(None, N.PCM_I16, lp(first), lp(ln), 2, 1.0, lp(off)) == -1
        assert b"NULL handle" in L.crispy_last_error()
        assert call(fake, N.PCM_U16, lp(first), lp(ln), 2, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, lp(first), lp(ln), 0, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, lp(first), lp(ln), N.FBANK_MAX_CHUNKS + 1, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, None, lp(ln), 2, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, lp(first), None, 2, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, lp(first), lp(ln), 2, 1.0, None) == -1
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            assert call(fake, N.PCM_I16, lp(first), lp(ln), 2, scale, lp(off)) == -1, scale
        assert call(fake, N.PCM_I16, lp(np.array([0, -1], np.int64)), lp(ln), 2, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, lp(first), lp(np.array([400, -1], np.int64)), 2, 1.0, lp(off)) == -1
        assert call(fake, N.PCM_I16, lp(first), lp(np.array([400, N.FBANK_MAX_CHUNK_SAMPLES + 1], np.int64)), 2, 1.0, lp(off)) == -1
        # rows x 320 bytes above 2 GB: 224 chunks of the longest length
        big = np.full(224, N.FBANK_MAX_CHUNK_SAMPLES, np.int64)
        assert O.n_frames(int(big[0])) * 224 * 320 > 2 << 30
        assert call(fake, N.PCM_I16, lp(np.zeros(224, np.int64)), lp(big), 224, 1.0, lp(np.zeros(225, np.int64))) == -1
        assert b"2 GB" in L.crispy_last_error()
        # the sizing call: frame_offset from the lengths alone, no device
        off[:] = -1
        assert call(fake, N.PCM_F32, lp(first), lp(ln), 2, 32768.0, lp(off)) == 0
        assert off.tolist() == [0, 1, 3]


def test_speech_segments_validation():
    N, L = _lib()
    sc = np.zeros((1, 4, 3), np.float32)
    out = [np.zeros(4), np.zeros(4), np.zeros(4, np.int64), np.zeros(4, np.int64)]
    ptr = (out[0].ctypes.data_as(C.POINTER(C.c_double)), out[1].ctypes.data_as(C.POINTER(C.c_double)),
           out[2].ctypes.data_as(C.POINTER(C.c_long)), out[3].ctypes.data_as(C.POINTER(C.c_long)))
    f = L.crispy_diar_speech_segments
    assert f(sc.ctypes.data, 1, 4, 3, 1000, 8000, 0.5, *ptr, 4) == -1
    assert b"16 kHz" in L.crispy_last_error()
    for gap in (float("nan"), float("inf"), float("-inf")):
        assert f(sc.ctypes.data, 1, 4, 3, 1000, 16000, gap, *ptr, 4) == -1
    assert f(sc.ctypes.data, 1, 4, 0, 1000, 16000, 0.5, *ptr, 4) == -1
    assert f(sc.ctypes.data, 1, 0, 3, 1000, 16000, 0.5, *ptr, 4) == -1
    assert f(sc.ctypes.data, -1, 4, 3, 1000, 16000, 0.5, *ptr, 4) == -1
    assert f(sc.ctypes.data, 1, 4, 3, 1000, 16000, 0.5, None, None, None, None, 4) == -1
    assert f(None, 1, 4, 3, 1000, 16000, 0.5, *ptr, 4) == -1
    assert f(None, 0, 4, 3, 1000, 16000, 0.5, *ptr, 4) == 0
    assert f(sc.ctypes.data, 1, 4, 3, 0, 16000, 0.5, *ptr, 4) == 0


# ---- speech segments against the oracle -----------------------------------------------------------------------------
def scores_of(mask, seed=0):
    """logits whose soft-max puts ~0.98 on silence or on one of the speech classes, frame by frame"""
    mask = np.asarray(mask, bool)
    rng = np.random.default_rng(seed)
    sc = rng.uniform(-1.0, 0.0, mask.shape + (N_CLASSES,)).astype(np.float32)
    cls = np.where(mask, rng.integers(1, N_CLASSES, mask.shape), 0)
    np.put_along_axis(sc, cls[..., None], np.float32(6.0), -1)
    p = O.p_silence(sc)
    assert (np.abs(p - 0.5) > 0.1).all()      # no frame's decision is within reach of an f32 soft-max's rounding
    return sc


def mask(n_windows, spans):
    m = np.zeros((n_windows, N_FRAMES), bool)
    for w, a, b in spans:
        m[w, a:b] = True
    return m


def both(m, n_samples, merge_gap, seed=0):
    from crispy_amd.diarize import speech_segments
    sc = scores_of(m, seed)
    got, want = speech_segments(sc, n_samples, merge_gap), O.speech_segments(sc, n_samples, merge_gap)
    assert got == want, (got, want)
    return got


def test_speech_across_a_window_boundary_is_one_segment():
    got = both(mask(3, [(0, 400, N_FRAMES), (1, 0, 200)]), 2 * WIN - 5, 0.5)
    assert got == [((721 + 400 * 270) / 16000, (WIN + 721 + 200 * 270) / 16000, 721 + 400 * 270, WIN + 200 * 270 - 400 * 270)]


def test_early_start_snaps_to_zero():
    # speech from frame k on: the shortened median windows put the smoothed start at frame 0, 0, 1, 3 -- 721 + 270 i < 1600
    for k in (0, 1, 3, 4):
        got = both(mask(2, [(0, k, 150)]), WIN, 0.5)
        assert got[0][2] == 0 and got[0][3] == 721 + 150 * 270
    got = both(mask(2, [(0, 5, 150)]), WIN, 0.5)      # the smoothed start is frame 5: sample 2071
    assert got[0][2] == 721 + 5 * 270 and got[0][3] == 145 * 270


def test_open_speech_closes_at_the_end_and_ends_are_clamped():
    n = WIN + 50000
    got = both(mask(3, [(1, 20, N_FRAMES), (2, 0, N_FRAMES)]), n, 0.5)      # still speech when the windows run out
    assert got == [((WIN + 721 + 20 * 270) / 16000, n / 16000, WIN + 721 + 20 * 270, n - (WIN + 721 + 20 * 270))]
    got = both(mask(3, [(1, 20, 400)]), n, 0.5)      # the end, at WIN + 108721, lies beyond n_samples
    assert got[0][2] + got[0][3] == n
    assert both(mask(3, [(1, 300, 500)]), n, 0.5) == []      # wholly beyond: start clamps to the end, dropped


def test_median_filter_removes_glitches_also_at_the_window_edges():
    m = mask(2, [(0, 100, 300)])
    for i in (0, 2, 4, 50, 584, 586, 588):      # lone speech frames, the first and the last five of the window among them
        m[0, i] = True
    for i in (150, 200):      # lone silent frames inside speech
        m[0, i] = False
    m[1, 0] = m[1, 588] = True
    got = both(m, 2 * WIN, 0.0)
    assert got == [((721 + 100 * 270) / 16000, (721 + 300 * 270) / 16000, 721 + 100 * 270, 200 * 270)]
    # two of three at the very edge outvote the shortened window's integer half: frames 0, 1 of a 6-frame window are not
    # more than 3, frames 0 ... 3 are
    m = mask(2, [(0, 0, 4), (0, 100, 300)])
    both(m, 2 * WIN, 0.0)
    m = mask(2, [(0, 585, 589), (0, 100, 300)])
    both(m, 2 * WIN, 0.0)


def test_merge_gap_exactly_and_one_sample_more():
    # segments at frames [20, 120) and [130, 230): the gap is 10 * 270 = 2700 samples (too long for the median filter to close)
    m = mask(2, [(0, 20, 120), (0, 130, 230)])
    for gap_samples, count in ((2700, 1), (2699, 2)):
        sc = scores_of(m)
        gap = gap_samples / 16000.0
        assert int(16000 * gap) == gap_samples
        from crispy_amd.diarize import speech_segments
        got, want = speech_segments(sc, WIN, gap), O.speech_segments(sc, WIN, gap)
        assert got == want and len(got) == count, (gap_samples, got)


def test_minimum_duration_exactly_and_one_sample_less():
    # a span ending at n_samples: 24000 samples is kept, 23999 is dropped beside a longer one
    start = 721 + 120 * 270
    for dur, kept in ((24000, 2), (23999, 1)):
        n = start + dur
        got = both(mask(2, [(0, 5, 97), (0, 120, N_FRAMES)]), n, 0.0)      # [2071, 26911): 24840 samples, and the clamped one
        assert len(got) == kept and got[0][3] == 92 * 270
        if kept == 2:
            assert got[1][2:] == (start, 24000)


def test_fallback_keeps_the_last_of_two_equally_long():
    got = both(mask(2, [(0, 20, 60), (0, 200, 240), (0, 400, 430)]), WIN, 0.0)
    assert got == [((721 + 200 * 270) / 16000, (721 + 240 * 270) / 16000, 721 + 200 * 270, 40 * 270)]


def test_empty_input_and_cap_smaller_than_the_count():
    N, L = _lib()
    from crispy_amd.diarize import speech_segments
    assert speech_segments(np.zeros((0, N_FRAMES, N_CLASSES), np.float32), 1000, 0.5) == []
    assert speech_segments(scores_of(mask(2, [(0, 20, 300)])), 0, 0.5) == []
    assert both(mask(2, []), WIN, 0.5) == []
    sc = scores_of(mask(2, [(0, 20, 120), (0, 200, 300), (0, 400, 500)]))
    want = O.speech_segments(sc, WIN, 0.0)
    assert len(want) == 3
    s, e = np.full(3, -1.0), np.full(3, -1.0)
    f, n = np.full(3, -1, np.int64), np.full(3, -1, np.int64)
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_long)
    cnt = L.crispy_diar_speech_segments(sc.ctypes.data, 2, N_FRAMES, N_CLASSES, WIN, 16000, 0.0, s.ctypes.data_as(dp), e.ctypes.data_as(dp),
                                        f.ctypes.data_as(lp), n.ctypes.data_as(lp), 2)
    assert cnt == 3
    assert [(s[i], e[i], f[i], n[i]) for i in range(2)] == want[:2]
    assert (s[2], e[2], f[2], n[2]) == (-1.0, -1.0, -1, -1)


def test_segmentation_windows():
    from crispy_amd.diarize import f32_to_i16, segmentation_windows
    x = f32_to_i16(np.random.default_rng(1).uniform(-1.2, 1.2, WIN + 7).astype(np.float32))
    w = segmentation_windows(x)
    assert w.shape == (3, WIN) and w.dtype == np.float32
    assert np.array_equal(w, O.segmentation_windows(x))
    assert np.array_equal(w.reshape(-1)[:x.size] * 32768, x.astype(np.float32)) and not w.reshape(-1)[x.size:].any()
    assert segmentation_windows(x[:WIN]).shape == (2, WIN) and segmentation_windows(x[:0]).shape == (0, WIN)
    edge = np.array([1.5, -1.5, np.inf, -np.inf, np.nan, -0.0, 1 / 32767, np.nextafter(np.float32(2 / 32767), np.float32(0))], np.float32)
    assert f32_to_i16(edge).tolist() == [32767, -32767, 32767, -32767, 0, 0, 1, 1]
    assert np.array_equal(f32_to_i16(edge), O.f32_to_i16(edge))


# ---- the float64 oracle against an independent implementation ---------------------------------------------------------
def test_f64_oracle_matches_the_transformers_fixture():
    g = np.load(os.path.join(ROOT, "tests", "golden", "fbank_golden.npz"))
    assert int((O.mel_filters() > 0).sum()) == 501
    for name in ("noise", "voiced", "tone"):
        for scale in (1, 32768):
            ref = g[f"{name}_scale{scale}"]
            got = O.fbank_raw(g[f"{name}_pcm"], float(scale))
            assert got.shape == ref.shape == (73, 80)
            err = float(np.abs(got - ref).max())
            print(f"fbank oracle vs fixture, {name} x{scale}: {err:.2e}")
            assert err <= 1e-5
    tone = O.mel_energies(g["tone_pcm"], 1.0)
    assert (tone < O.EPS).mean() > 0.2 and not (O.mel_energies(g["tone_pcm"], 32768.0) < O.EPS).any()      # why scale is a parameter

"""CPU tests of the segmentation network's entry points (include/crispy_hip.h, "Segmentation network"): the new symbols on every
layer, the frame and window counts against the torch oracle of tests/seg_oracle.py, and every check crispy_diar_seg_load and
the forward / recording entry points make before a device is touched (a fake handle is never dereferenced)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import seg_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crispy_diar_seg_frames", "crispy_diar_seg_windows", "crispy_diar_seg_load", "crispy_diar_seg_loaded",
       "crispy_diar_seg_forward_device", "crispy_diar_seg_scores_device", "crispy_diar_seg_scores")
WIN = 160000


def _lib():
    from crispy_amd import _native as N
    return N, N.lib()


@pytest.fixture(scope="module")
def weights():
    return SO.make_weights(1)


def test_new_symbols_on_every_layer_and_abi_unchanged():
    N, L = _lib()
    assert N.DIAR_SEG_SYMBOLS == NEW and set(NEW) <= set(N.ALL_SYMBOLS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crispy_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(L, s).argtypes is not None, s
        assert re.search(r"pub fn %s\(" % s, rust), s
    assert L.crispy_diar_seg_frames.restype is C.c_long and L.crispy_diar_seg_windows.restype is C.c_long
    assert L.crispy_abi_version() == 6 == N.ABI_VERSION
    assert "#define CRISPY_ABI_VERSION 6" in hdr


def test_frames_equal_the_oracles_output_length(weights):
    from crispy_amd.diarize import seg_frames
    net = SO.PyanNet(weights, dtype=__import__("torch").float32)
    rng = np.random.default_rng(2)
    for n in (990, 991, 992, 1260, 1261, 3691, 8000, 159999, 160000):
        x = (0.1 * rng.standard_normal((1, n))).astype(np.float32)
        if n == 990:      # the last pooling is left with two positions: torch refuses, the count is 0
            with pytest.raises(RuntimeError):
                net.scores(x)
            want = 0
        else:
            want = net.scores(x).shape[1]
        assert seg_frames(n) == want == SO.n_frames(n), (n, seg_frames(n), want)
    assert seg_frames(991) == 1 and seg_frames(WIN) == 589 and seg_frames(0) == 0 and seg_frames(-5) == 0


def test_windows_equal_segmentation_windows():
    from crispy_amd.diarize import seg_windows, segmentation_windows
    for n in (0, 1, WIN, WIN + 1):
        assert seg_windows(n) == len(segmentation_windows(np.zeros(n, np.int16))) == len(SO.segmentation_windows(np.zeros(n, np.int16))), n
    assert [seg_windows(n) for n in (0, 1, WIN, WIN + 1)] == [0, 2, 2, 3]


def _load(L, h, tensors, counts=None, null=None):
    names = list(tensors)
    arrs = [np.ascontiguousarray(tensors[k], dtype=np.float32).reshape(-1) for k in names]
    cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
    cd = (C.c_void_p * len(names))(*[None if k == null else a.ctypes.data for k, a in zip(names, arrs)])
    cnt = np.array([a.size if counts is None or k not in counts else counts[k] for k, a in zip(names, arrs)], np.int64)
    rc = L.crispy_diar_seg_load(h, cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), len(names))
    return rc, L.crispy_last_error()


def test_load_validates_before_touching_a_device(weights):
    N, L = _lib()
    fake = C.c_void_p(1)      # never dereferenced: every case below fails before the handle is used
    assert len(weights) == 51
    rc, msg = _load(L, None, weights)
    assert rc == -1 and b"NULL handle" in msg
    assert L.crispy_diar_seg_loaded(None) == 0
    # a missing tensor, one of each family
    for name in ("sincnet.conv1d.0.filters", "lstm.weight_hh_l2_reverse", "classifier.bias", "sincnet.wav_norm1d.weight"):
        rc, msg = _load(L, fake, {k: v for k, v in weights.items() if k != name})
        assert rc == -1 and name.encode() in msg and b"missing" in msg, (name, msg)
    # a duplicate: the same name twice in the list
    names = list(weights) + ["linear.1.bias"]
    arrs = [np.ascontiguousarray(weights[k]).reshape(-1) for k in names]
    cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
    cd = (C.c_void_p * len(names))(*[a.ctypes.data for a in arrs])
    cnt = np.array([a.size for a in arrs], np.int64)
    assert L.crispy_diar_seg_load(fake, cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), len(names)) == -1
    assert b"linear.1.bias" in L.crispy_last_error() and b"twice" in L.crispy_last_error()
    # an unknown name (ONNX's fused LSTM tensor, say)
    rc, msg = _load(L, fake, dict(weights, **{"lstm.W_l0": np.zeros(4, np.float32)}))
    assert rc == -1 and b"lstm.W_l0" in msg and b"unknown" in msg
    # a count off by one, either way
    for name, off in (("lstm.weight_ih_l0", -1), ("sincnet.norm1d.1.bias", 1), ("sincnet.conv1d.0.filters", -1)):
        rc, msg = _load(L, fake, weights, counts={name: int(np.asarray(weights[name]).size) + off})
        assert rc == -1 and name.encode() in msg, (name, msg)
    # a NULL pointer
    rc, msg = _load(L, fake, weights, null="linear.0.weight")
    assert rc == -1 and b"linear.0.weight" in msg and b"NULL" in msg
    # a NaN and an infinite weight
    for name, bad in (("lstm.bias_hh_l3", np.nan), ("sincnet.conv1d.2.weight", np.inf)):
        w = dict(weights)
        w[name] = np.array(weights[name], np.float32)
        w[name].reshape(-1)[-1] = bad
        rc, msg = _load(L, fake, w)
        assert rc == -1 and name.encode() in msg and b"non-finite" in msg, (name, msg)
    lp = C.POINTER(C.c_long)
    assert L.crispy_diar_seg_load(fake, None, None, None, 51) == -1
    assert L.crispy_diar_seg_load(fake, cn, cd, cnt.ctypes.data_as(lp), 0) == -1


def test_forward_and_scores_validate_before_touching_a_device():
    N, L = _lib()
    fake, buf = C.c_void_p(1), C.c_void_p(64)      # never dereferenced
    fwd = L.crispy_diar_seg_forward_device
    assert fwd(None, buf, 1, WIN, buf, None, None, None) == -1 and b"NULL handle" in L.crispy_last_error()
    for ln in (990, WIN + 1, 0, -1):
        assert fwd(fake, buf, 1, ln, buf, None, None, None) == -1 and b"len" in L.crispy_last_error(), ln
    for n_win in (0, -1, N.SEG_MAX_WINDOWS + 1):
        assert fwd(fake, buf, n_win, WIN, buf, None, None, None) == -1 and b"n_win" in L.crispy_last_error(), n_win
    assert fwd(fake, None, 1, WIN, buf, None, None, None) == -1
    assert fwd(fake, buf, 1, WIN, None, None, None, None) == -1
    for dev in (True, False):
        def call(h, pcm, fmt, n, out):
            if dev:
                return L.crispy_diar_seg_scores_device(h, pcm, fmt, n, out, None)
            return L.crispy_diar_seg_scores(h, pcm, fmt, n, out)
        assert call(None, buf, N.PCM_I16, 100, buf) == -1 and b"NULL handle" in L.crispy_last_error()
        assert call(fake, buf, N.PCM_U16, 100, buf) == -1 and b"pcm_format" in L.crispy_last_error()
        for n in (0, -1, N.SEG_MAX_SAMPLES + 1):
            assert call(fake, buf, N.PCM_I16, n, buf) == -1 and b"n_samples" in L.crispy_last_error(), n
        assert call(fake, None, N.PCM_F32, 100, buf) == -1
        assert call(fake, buf, N.PCM_F32, 100, None) == -1


def test_run_diarization_without_a_network_is_a_clear_error():
    from crispy_amd import diarize as D

    class NoNetwork:
        segmentation_loaded = False

    with pytest.raises(ValueError, match="no segmentation network is loaded"):
        D.run_diarization(np.zeros(1000, np.int16), None, lambda f: f, 2, 0.5, NoNetwork())

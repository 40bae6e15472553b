"""GPU tests of the segmentation network (crispy_diar_seg_*, include/crispy_hip.h) against tests/seg_oracle.py: scores and both
stage outputs within a bound taken from the float32 torch oracle's own distance to the float64 oracle, on short windows over
every pooling remainder and on full windows (a zero window among them); batch, position and turn independence byte for byte;
the recording entry points against the forward; a reload; and run_diarization end to end with seg_fn=None.

The bound (the rule of tests/test_gpu_diar_fbank.py): per case and per tensor, the GPU's largest distance to float64 stays
within 4 x the float32 oracle's.  Both are f32 arithmetic on the same operands; a different but equally valid summation order
over K <= 400 taps and up to 589 recurrent steps lands within a small multiple of another implementation's error.  Where the
float32 oracle is exact (a tensor both compute without rounding) the bound is 0 and the GPU has to be exact as well."""
import ctypes as C

import numpy as np
import pytest

from tests import fbank_oracle as FO
from tests import seg_oracle as SO
from tests.native_variant import library_variant

pytestmark = pytest.mark.gpu

SR, WIN = 16000, 160000
FACTOR = 4.0
# short windows: (c0 % 3, c1 % 3, c2 % 3), the positions each MaxPool1d(3) drops -- every remainder at every stage; 991 is one frame
SHORT = {991: (0, 0, 0), 5000: (1, 1, 2), 6001: (0, 2, 1), 12345: (1, 0, 0), 15000: (2, 1, 2), 22222: (2, 2, 1)}
E2E_WEIGHTS, E2E_CLASSIFIER, E2E_RECORDING = 1, 9594, 100      # chosen on the CPU: see test_run_diarization_end_to_end


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def weights():
    return SO.make_weights(1)


@pytest.fixture(scope="module")
def oracles(weights):
    import torch
    return SO.PyanNet(weights, torch.float64), SO.PyanNet(weights, torch.float32)


@pytest.fixture(scope="module")
def diar(weights):
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    d.load_segmentation(weights)
    yield d
    d.close()


def check(got, x, oracles, what):
    """got = (scores, sincnet, lstm) of the GPU on windows x -> the ratios GPU / float32 oracle, per tensor"""
    o64, o32 = oracles
    r64, r32 = o64.forward(x), o32.forward(x)
    ratios = []
    for name, g, a, b in zip(("scores", "sincnet", "lstm"), got, r64, r32):
        assert g.shape == a.shape, (what, name, g.shape, a.shape)
        assert np.isfinite(g).all(), (what, name)
        yard = float(np.abs(b.astype(np.float64) - a).max())
        err = float(np.abs(g.astype(np.float64) - a).max())
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
        print(f"seg {what} {name}: float32 oracle {yard:.3e}, GPU {err:.3e} from float64 (ratio {ratio:.2f}, bound {FACTOR:g})")
        ratios.append((name, err, yard))
    for name, err, yard in ratios:
        assert err <= FACTOR * yard, (what, name, err, yard)
    return ratios


def signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.2 * np.sin(2 * np.pi * 220.0 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 2.0 * t)) + 0.05 * rng.standard_normal(n)
    return FO.f32_to_i16(x.astype(np.float32)).astype(np.float32) / np.float32(32768.0)


@pytest.mark.parametrize("n", list(SHORT))
def test_short_windows_every_floor(diar, oracles, n):
    from crispy_amd.diarize import seg_frames
    assert SO.pool_remainders(n) == SHORT[n] and seg_frames(n) == SO.n_frames(n) >= 1
    for stage in range(3):
        assert {r[stage] for r in SHORT.values()} == {0, 1, 2}
    x = np.stack([signal(n, 3), signal(n, 4)[::-1].copy()])
    check(diar.seg_forward(x, taps=True), x, oracles, f"len {n}")


def full_windows():
    rng = np.random.default_rng(5)
    burst = (1e-4 * rng.standard_normal(WIN)).astype(np.float32)
    burst[70000:74000] += (0.8 * rng.standard_normal(4000)).astype(np.float32)
    burst = FO.f32_to_i16(np.clip(burst, -1, 1)).astype(np.float32) / np.float32(32768.0)
    return np.stack([signal(WIN, 6), burst, np.zeros(WIN, np.float32)])


def test_full_windows(diar, oracles):
    x = full_windows()
    got = diar.seg_forward(x, taps=True)
    assert got[0].shape == (3, 589, 7)
    for w, what in enumerate(("tone plus noise", "silence with a burst", "all zeros")):
        check(tuple(g[w:w + 1] for g in got), x[w:w + 1], oracles, what)
    # log_softmax: every row sums to one
    assert np.abs(np.exp(got[0].astype(np.float64)).sum(-1) - 1.0).max() < 1e-5


def test_bytes_alone_in_a_batch_and_in_turns(diar, weights):
    from crispy_amd.diarize import Diarizer
    x = full_windows()
    mine = x[0:1]
    alone = diar.seg_forward(mine, taps=True)
    first = diar.seg_forward(np.concatenate([mine, x[1:3]]), taps=True)
    five = np.concatenate([x[1:3], x[1:3], mine])
    fifth = diar.seg_forward(five, taps=True)
    for a, b, c in zip(alone, first, fifth):
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[0]), bits(c[4]))
    # the developer build with turns of 2 windows: 2 + 2 + 1, the bytes of the single turn
    with library_variant("dev", {"CRISPY_DIAR_SEG_TURN": "2"}):
        d = Diarizer(0)
        try:
            d.load_segmentation(weights)
            turns = d.seg_forward(five, taps=True)
        finally:
            d.close()
    for a, b in zip(fifth, turns):
        assert np.array_equal(bits(a), bits(b))
    short = np.stack([signal(6001, 8 + i) for i in range(5)])
    with library_variant("dev", {"CRISPY_DIAR_SEG_TURN": "2"}):
        d = Diarizer(0)
        try:
            d.load_segmentation(weights)
            turns = d.seg_forward(short, taps=True)
        finally:
            d.close()
    for a, b in zip(diar.seg_forward(short, taps=True), turns):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("n", [1, WIN, WIN + 1, 250000])
def test_recording_entry(diar, n):
    import torch
    from crispy_amd.diarize import f32_to_i16, seg_windows, segmentation_windows
    rng = np.random.default_rng(n % 1000)
    f = rng.uniform(-1.2, 1.2, n).astype(np.float32)
    f[:min(n, 4)] = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)[:min(n, 4)]
    x = f32_to_i16(f)
    want = diar.seg_forward(segmentation_windows(x))
    got = diar.segmentation_scores(x)
    assert got.shape == want.shape == (seg_windows(n), 589, 7) and np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(diar.segmentation_scores(f)), bits(want))      # f32 through f32_to_i16 on the device
    dev = diar.segmentation_scores_device(torch.from_numpy(x).cuda())
    assert np.array_equal(bits(dev.cpu().numpy()), bits(want))
    dev = diar.segmentation_scores_device(torch.from_numpy(f).cuda())
    assert np.array_equal(bits(dev.cpu().numpy()), bits(want))


def test_reload_and_forward_before_a_load(oracles):
    import torch
    from crispy_amd.diarize import Diarizer
    from crispy_amd import _native as N
    x = np.stack([signal(12345, 21), signal(12345, 22)])
    d = Diarizer(0)
    try:
        assert not d.segmentation_loaded
        with pytest.raises(N.CrispyError, match="no segmentation network is loaded") as e:
            d.seg_forward(x)
        assert e.value.code == -1
        with pytest.raises(N.CrispyError, match="no segmentation network is loaded"):
            d.segmentation_scores(np.zeros(100, np.int16))
        d.load_segmentation(SO.make_weights(1))
        assert d.segmentation_loaded
        first = d.seg_forward(x, taps=True)
        check(first, x, oracles, "first load")
        second_w = SO.make_weights(2)
        d.load_segmentation(second_w)
        second = d.seg_forward(x, taps=True)
        check(second, x, (SO.PyanNet(second_w, torch.float64), SO.PyanNet(second_w, torch.float32)), "second load")
        assert not np.array_equal(bits(first[0]), bits(second[0]))
    finally:
        d.close()


# ---- end to end -----------------------------------------------------------------------------------------------------
def recording(seed):
    """25 s: a quiet noise floor with four loud stretches (an amplitude-modulated tone plus noise) at seeded places"""
    rng = np.random.default_rng(seed)
    n = 25 * SR
    x = 0.002 * rng.standard_normal(n)
    t = np.arange(n) / SR
    edges = np.sort(rng.uniform(1.0, 24.0, 8))
    for a, b in zip(edges[0::2], edges[1::2]):
        s, e = int(a * SR), int(b * SR)
        f0 = rng.uniform(100, 300)
        x[s:e] += 0.3 * np.sin(2 * np.pi * f0 * t[s:e]) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t[s:e])) + 0.1 * rng.standard_normal(e - s)
    return FO.f32_to_i16(np.clip(x, -1, 1).astype(np.float32))


PROJ = np.random.default_rng(29).standard_normal((80, 48))


def emb_stub(feats):
    """a fixed random projection of the per-bin standard deviation of the features (about its mean over the bins)"""
    sd = np.asarray(feats, np.float64).std(0)
    return ((sd - sd.mean()) @ PROJ).astype(np.float32)


def test_run_diarization_end_to_end():
    """The weights' classifier seed and the recording's seed were chosen on the CPU so that the float64 oracle alone gives both
    states at least 10 % of the frames, at least four changes of state after the median filter, and no frame with
    |p_sil - 0.5| < 1e-3 (found: 58 % speech, 13 changes, the closest frame at 4.0e-3); asserted here before anything is compared."""
    import torch
    from crispy_amd import diarize as D
    w = SO.make_weights(E2E_WEIGHTS, classifier_seed=E2E_CLASSIFIER)
    x = recording(E2E_RECORDING)
    windows = SO.segmentation_windows(x)
    s64 = SO.PyanNet(w, torch.float64).scores(windows)
    p = FO.p_silence(s64)
    speech = p <= 0.5
    smoothed = np.zeros_like(speech)
    for i in range(speech.shape[1]):
        a, b = max(i - 5, 0), min(i + 6, speech.shape[1])
        smoothed[:, i] = speech[:, a:b].sum(1) > (b - a) // 2
    flat = smoothed.reshape(-1)
    changes = int((flat[1:] != flat[:-1]).sum())
    print(f"end to end fixture: {speech.mean():.3f} speech, {changes} changes, closest frame {np.abs(p - 0.5).min():.2e}")
    assert 0.1 <= speech.mean() <= 0.9 and changes >= 4 and np.abs(p - 0.5).min() >= 1e-3
    o32 = SO.PyanNet(w, torch.float32)
    merge_gap, max_speakers = 0.5, 2
    d = D.Diarizer(0)
    try:
        d.load_segmentation(w)
        got = D.run_diarization(x, None, emb_stub, max_speakers, merge_gap, d)
        want = D.run_diarization(x, lambda win: o32.scores(win[None])[0], emb_stub, max_speakers, merge_gap, d)
        segs = D.speech_segments(d.segmentation_scores(x), x.size, merge_gap)
    finally:
        d.close()
    assert segs == D.speech_segments(s64.astype(np.float32), x.size, merge_gap) and len(segs) >= 1
    assert len(want) >= 1 and got == want, (got, want)

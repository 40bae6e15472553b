"""CPU tests of Parakeet's log-mel front end: tests/pk_mel_oracle.py pinned against transformers' ParakeetFeatureExtractor (where it is
installed) and against the rows recorded from it in tests/golden/parakeet_mel_golden.npz (everywhere), the built-in filter table
against transformers.audio_utils.mel_filter_bank and against the oracle's restatement, and crispy_pk_feature_rows.

The pin: the library's f32 rows lie within 4 x the float32 restatement's own distance to the float64 restatement.  Both are f32
arithmetic on the same operands, so they land within a small multiple of each other's rounding error of the exact result; a wrong
window position, row count or variance divisor shows at 1e-2 or more, a thousand times the yardstick (1e-5 ... 1e-4)."""
import importlib.util
import os

import numpy as np
import pytest

from tests import pk_mel_oracle as MO

FACTOR = 4.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parakeet_mel_golden.npz")
HAVE_HF = importlib.util.find_spec("transformers") is not None
CLIPS = (("ramped 337", MO.ramped, 337, 5), ("ramped 497", MO.ramped, 497, 5), ("noise 6200", MO.noise, 6200, 3), ("speech-like 20000", MO.speechlike, 20000, 4))


def ordered(a):
    """f32 -> integers whose differences count ulps; -0 (numpy's maximum(0, -0.0) keeps the sign) and +0 are the same number"""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def pin(lib_rows, pcm, mel_bins, what):
    import torch
    fb = MO.slaney_filters(mel_bins)
    r64 = MO.features(pcm, fb, torch.float64)[0]
    r32 = MO.features(pcm, fb, torch.float32)[0]
    assert lib_rows.shape == r64.shape == (MO.rows(len(pcm)), mel_bins), (what, lib_rows.shape, r64.shape)
    yard = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(lib_rows.astype(np.float64) - r64).max())
    print(f"pk mel pin {what} M={mel_bins}: float32 restatement {yard:.3e}, library {err:.3e} from float64 (ratio {err / yard:.2f}, bound {FACTOR:g})")
    assert 0.0 < yard < 1e-3, (what, yard)
    assert err <= FACTOR * yard, (what, mel_bins, err, yard)


@pytest.mark.skipif(not HAVE_HF, reason="transformers is not installed (the golden file carries the pin)")
@pytest.mark.parametrize("mel_bins", [80, 128])
def test_oracle_matches_the_installed_feature_extractor(mel_bins):
    fe = MO.hf_extractor(mel_bins)
    for what, make, n, seed in CLIPS:
        x = make(n, seed)
        pin(MO.hf_features(fe, x), x, mel_bins, what)


@pytest.mark.skipif(not HAVE_HF, reason="transformers is not installed")
def test_a_clip_does_not_depend_on_its_batch():
    """5000 samples alone and beside a 2 s clip: the library's rows of the short clip are the same"""
    fe = MO.hf_extractor(80)
    a, b = MO.noise(5000, 11), MO.noise(32000, 12)
    alone = MO.hf_features(fe, a)
    both = fe([a, b], sampling_rate=16000, return_tensors="pt")["input_features"][0, :MO.rows(5000)].numpy()
    assert float(np.abs(alone - both).max()) == 0.0


@pytest.mark.parametrize("mel_bins", [80, 128])
def test_oracle_matches_the_recorded_rows(mel_bins):
    g = np.load(GOLDEN)
    names = sorted(k[len("pcm_"):] for k in g.files if k.startswith("pcm_"))
    assert names == ["rows2", "rows3", "rows36"]
    for name in names:
        pcm = g[f"pcm_{name}"]
        assert pcm.dtype == np.float32
        pin(g[f"rows_{mel_bins}_{name}"], pcm, mel_bins, f"golden {name}")
    assert [MO.rows(len(g[f"pcm_{n}"])) for n in names] == [2, 3, 36]


def test_golden_file_is_small_and_holds_arrays_only():
    assert os.path.getsize(GOLDEN) < 64 * 1024
    g = np.load(GOLDEN, allow_pickle=False)
    for k in g.files:
        assert g[k].dtype in (np.float32,) or k == "transformers_version", k


@pytest.mark.parametrize("mel_bins", [80, 128, 1, 17, 64])
def test_built_in_filters(mel_bins):
    """crispy_pk_mel_filters (host only, no device) against mel_filter_bank and the oracle's restatement: within 1 ulp of f32"""
    from crispy_amd.parakeet import pk_mel_filters
    got = pk_mel_filters(mel_bins)
    refs = [MO.slaney_filters(mel_bins)]
    if HAVE_HF:
        from transformers.audio_utils import mel_filter_bank
        refs.append(np.ascontiguousarray(mel_filter_bank(MO.SPEC, mel_bins, 0, 8000, 16000, norm="slaney", mel_scale="slaney").T.astype(np.float32)))
    for ref in refs:
        assert got.shape == ref.shape == (mel_bins, MO.SPEC)
        assert ((got != 0) == (ref != 0)).all()
        ulp = np.abs(ordered(got) - ordered(ref))
        assert int(ulp.max()) <= 1, int(ulp.max())
    assert (got >= 0).all() and (got.sum(1) > 0).all()


def test_built_in_filters_limits():
    from crispy_amd import _native as N
    from crispy_amd.parakeet import pk_mel_filters
    for bad in (0, -1, 129):
        with pytest.raises(N.CrispyError, match="mel_bins"):
            pk_mel_filters(bad)


def test_feature_rows():
    from crispy_amd.parakeet import pk_feature_rows
    assert [pk_feature_rows(n) for n in (0, 319, 320, 479, 480, 6_400_000, 6_400_160)] == [0, 1, 2, 2, 3, 40000, 40001]
    assert pk_feature_rows(-5) == 0 and pk_feature_rows(159) == 0 and pk_feature_rows(160) == 1
    assert all(pk_feature_rows(n) == MO.rows(n) for n in range(0, 2000, 7))

"""GPU tests of Parakeet's log-mel front end and of the whole arm (crispy_pk_features*, crispy_pk_set_mel_filters, crispy_pk_transcribe*,
include/crispy_hip.h) against tests/pk_mel_oracle.py: the rows before and after normalisation on clips at every edge of the row count
and of the frame kernel's tile, the transform bin by bin through identity filter banks, the clip's own edges (large last samples,
neighbours 1e4 times larger), batch, position and call independence byte for byte, the normalisation alone from the device's own
rows up to 40 000 of them, a silent clip, the limits, and samples to words against the three stages called one after the other.

The bound (the rule of tests/test_gpu_parakeet_encoder.py): per clip and per tensor, the GPU's largest distance to float64 stays within
4 x the float32 oracle's.  Both are f32 arithmetic on the same operands.  A bin whose values over the clip are rounding error alone
would make the normalised rows noise in every implementation, so the inputs are broadband (noise, or a floor of noise under a tone)
and every ratio test asserts that each bin's float64 std is at least 0.05.  The short clips use seed 5 of pk_mel_oracle.ramped: of
seeds 1 ... 8 it is one whose two or three rows differ by that much in all 128 bins -- a property of the float64 oracle alone."""
import numpy as np
import pytest

from tests import pk_mel_oracle as MO

pytestmark = pytest.mark.gpu

FACTOR = 4.0
MIN_STD = 0.05
TILE = 32      # frames of one workgroup of the frame kernel (crispy_amd._native.PK_MEL_TILE_FRAMES, asserted below)
# samples: 2 rows at the least, 2 rows one sample on, 2 rows at the most, 3 rows, an odd 2-row clip; one tile less a row, a tile to the
# last sample, a tile and a row; three tiles with a last one of six rows (a wave's second batch of frames half empty)
EDGES = (320, 321, 479, 480, 337, 160 * (TILE - 1), 160 * TILE + 159, 160 * (TILE + 1), 160 * 70 + 3)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def edge_clip(n):
    return MO.ramped(n, 5) if n < 1000 else MO.noise(n, n)


def ratio(got, r64, r32, what):
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert np.isfinite(got).all(), what
    yard = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(got.astype(np.float64) - r64).max())
    r = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    print(f"pk mel {what}: float32 oracle {yard:.3e}, GPU {err:.3e} from float64 (ratio {r:.2f}, bound {FACTOR:g})")
    return err, yard


def check_clip(pcm, fb, got_rows, got_raw, what):
    """the GPU's rows before and after normalisation of one clip against the oracles"""
    import torch
    r64, r32 = MO.features(pcm, fb, torch.float64), MO.features(pcm, fb, torch.float32)
    assert float(r64[3].min()) >= MIN_STD, (what, float(r64[3].min()))
    pairs = [ratio(got_raw, r64[1], r32[1], f"{what} raw"), ratio(got_rows, r64[0], r32[0], f"{what} rows")]
    for err, yard in pairs:
        assert err <= FACTOR * yard, (what, err, yard)


@pytest.fixture(scope="module")
def enc():
    """a handle without a load: the front end needs none"""
    from crispy_amd import ParakeetEncoder
    e = ParakeetEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def edge_clips():
    return [edge_clip(n) for n in EDGES]


@pytest.fixture(scope="module")
def edge_gpu(enc, edge_clips):
    """(rows, raw rows, stats) per clip of the edge clips in ONE ragged call, per mel_bins; shared, unchanged"""
    return {M: enc.features(edge_clips, mel_bins=M, taps=True) for M in (80, 128)}


def test_tile_constant():
    from crispy_amd import _native as N
    assert N.PK_MEL_TILE_FRAMES == TILE


# ---- 1. rows before and after normalisation at the edges ----------------------------------------------------------------------
@pytest.mark.parametrize("mel_bins", [80, 128])
def test_edges_against_the_oracle(edge_clips, edge_gpu, mel_bins):
    fb = MO.slaney_filters(mel_bins)
    rows, raw, _stats = edge_gpu[mel_bins]
    for n, pcm, a, b in zip(EDGES, edge_clips, rows, raw):
        assert a.shape == (n // 160, mel_bins)
        check_clip(pcm, fb, a, b, f"M={mel_bins} {n} samples")


# ---- 2. the transform, bin by bin ------------------------------------------------------------------------------------------------
def tone_clip():
    n = 3000
    t = np.arange(n)
    tone = np.linspace(0.1, 0.5, n) * np.sin(2 * np.pi * 1000.0 / 16000.0 * t)
    return (MO.noise(n, 21, 0.05) + tone).astype(np.float32)


def identity_banks():
    lo, hi, last = np.zeros((128, 257), np.float32), np.zeros((128, 257), np.float32), np.zeros((1, 257), np.float32)
    lo[np.arange(128), np.arange(128)] = 1.0
    hi[np.arange(128), 128 + np.arange(128)] = 1.0
    last[0, 256] = 1.0
    return (("bins 0-127", lo), ("bins 128-255", hi), ("bin 256", last))


def test_transform_bin_by_bin_and_filter_override(enc):
    import torch
    pcm = tone_clip()
    before = enc.features([pcm], mel_bins=128, taps=True)
    try:
        for what, fb in identity_banks():
            enc.set_mel_filters(fb)
            _rows, raw, _stats = enc.features([pcm], mel_bins=fb.shape[0], taps=True)
            r64, r32 = MO.features(pcm, fb, torch.float64), MO.features(pcm, fb, torch.float32)
            assert float(r64[3].min()) >= MIN_STD, (what, float(r64[3].min()))
            err, yard = ratio(raw[0], r64[1], r32[1], f"identity {what} raw")
            assert err <= FACTOR * yard, (what, err, yard)
        from crispy_amd import _native as N
        with pytest.raises(N.CrispyError, match="mel_bins"):      # the filters set have 1 bin
            enc.features([pcm], mel_bins=128)
        with pytest.raises(N.CrispyError, match="4096"):          # 17 x 257 = 4369 taps
            enc.set_mel_filters(np.ones((17, 257), np.float32))
        got = enc.features([pcm], mel_bins=1, taps=True)          # the refused matrix left the handle as it was
        assert np.array_equal(bits(got[1][0]), bits(raw[0]))
    finally:
        enc.set_mel_filters(None)
    after = enc.features([pcm], mel_bins=128, taps=True)
    for a, b in zip(before, after):
        assert np.array_equal(bits(a[0]), bits(b[0]))
    check_clip(pcm, MO.slaney_filters(128), after[0][0], after[1][0], "tone clip, built-in filters")


# ---- 3. the clip's own edges ------------------------------------------------------------------------------------------------------
def loud_end_clip():
    x = MO.noise(1000, 31)
    x[-6:] = np.float32(40.0) * np.array([1, -1, 1, 1, -1, 1], np.float32)
    return x


def test_large_last_samples(enc):
    """y[n] = 0: a front end that forms x[n] - 0.97 x[n - 1] behind the clip's end sees -0.97 x 40 there"""
    pcm = loud_end_clip()
    alone = enc.features([pcm], mel_bins=128, taps=True)
    check_clip(pcm, MO.slaney_filters(128), alone[0][0], alone[1][0], "large last samples")
    batch = enc.features([MO.noise(700, 32), pcm, MO.noise(650, 33)], mel_bins=128, taps=True)
    for a, b in zip(alone, batch):
        assert np.array_equal(bits(a[0]), bits(b[1]))


def test_neighbours_1e4_times_larger(enc, edge_clips, edge_gpu):
    big = [(MO.noise(n, s) * np.float32(1e4)).astype(np.float32) for n, s in ((1123, 41), (960, 42))]
    for i in (0, 4, 6):      # 320 samples, 337 samples, a whole tile to the last sample
        got = enc.features([big[0], edge_clips[i], big[1]], mel_bins=128, taps=True)
        for a, b in zip(got, edge_gpu[128]):
            assert np.array_equal(bits(a[1]), bits(b[i])), EDGES[i]


def test_batch_position_and_call_independence(enc, edge_clips, edge_gpu):
    for M in (80, 128):
        again = enc.features(edge_clips, mel_bins=M, taps=True)
        k = 4
        rotated = enc.features(edge_clips[k:] + edge_clips[:k], mel_bins=M, taps=True)
        for first, second, rot in zip(edge_gpu[M], again, rotated):
            for i in range(len(EDGES)):
                assert np.array_equal(bits(first[i]), bits(second[i])), (M, EDGES[i])
                assert np.array_equal(bits(first[i]), bits(rot[(i - k) % len(EDGES)])), (M, EDGES[i])
        alone = enc.features([edge_clips[-1]], mel_bins=M, taps=True)
        for first, one in zip(edge_gpu[M], alone):
            assert np.array_equal(bits(first[-1]), bits(one[0])), M


def test_device_form_matches_host_form(enc, edge_clips, edge_gpu):
    import torch
    got = enc.features_device([torch.from_numpy(c).cuda() for c in edge_clips], mel_bins=128, taps=True)
    for dev, host in zip(got, edge_gpu[128]):
        for a, b in zip(dev, host):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b))
    plain = enc.features_device([torch.from_numpy(c).cuda() for c in edge_clips], mel_bins=128)      # NULL taps
    for a, b in zip(plain, edge_gpu[128][0]):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


# ---- 4. the normalisation alone ------------------------------------------------------------------------------------------------------
def check_normalisation(raw, rows, stats, what):
    """from the device's own rows before normalisation: its rows and statistics against torch's in float64, by the rule"""
    import torch
    r64 = MO.normalise(torch.from_numpy(raw).to(torch.float64))
    r32 = MO.normalise(torch.from_numpy(raw))
    pairs = [ratio(rows, r64[0].numpy(), r32[0].numpy(), f"{what} normalised"), ratio(stats[0], r64[1].numpy(), r32[1].numpy(), f"{what} mean"),
             ratio(stats[1], r64[2].numpy(), r32[2].numpy(), f"{what} std")]
    assert float(r64[2].min()) >= MIN_STD, (what, float(r64[2].min()))
    for err, yard in pairs:
        assert err <= FACTOR * yard, (what, err, yard)


@pytest.mark.parametrize("mel_bins", [80, 128])
def test_normalisation_from_the_device_rows(edge_gpu, mel_bins):
    rows, raw, stats = edge_gpu[mel_bins]
    for i, n in enumerate(EDGES):
        check_normalisation(raw[i], rows[i], stats[i], f"M={mel_bins} {n} samples")


def test_normalisation_at_40000_rows(enc):
    pcm = MO.noise(160 * 40000 + 100, 51)
    rows, raw, stats = enc.features([pcm], mel_bins=128, taps=True)
    assert rows[0].shape == (40000, 128)
    check_normalisation(raw[0], rows[0], stats[0], "40000 rows")


def test_silent_clip(enc):
    for M in (80, 128):
        rows, raw, stats = enc.features([np.zeros(1700, np.float32), MO.noise(500, 61)], mel_bins=M, taps=True)
        floor = np.float32(np.log(np.float64(2.0 ** -24)))
        assert raw[0].shape == (10, M) and (raw[0] == floor).all(), (raw[0].min(), raw[0].max(), floor)
        assert np.array_equal(bits(rows[0]), np.zeros((10, M), np.uint32))      # exactly +0
        assert (stats[0][0] == floor).all() and (stats[0][1] == 0).all()


def test_limits(enc):
    from crispy_amd import _native as N
    ok = MO.noise(400, 71)
    with pytest.raises(N.CrispyError, match="clip 1 has 319 samples"):
        enc.features([ok, MO.noise(319, 72)], mel_bins=128)
    with pytest.raises(N.CrispyError, match="clip 0 has 40001 rows"):
        enc.features([np.zeros(160 * 40001, np.float32)], mel_bins=128)
    for bad in (0, 129):
        with pytest.raises(N.CrispyError, match="mel_bins"):
            enc.features([ok], mel_bins=bad)
    with pytest.raises(N.CrispyError, match="n_clips"):
        enc.features([], mel_bins=128)
    assert enc.features([ok], mel_bins=1)[0].shape == (2, 1)      # any width from 1


# ---- 5. samples to words --------------------------------------------------------------------------------------------------------
def test_transcribe_equals_the_three_stages(enc):
    import torch

    from crispy_amd import Parakeet, ParakeetTDT
    from crispy_amd import _native as N
    from crispy_amd.parakeet import pk_feature_rows, pk_frames, pk_tdt_words
    from tests import pk_oracle as PO
    from tests import pk_tdt_oracle as TO
    state = {"encoder." + k: v for k, v in PO.make_weights(PO.TINY, 1).items()}
    state.update(TO.make_tdt_weights(TO.TINY_TDT, 3))
    clips = [MO.speechlike(16000, 81), MO.noise(4003, 82), MO.speechlike(9100, 83)]
    pieces = [(TO.MARK if i % 3 == 0 else "") + f"p{i}" for i in range(TO.TINY_TDT.vocab)]
    pk = Parakeet(0)
    try:
        with pytest.raises(N.CrispyError, match="no encoder is loaded"):
            pk.transcribe(clips)
        pk.encoder.load(PO.TINY.as_dict(), state)
        with pytest.raises(N.CrispyError, match="no decoder is loaded"):
            pk.transcribe(clips)
        pk.load(PO.TINY.as_dict(), TO.TINY_TDT.as_dict(), state)
        with pytest.raises(N.CrispyError, match="mel_bins"):      # after a load the width is the encoder's
            pk.encoder.features(clips, mel_bins=80)
        feats = pk.encoder.features(clips)
        for a, b in zip(feats, enc.features(clips, mel_bins=128)):      # the same rows as a handle without a load
            assert np.array_equal(bits(a), bits(b))
        frames = pk.encoder.encode(feats)
        want = pk.decoder.decode(frames)
        got = pk.transcribe(clips, pieces)
        dev = pk.transcribe_device([torch.from_numpy(c).cuda() for c in clips], pieces)
        raw_dev = pk.transcribe_device([torch.from_numpy(c).cuda() for c in clips])
        for c, (g, d, r, w) in enumerate(zip(got, dev, raw_dev, want)):
            t = pk_frames(pk_feature_rows(len(clips[c])))
            assert frames[c].shape[0] == t
            assert g["steps"].dtype == np.int32 and np.array_equal(g["steps"], w) and np.array_equal(d["steps"], w)
            assert np.array_equal(r["steps"].cpu().numpy(), w)
            words = pk_tdt_words(w, pieces, t, TO.TINY_TDT.blank)
            print(f"pk transcribe clip {c}: {t} frames, {len(w)} steps, {len(words)} words")
            assert g["words"] == words and d["words"] == words
            assert g["text"] == " ".join(x for _a, _b, x in words).strip() == d["text"]
        assert sum(len(g["steps"]) for g in got) > 0
        again = pk.transcribe(clips[::-1])
        for a, b in zip(again[::-1], want):
            assert np.array_equal(a["steps"], b)
        other = ParakeetTDT(0)
        try:
            narrow = TO.TdtConfig(hidden=128, decoder_hidden=128, decoder_layers=2, vocab=33, blank=32)
            other.load(narrow.as_dict(), TO.make_tdt_weights(narrow, 3))
            mine, pk.decoder = pk.decoder, other
            with pytest.raises(N.CrispyError, match="hidden"):
                pk.transcribe(clips)
            pk.decoder = mine
        finally:
            other.close()
    finally:
        pk.close()

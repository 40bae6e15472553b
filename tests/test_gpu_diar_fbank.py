"""GPU tests of the Kaldi fbank of the diarization front end (crispy_diar_fbank*, include/crispy_hip.h) against
tests/fbank_oracle.py: the rows before the mean subtraction within a bound taken from the float32 restatement's own
distance to float64, the mean subtraction bit for bit, every chunk length at which the kernel takes another path, batch
independence byte for byte, the f32 entry against the i16 entry, the limits, and run_diarization end to end with stub
networks against the oracle composition."""
import ctypes as C

import numpy as np
import pytest

from tests import fbank_oracle as O
from tests import nme_sc_oracle as NO

pytestmark = pytest.mark.gpu

SR = 16000
WAVE_F, TILE_F, BATCH_F = 8, 32, 4      # crispy_amd/csrc/diar_internal.h: frames per wave and per workgroup; diar_fbank.hip: FB_NF


@pytest.fixture(scope="module")
def diar():
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    yield d
    d.close()


def run(diar, pcm, chunks, scale):
    """-> (feats, raw, frame_offset) as numpy"""
    import torch
    feats, raw, off = diar.fbank_device(torch.from_numpy(np.ascontiguousarray(pcm)).cuda(), chunks, scale, raw=True)
    return feats.cpu().numpy(), raw.cpu().numpy(), off


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_raw(raw, pcm_i16, scale, what):
    """|raw - log(max(m_ref, eps))| <= log1p(tau * m_frame_max / max(m_ref, eps)) + 2^-22 * max(1, |raw_ref|), tau = 4 x the float32
    restatement's own largest |m32 - m64| / m_frame_max on this input.  Returns (the f32 ratio, the GPU's observed ratio)."""
    m64 = O.mel_energies(pcm_i16, scale, np.float64)
    m32 = O.mel_energies(pcm_i16, scale, np.float32).astype(np.float64)
    assert raw.shape == m64.shape, (what, raw.shape, m64.shape)
    if len(m64) == 0:
        return 0.0, 0.0
    fmax = m64.max(1, keepdims=True)
    live = fmax[:, 0] > 0      # an all-zero frame is exact in every arithmetic
    assert not m32[~live].any()
    r32 = float((np.abs(m32 - m64)[live] / fmax[live]).max()) if live.any() else 0.0
    tau = 4.0 * r32
    ref = np.log(np.maximum(m64, O.EPS))
    bound = np.log1p(tau * fmax / np.maximum(m64, O.EPS)) + 2.0 ** -22 * np.maximum(1.0, np.abs(ref))
    err = np.abs(raw.astype(np.float64) - ref)
    above = live[:, None] & (m64 > O.EPS)
    rgpu = float((np.abs(np.exp(raw.astype(np.float64)) - m64) / np.where(fmax > 0, fmax, 1.0))[above].max()) if above.any() else 0.0
    print(f"fbank {what} x{scale:g}: f32 restatement {r32:.2e}, GPU (through its log) {rgpu:.2e} of the frame maximum; "
          f"worst error / bound {float((err / bound).max()):.2f}")
    assert (err <= bound).all(), (what, scale, float((err / bound).max()))
    return r32, rgpu


def signals():
    rng = np.random.default_rng(7)
    n = SR
    t = np.arange(n) / SR
    voiced = sum(0.3 / h * np.sin(2 * np.pi * 140.0 * h * t + h) for h in range(1, 20)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t))
    half = 0.1 * rng.standard_normal(n)
    half[:n // 2] = 0
    return {
        "noise_0.1": 0.1 * rng.standard_normal(n),
        "voiced": voiced + 0.01 * rng.standard_normal(n),
        "tone_1k": 0.5 * np.sin(2 * np.pi * 1000.0 * t),
        "noise_0.001": 0.001 * rng.standard_normal(n),
        "half_silence": half,
        "clipped": np.clip(1.0 * rng.standard_normal(n), -1, 1),
    }


SIGNALS = {k: O.f32_to_i16(v.astype(np.float32)) for k, v in signals().items()}


@pytest.mark.parametrize("scale", [1.0, 32768.0])
@pytest.mark.parametrize("name", list(SIGNALS))
def test_values_against_the_f64_oracle(diar, name, scale):
    x = SIGNALS[name]
    feats, raw, off = run(diar, x, [(0, len(x))], scale)
    assert off.tolist() == [0, 98]
    check_raw(raw, x, scale, name)
    assert np.array_equal(bits(feats), bits(O.subtract_mean(raw)))


def test_mean_subtraction_bit_for_bit(diar):
    rng = np.random.default_rng(11)
    x = O.f32_to_i16((0.2 * rng.standard_normal(9000)).astype(np.float32))
    x[6000:] = 0
    chunks = [(0, 5000), (100, 400), (6100, 2000), (0, 9000), (2000, 560)]
    feats, raw, off = run(diar, x, chunks, 32768.0)
    for c in range(len(chunks)):
        r, f = raw[off[c]:off[c + 1]], feats[off[c]:off[c + 1]]
        assert len(r) == O.n_frames(chunks[c][1])
        assert np.array_equal(bits(f), bits(r - (np.add.accumulate(r, 0)[-1] / np.float32(len(r))))), c
    assert not bits(feats[off[1]:off[2]]).any()      # one frame: every value +0.0
    zero = raw[off[2]:off[3]]                        # all-zero samples: the floor alone
    assert (bits(zero) == bits(zero)[0, 0]).all() and abs(float(zero[0, 0]) - np.log(O.EPS)) <= 2.0 ** -22 * abs(np.log(O.EPS))


def ragged_lengths():
    lens = [0, 399, 400, 559, 560, 64000]
    for f in (BATCH_F, WAVE_F, TILE_F):      # F - 1, F, F and F + 1 frames
        lens += [160 * f + 239, 160 * f + 240, 160 * f + 241, 160 * f + 400]
    return lens


def test_lengths_and_raggedness(diar):
    rng = np.random.default_rng(13)
    x = O.f32_to_i16((0.1 * rng.standard_normal(70000)).astype(np.float32))
    lens = ragged_lengths()
    firsts = [int(v) for v in rng.integers(0, 70000 - 64000, len(lens))]
    firsts[5] = 0
    firsts[3] = 69000      # out of order, and overlapping the others
    chunks = list(zip(firsts, lens))
    feats, raw, off = run(diar, x, chunks, 32768.0)
    assert off.tolist() == np.concatenate([[0], np.cumsum([O.n_frames(n) for n in lens])]).tolist()
    filler = [(int(a), int(b)) for a, b in zip(rng.integers(0, 60000, 32), rng.integers(0, 3000, 32))]
    for c, (first, n) in enumerate(chunks):
        mine_f, mine_r = feats[off[c]:off[c + 1]], raw[off[c]:off[c + 1]]
        check_raw(mine_r, x[first:first + n], 32768.0, f"len {n}")
        a_f, a_r, a_off = run(diar, x, [(first, n)], 32768.0)
        assert a_off.tolist() == [0, O.n_frames(n)]
        assert np.array_equal(bits(a_f), bits(mine_f)) and np.array_equal(bits(a_r), bits(mine_r)), n
        pos = (5 * c + 3) % 33
        b_f, b_r, b_off = run(diar, x, filler[:pos] + [(first, n)] + filler[pos:], 32768.0)
        assert np.array_equal(bits(b_f[b_off[pos]:b_off[pos + 1]]), bits(mine_f)), (n, pos)
        assert np.array_equal(bits(b_r[b_off[pos]:b_off[pos + 1]]), bits(mine_r)), (n, pos)


def test_host_entry_equals_device_entry(diar):
    rng = np.random.default_rng(17)
    x = O.f32_to_i16((0.1 * rng.standard_normal(12000)).astype(np.float32))
    chunks = [(3000, 5000), (11000, 399), (2000, 400), (5000, 7000)]      # the upload starts at the smallest first with rows
    feats, _raw, off = run(diar, x, chunks, 1.0)
    got = diar.fbank(x, chunks, 1.0)
    assert [len(g) for g in got] == [O.n_frames(n) for _f, n in chunks]
    for c in range(len(chunks)):
        assert np.array_equal(bits(got[c]), bits(feats[off[c]:off[c + 1]])), c
    assert [g.shape for g in diar.fbank(x, [(0, 100), (50, 399)], 1.0)] == [(0, 80), (0, 80)]


def test_f32_entry_equals_i16_entry_bit_for_bit(diar):
    rng = np.random.default_rng(19)
    x = rng.uniform(-1.3, 1.3, 4000).astype(np.float32)
    k = np.arange(1, 200, dtype=np.float32)
    exact = k / np.float32(32767.0)
    special = np.concatenate([[1.5, -1.5, np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, -1.0], exact, -exact,
                              np.nextafter(exact, np.float32(2)), np.nextafter(exact, np.float32(-2)),
                              -np.nextafter(exact, np.float32(2)), -np.nextafter(exact, np.float32(-2))]).astype(np.float32)
    x[100:100 + len(special)] = special
    q = O.f32_to_i16(x)
    assert q[100:106].tolist() == [32767, -32767, 32767, -32767, 0, 0]
    chunks = [(0, 4000), (90, 1000)]
    for scale in (1.0, 32768.0):
        f_feats, f_raw, f_off = run(diar, x, chunks, scale)
        i_feats, i_raw, i_off = run(diar, q, chunks, scale)
        assert f_off.tolist() == i_off.tolist()
        assert np.array_equal(bits(f_raw), bits(i_raw)) and np.array_equal(bits(f_feats), bits(i_feats))
        assert np.isfinite(f_raw).all()


def test_limits_are_invalid_arg_before_any_launch(diar):
    import torch
    from crispy_amd import _native as N
    L = diar._L
    pcm = torch.zeros(1000, dtype=torch.int16, device="cuda")
    feats = torch.full((4, 80), 7.0, device="cuda")
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_long))      # noqa: E731
    torch.cuda.synchronize()

    def call(first, ln, n, scale=1.0, fmt=N.PCM_I16, d_pcm=pcm.data_ptr()):
        first, ln = np.asarray(first, np.int64), np.asarray(ln, np.int64)
        off = np.zeros(max(n, 0) + 1, np.int64)
        return L.crispy_diar_fbank_device(diar._h, d_pcm, fmt, lp(first), lp(ln), n, scale, feats.data_ptr(), None, lp(off), None)

    assert call([0], [560], 0) == -1
    assert call(np.zeros(N.FBANK_MAX_CHUNKS + 1), np.zeros(N.FBANK_MAX_CHUNKS + 1), N.FBANK_MAX_CHUNKS + 1) == -1
    assert call([0], [N.FBANK_MAX_CHUNK_SAMPLES + 1], 1) == -1
    assert call([0], [-1], 1) == -1
    assert call([-1], [560], 1) == -1
    assert call(np.zeros(224), np.full(224, N.FBANK_MAX_CHUNK_SAMPLES), 224) == -1
    for scale in (0.0, -2.0, float("inf"), float("nan")):
        assert call([0], [560], 1, scale=scale) == -1
    assert call([0], [560], 1, fmt=N.PCM_U16) == -1
    assert call([0], [560], 1, d_pcm=None) == -1
    torch.cuda.synchronize()
    assert (feats == 7.0).all()      # nothing was written
    assert call([0], [560], 1) == 0
    torch.cuda.synchronize()
    assert not (feats[:2] == 7.0).any() and (feats[2:] == 7.0).all()


# ---- end to end -----------------------------------------------------------------------------------------------------
def two_speaker_audio():
    """40 s: two "speakers" as noise with opposite spectral tilts -- A loud below 2 kHz, B loud above -- whose loud band is
    amplitude-modulated at 3 Hz, separated by silences.  (The features have their per-chunk mean removed, so a constant tilt
    alone leaves no trace in them; the modulation of the loud band does, in the per-bin standard deviation.)"""
    rng = np.random.default_rng(23)
    n = 40 * SR
    spec = np.fft.rfft(rng.standard_normal(n))
    cut = int(2000 / (SR / 2) * (len(spec) - 1))
    lo, hi = spec.copy(), spec.copy()
    lo[cut:] = 0
    hi[:cut] = 0
    lo, hi = np.fft.irfft(lo, n), np.fft.irfft(hi, n)
    lo, hi = lo / lo.std(), hi / hi.std()
    mod = 1.0 + 0.9 * np.sin(2 * np.pi * 3.0 * np.arange(n) / SR)
    a, b = 0.1 * lo * mod + 0.01 * hi, 0.1 * hi * mod + 0.01 * lo
    x = np.zeros(n)
    who = [i % 2 for i in range(8)]      # eight turns of 4.2 s (two chunks each), 0.8 s of silence between them
    for i, w in enumerate(who):
        s, e = int((0.5 + 5 * i) * SR), int((0.5 + 5 * i + 4.2) * SR)
        x[s:e] = (a, b)[w][s:e]
    return x.astype(np.float32), who


def seg_stub(window):
    """+-5 logits from the RMS of the 270 samples around each frame's centre"""
    w = np.asarray(window, np.float64)
    fr = w[586:586 + 589 * 270].reshape(589, 270)
    speech = np.sqrt((fr * fr).mean(1)) > 0.002
    sc = np.full((589, 7), -5.0, np.float32)
    sc[:, 0] = np.where(speech, -5.0, 5.0)
    sc[:, 1] = np.where(speech, 5.0, -5.0)
    return sc


PROJ = np.random.default_rng(29).standard_normal((80, 48))


def emb_stub(feats):
    """a fixed random projection of the per-bin standard deviation of the features (about its mean over the bins)"""
    sd = np.asarray(feats, np.float64).std(0)
    return ((sd - sd.mean()) @ PROJ).astype(np.float32)


def test_run_diarization_end_to_end(diar):
    from crispy_amd import diarize as D
    audio, who = two_speaker_audio()
    merge_gap, max_speakers = 0.5, 2
    got = D.run_diarization(audio, seg_stub, emb_stub, max_speakers, merge_gap, diar)
    # the oracle composition: numpy fbank, tests/nme_sc_oracle.py, the existing host functions
    x = O.f32_to_i16(audio)
    scores = np.stack([seg_stub(w) for w in O.segmentation_windows(x)])
    assert (np.abs(O.p_silence(scores) - 0.5) > 0.1).all()
    segs = O.speech_segments(scores, len(x), merge_gap)
    assert len(segs) == 8
    plan = D.chunk_plan([(s, e, n) for s, e, _f, n in segs])
    emb = np.stack([emb_stub(O.fbank(x[segs[g][2] + f:segs[g][2] + f + n], 1.0)) for _s, _e, g, f, n in plan])
    unit = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    cos = unit @ unit.T
    same = np.equal.outer([who[p[2]] for p in plan], [who[p[2]] for p in plan])
    print(f"end to end: {len(plan)} chunks, within-speaker cosine >= {cos[same].min():.3f}, across <= {cos[~same].max():.3f}")
    assert cos[same].min() > 0.9 and cos[~same].max() < 0.3      # no clustering decision is close
    r64, r32 = NO.nme_sc(emb, max_speakers), NO.nme_sc(emb, max_speakers, solver="f32")
    assert len(plan) == 16 and r64["k"] == 2 and NO.admissible(len(plan), r64, r32) == []
    labels = r64["labels"]
    want = D.speaker_segments([p[0] for p in plan], [p[1] for p in plan], labels, merge_gap)
    assert [w[2] for w in want] == [1, 2] * 4
    assert got == want, (got, want)

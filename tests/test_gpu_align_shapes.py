"""Word alignment at the shapes production runs and against a reference that is not tests/align_oracle.py:

  * HF transformers' own alignment matrix and DTW path (tests/golden/whisper_tiny_align_golden.npz, made by
    tests/golden/make_whisper_align_golden.py) -- probabilities of the library's pass over the same audio and tokens, and
    crispy_asr_dtw_device on HF's matrix giving HF's path exactly;
  * the catalog width d = 768 (dense in precision modes 0 and 1, resident q5_0 blocks);
  * ~220 token rows (the DTW kernel over four waves, the matrix kernel above 64 KB of LDS), the DTW at 226 x 1500;
  * windows shorter than the matrix kernel's tile (n_frames 12 and 30: the reflected halo stays inside the clip's keys);
  * every window of a clip of several windows (seek > 0, a partial last window): token times and words equal the stage
    pass on that window's own encoder output and the oracle's words."""
import os

import numpy as np
import pytest

from tests import align_oracle as AO

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "whisper_tiny_align_golden.npz")


def _rows(hp, n_text, seed):
    from oracle import whisper_oracle as WO
    sp = WO.special_tokens(hp.n_vocab)
    rng = np.random.default_rng(seed)
    return [sp["sot"], sp["lang0"], sp["transcribe"], sp["not_"]] + rng.integers(0, sp["eot"], n_text).tolist() + [sp["eot"]]


def _stage(m, hp, W, precision, n_frames, heads, n_text, tol_p, tol_m, scale=0.02, seed=0):
    """One stage call over two clips against the oracle: probabilities, matrix (bounds given), DTW exact."""
    import torch
    g = torch.Generator().manual_seed(100 + seed)
    enc = torch.randn(2, hp.n_audio_ctx, hp.n_audio_state, generator=g) * scale
    rows = [_rows(hp, n_text, seed + 1), _rows(hp, max(2, n_text // 2), seed + 2)]
    nh = len(heads)
    ld = max(len(r) for r in rows)
    probs = torch.zeros(2, nh, ld, hp.n_audio_ctx, device="cuda")
    mat = torch.zeros(2, ld, hp.n_audio_ctx, device="cuda")
    d_enc = enc.cuda()
    torch.cuda.synchronize()
    nf = list(n_frames)
    jt = m.align_device(d_enc.data_ptr(), rows, 3, nf, heads, probs.data_ptr(), mat.data_ptr(), ld)
    P, Mx = probs.cpu().numpy(), mat.cpu().numpy()
    for b in range(2):
        F, R = nf[b] // 2, len(rows[b])
        p_ref, m_ref = AO.alignment(W, hp, enc[b].numpy().astype(np.float64), rows[b], nf[b], heads, f16=precision == 1)
        dp = np.abs(P[b, :, :R, :F] - p_ref).max()
        dm = np.abs(Mx[b, :R, :F] - m_ref).max()
        print(f"d {hp.n_text_state} mode {precision} rows {R} frames {nf[b]}: probabilities {dp:.2e}, matrix {dm:.2e}")
        assert dp < tol_p and dm < tol_m
        ti, tj = AO.dtw(-Mx[b, 3:R - 1, :F])
        assert np.array_equal(jt[b, :R - 4], (AO.jump_indices(ti, tj)[:R - 4] * 0.02).astype(np.float32))


@pytest.fixture(scope="module")
def tiny():
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams.tiny()
    W = synthetic_whisper_weights(hp, 0, sensitive=True)
    m = WhisperModel(hp, W)
    yield hp, W, m
    m.close()


HEADS = [(2, 2), (3, 0), (3, 2), (3, 3), (3, 4), (3, 5)]


@pytest.mark.parametrize("n_frames", [(12, 30), (30, 35)])
def test_windows_shorter_than_the_matrix_tile(tiny, n_frames):
    hp, W, m = tiny
    m.set_precision(0)
    _stage(m, hp, W, 0, n_frames, HEADS, 9, 1e-5, 5e-5)


def test_220_token_rows(tiny):
    """R = 221: the matrix kernel takes 72 KB of LDS (the attribute path above 64 KB), the DTW 217 rows = four waves."""
    hp, W, m = tiny
    m.set_precision(0)
    _stage(m, hp, W, 0, (3000, 2750), HEADS, 216, 1e-5, 5e-5)


@pytest.mark.parametrize("kind", ["ties", "random"])
def test_dtw_at_226_by_1500(tiny, kind):
    import torch
    _, _, m = tiny
    rng = np.random.default_rng(5)
    n, f = 226, 1500
    x = rng.integers(-1, 2, (n, f)).astype(np.float32) if kind == "ties" else rng.standard_normal((n, f)).astype(np.float32)
    d = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    ti, tj = m.dtw_device(d.data_ptr(), n, f, f)
    ri, rj = AO.dtw(x)
    assert np.array_equal(ti, ri) and np.array_equal(tj, rj)


def test_hf_golden():
    """Mode 0 on the library's own log-mel + encoder of the golden's audio: probabilities within 1e-4 of HF's
    (a sample of every 50th frame), the head-averaged matrix close to HF's; and the DTW kernel on HF's own matrix gives
    HF's path, cell for cell."""
    import torch
    from crispy_amd import synth_audio
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    G = np.load(GOLD)
    heads = [tuple(int(v) for v in h) for h in G["heads"]]
    hp = HParams.tiny()
    m = WhisperModel(hp, synthetic_whisper_weights(hp, 0))
    try:
        m.set_precision(0)
        for ci in range(2):
            seed, n = (int(v) for v in G[f"c{ci}_clip"])
            toks = [int(t) for t in G[f"c{ci}_tokens"]]
            enc = torch.from_numpy(m.encode([synth_audio.clip16k_np(seed, n)])).cuda()
            R = len(toks)
            probs = torch.zeros(1, len(heads), R, hp.n_audio_ctx, device="cuda")
            mat = torch.zeros(1, R, hp.n_audio_ctx, device="cuda")
            torch.cuda.synchronize()
            m.align_device(enc.data_ptr(), [toks], 3, [3000], heads, probs.data_ptr(), mat.data_ptr(), R)
            dp = np.abs(probs.cpu().numpy()[0, :, :, ::50] - G[f"c{ci}_probs"]).max()
            print(f"clip {ci}: probabilities {dp:.2e} (max {G[f'c{ci}_probs'].max():.2e})")
            assert dp < 1e-4
            if ci == 0:
                dm = np.abs(mat.cpu().numpy()[0, 3:R - 1, :1500] - G["c0_matrix"]).max()
                print(f"clip 0: matrix {dm:.2e}")
                assert dm < 5e-2           # z-scores of probabilities ~1/1500 apart: the encoders' 1e-5 differences, x 1/std
                hm = torch.from_numpy(-G["c0_matrix"]).cuda()
                torch.cuda.synchronize()
                ti, tj = m.dtw_device(hm.data_ptr(), hm.shape[0], hm.shape[1], hm.shape[1])
                assert np.array_equal(ti, G["c0_path"][0]) and np.array_equal(tj, G["c0_path"][1])
    finally:
        m.close()


# ---- d = 768 (the catalog's small width): dense in both modes, resident q5_0 ----
SMALL_HEADS = [(6, 1), (9, 4), (11, 11)]


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams.small()
    return hp, synthetic_whisper_weights(hp, 0)


@pytest.mark.parametrize("precision", [0, 1])
def test_d768_dense(small, precision):
    from crispy_amd.asr import WhisperModel
    hp, W = small
    m = WhisperModel(hp, W)
    try:
        m.set_precision(precision)
        # the synthetic d = 768 weights attend almost uniformly (probabilities within 1e-9 of the oracle's, their spread
        # over the rows ~1e-6): the z-scores amplify that, measured 2.5e-4 (mode 0) / 5e-3 (mode 1)
        _stage(m, hp, W, precision, (3000, 1800), SMALL_HEADS, 12, 1e-5 if precision == 0 else 1e-3,
               1e-3 if precision == 0 else 1.5e-2)
    finally:
        m.close()


def test_d768_resident_q5_0(small, tmp_path):
    from crispy_amd.asr import WhisperEngine
    from crispy_amd.ggml_io import synthetic_vocab, write_ggml_quantized
    from crispy_amd.mel_filters import whisper_mel_filters
    hp, W = small
    path = str(tmp_path / "small-q5_0.bin")
    Wq = write_ggml_quantized(path, hp, W, whisper_mel_filters(hp.n_mels), synthetic_vocab(hp.n_vocab), "q5_0")
    eng = WhisperEngine(path, resident=True)
    try:
        eng.set_precision(1)
        _stage(eng, hp, Wq, 1, (3000, 2222), SMALL_HEADS, 12, 1e-3, 1.5e-2)
    finally:
        eng.close()


# ---- every window of a clip of several windows ----
def test_every_window_of_a_long_clip(tmp_path):
    """The scripted engine of tests/test_gpu_align.py, a 30 s clip and a 13 s one: per kept window, the token times are
    seek x 0.01 + the stage pass's jump times on that window's encoder output (the engine's own log-mel window at its
    seek, n_frames = min(3000, seek_end - seek)), and the words those of the oracle."""
    import torch
    from crispy_amd.asr import LogMel, transcribe_batch
    from tests import test_gpu_align as T
    eng, sp = T.make_engine(str(tmp_path))
    try:
        mel = LogMel(80)
        checked = 0
        for x in (T._clips()[2], T._clips()[0]):
            on = transcribe_batch(eng, [x], language_token=sp["lang0"], timestamps=True, with_segments=True, with_words=True,
                                  dtw=True, dtw_heads=T.HEADS)[0]
            tokens, wins, times, words = on[1], on[4], on[5], on[6]
            seek_end = 1 + (x.size + 200 - 400) // 160
            d_pcm = torch.from_numpy(x).cuda()
            mel_t = torch.zeros(3002 * 80 * 2, device="cuda")
            enc = torch.zeros(1, eng.hp.n_audio_ctx, eng.hp.n_audio_state, device="cuda")
            torch.cuda.synchronize()
            mel.compute_device(d_pcm.data_ptr(), x.size, np.array([x.size]), 0, mel_t.data_ptr())
            pos, wi = 0, 0
            for w in wins:
                n = w["n_tokens"]
                seg = tokens[pos:pos + n]
                at = [pos + i for i, t in enumerate(seg) if t < sp["eot"]]
                pos += n
                if not at or w["no_speech"]:
                    continue
                mel.window_device([0], [w["seek"]], 0, mel_t.data_ptr())
                mel.synchronize()
                eng.encode_device(mel_t.data_ptr(), 1, enc.data_ptr())
                eng.synchronize()
                first = [tokens[i] for i in at]
                row = [sp["sot"], sp["lang0"], sp["transcribe"], sp["not_"]] + first + [sp["eot"]]
                jt = eng.align_device(enc.data_ptr(), [row], 3, [min(3000, seek_end - w["seek"])], T.HEADS)[0]
                idx = np.rint(jt[:len(first) + 1] / 0.02).astype(int)
                assert [times[i] for i in at] == [float(AO.token_time(w["seek"], k)) for k in idx[:len(first)]]
                ref = AO.window_words([eng.token_text(t) for t in first], idx, w["seek"])
                got = words[wi:wi + len(ref)]
                wi += len(ref)
                assert [tuple(g) for g in got] == [(float(a), float(b), t, at[f], k) for a, b, t, f, k in ref]
                checked += 1
        assert checked >= 3, checked
        mel.close()
    finally:
        eng.close()

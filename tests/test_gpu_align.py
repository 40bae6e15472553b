"""Word-level timestamps (crispy_asr_opts::dtw_token_timestamps) on the GPU: the stage entry points against the float64
oracle (tests/align_oracle.py), the DTW kernel on tie matrices, and the seek loop with the option on -- same tokens,
text, segments and windows as with it off, a clip's times and words the same alone and in any batch, recording and
host wrappers shifting them by the chunk offset."""
import os

import numpy as np
import pytest

from tests import align_oracle as AO

pytestmark = pytest.mark.gpu

HEADS = [(2, 2), (3, 0), (3, 2), (3, 3), (3, 4), (3, 5)]


@pytest.fixture(scope="module")
def tiny():
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams.tiny()
    W = synthetic_whisper_weights(hp, 0, sensitive=True)
    m = WhisperModel(hp, W)
    yield hp, W, m
    m.close()


def _rows(hp, n_text, seed):
    from oracle import whisper_oracle as WO
    sp = WO.special_tokens(hp.n_vocab)
    rng = np.random.default_rng(seed)
    sot = [sp["sot"], sp["lang0"], sp["transcribe"]]
    return sot + [sp["not_"]] + rng.integers(0, sp["eot"], n_text).tolist() + [sp["eot"]]


# bounds: probabilities 1e-5 (mode 0) / 1e-3 (mode 1: f32 q against the f16 cross K, the oracle's q in float64); the
# matrix is a z-score over the rows of probabilities near 1 / F, so an absolute error of the probabilities is amplified
# by 1 / std -- bounded here at 5e-5 (mode 0; measured 2.4e-6) and 1.5e-2 (mode 1; measured 3.7e-3)
@pytest.mark.parametrize("precision,n_frames,heads", [(0, 3000, HEADS), (1, 3000, HEADS), (0, 1234, None), (1, 2001, [(1, 5), (3, 1)])])
def test_stage_entry_point_matches_the_oracle(tiny, precision, n_frames, heads):
    import torch
    hp, W, m = tiny
    m.set_precision(precision)
    g = torch.Generator().manual_seed(7 + n_frames)
    # encoder outputs scaled so that the scores stay within about +-7, as a trained model's alignment heads do (at +-170 the
    # probabilities underflow in f32, and the z-scores of openai's f32 recipe with them)
    enc = torch.randn(2, hp.n_audio_ctx, hp.n_audio_state, generator=g) * 0.02
    d_enc = enc.to("cuda")
    rows = [_rows(hp, 17, 1), _rows(hp, 9, 2)]
    nh = len(heads) if heads else (hp.n_text_layer - hp.n_text_layer // 2) * hp.n_text_head
    ld = max(len(r) for r in rows)
    probs = torch.zeros(2, nh, ld, hp.n_audio_ctx, device="cuda")
    mat = torch.zeros(2, ld, hp.n_audio_ctx, device="cuda")
    nf = [n_frames, min(n_frames, 2400)]
    torch.cuda.synchronize()
    jt = m.align_device(d_enc.data_ptr(), rows, 3, nf, heads, probs.data_ptr(), mat.data_ptr(), ld)
    P, Mx = probs.cpu().numpy(), mat.cpu().numpy()
    for b in range(2):
        F, R = nf[b] // 2, len(rows[b])
        p_ref, m_ref = AO.alignment(W, hp, enc[b].numpy().astype(np.float64), rows[b], nf[b], heads, f16=precision == 1)
        dp = np.abs(P[b, :, :R, :F] - p_ref).max()
        dm = np.abs(Mx[b, :R, :F] - m_ref).max()
        print(f"mode {precision} clip {b}: probabilities {dp:.2e}, matrix {dm:.2e}")
        assert dp < (1e-5 if precision == 0 else 1e-3)
        assert dm < (5e-5 if precision == 0 else 1.5e-2)
        # the DTW: exactly the oracle's on the library's own matrix
        ti, tj = AO.dtw(-Mx[b, 3:R - 1, :F])
        want = (AO.jump_indices(ti, tj)[:R - 4] * 0.02).astype(np.float32)
        assert np.array_equal(jt[b, :R - 4], want)
    m.set_precision(0)


@pytest.mark.parametrize("kind", ["zeros", "constant_rows", "stripes", "random", "ints"])
def test_dtw_kernel_equals_the_oracle_on_ties(tiny, kind):
    import torch
    _, _, m = tiny
    rng = np.random.default_rng(3)
    n, f = 37, 301
    if kind == "zeros":
        x = np.zeros((n, f), np.float32)
    elif kind == "constant_rows":
        x = np.repeat(rng.integers(0, 3, n).astype(np.float32)[:, None], f, 1)
    elif kind == "stripes":
        x = (np.indices((n, f)).sum(0) % 3).astype(np.float32)
    elif kind == "ints":
        x = rng.integers(-2, 3, (n, f)).astype(np.float32)
    else:
        x = rng.standard_normal((n, f)).astype(np.float32)
    ld = f + 3
    d = torch.zeros(n, ld, device="cuda")
    d[:, :f] = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    ti, tj = m.dtw_device(d.data_ptr(), n, f, ld)
    ri, rj = AO.dtw(x)
    assert np.array_equal(ti, ri) and np.array_equal(tj, rj)


# ---- the seek loop with the option on (a scripted model: predictable windows, several per clip, prompts with past text) ----
@pytest.fixture(scope="module")
def engine(tmp_path_factory):
    eng, sp = make_engine(str(tmp_path_factory.mktemp("ggml_align")))
    yield eng, sp
    eng.close()


def make_engine(tmpdir):
    from crispy_amd.asr import WhisperEngine
    from crispy_amd.ggml_io import synthetic_vocab, write_ggml
    from crispy_amd.mel_filters import whisper_mel_filters
    from crispy_amd.whisper_weights import HParams
    from oracle import whisper_oracle as WO
    from tests.scripted_model import script_rows, scripted_whisper_weights
    hp = HParams.tiny()
    sp = WO.special_tokens(hp.n_vocab)
    BEG, EOT = sp["beg"], sp["eot"]
    rows = script_rows(2, [BEG, 1001, 1002, 1003, 1004, 1005, BEG + 300, BEG + 300, 1006, 1007, 1002, EOT])
    W = scripted_whisper_weights(hp, rows, gain=100.0)
    vocab = synthetic_vocab(hp.n_vocab)
    vocab[1002] = b","                              # punctuation: merged into the word in front of it
    vocab[1003] = b"ab"                             # no leading space: continues the word in front of it
    vocab[1004] = b" \xe2\x82"                      # a character split across two tokens
    vocab[1005] = b"\xac"
    path = os.path.join(tmpdir, "tiny-align.bin")
    write_ggml(path, hp, W, whisper_mel_filters(80), vocab, f16=False)
    eng = WhisperEngine(path)
    eng.set_precision(1)
    return eng, sp


def _clips():
    from crispy_amd import synth_audio
    base = synth_audio.clip16k_np(80, 16000 * 30)
    return [base[:16000 * n] for n in (13, 7, 30, 3)]


def test_option_changes_nothing_else_and_clips_align_as_alone(engine):
    from crispy_amd.asr import transcribe_batch
    eng, sp = engine
    clips = _clips()
    kw = dict(language_token=sp["lang0"], timestamps=True, with_segments=True)
    off = transcribe_batch(eng, clips, **kw)
    on = transcribe_batch(eng, clips, dtw=True, with_words=True, dtw_heads=HEADS, **kw)
    for c in range(len(clips)):
        assert on[c][:5] == off[c]                                   # tokens, text, language, segments, windows
        tokens, times, words = on[c][1], on[c][5], on[c][6]
        assert times is not None and len(times) == len(tokens)
        assert all((t < 0) == (tok >= sp["eot"]) for tok, t in zip(tokens, times))
        assert words and all(w[0] <= w[1] for w in words)
        assert on[c] == transcribe_batch(eng, [clips[c]], dtw=True, with_words=True, dtw_heads=HEADS, **kw)[0]
    assert any(len(o[4]) > 1 for o in on)                            # several windows: the second one with past text
    # 70 clips of mixed lengths: every clip's result is its solo result, bit for bit
    many = [clips[i % 4][: 16000 * (3 + (i * 7) % 27)] for i in range(70)]
    big = transcribe_batch(eng, many, dtw=True, with_words=True, dtw_heads=HEADS, **kw)
    for c in (0, 1, 2, 3, 33, 69):
        solo = transcribe_batch(eng, [many[c]], dtw=True, with_words=True, dtw_heads=HEADS, **kw)[0]
        assert big[c] == solo, c
    # default heads run too
    dflt = transcribe_batch(eng, clips[:2], dtw=True, with_words=True, **kw)
    assert [d[:5] for d in dflt] == off[:2]


def test_first_window_times_and_words_equal_the_stage_pass_and_the_oracle(engine):
    """The first window of each clip (seek 0): token times are the stage entry point's jump times on the same tokens and
    encoder output; the words are what the oracle splits and merges from those times."""
    import torch
    from crispy_amd.asr import transcribe_batch
    eng, sp = engine
    clips = _clips()
    kw = dict(language_token=sp["lang0"], timestamps=True, with_segments=True)
    on = transcribe_batch(eng, clips, dtw=True, with_words=True, dtw_heads=HEADS, **kw)
    enc = torch.from_numpy(eng.encode(clips)).cuda()
    torch.cuda.synchronize()
    for c, x in enumerate(clips):
        tokens, wins, times, words = on[c][1], on[c][4], on[c][5], on[c][6]
        n0 = wins[0]["n_tokens"]
        first = [t for t in tokens[:n0] if t < sp["eot"]]
        at = [i for i, t in enumerate(tokens[:n0]) if t < sp["eot"]]
        seek_end = 1 + (x.size + 200 - 400) // 160
        row = [sp["sot"], sp["lang0"], sp["transcribe"], sp["not_"]] + first + [sp["eot"]]
        jt = eng.align_device(enc[c:c + 1].data_ptr(), [row], 3, [min(3000, seek_end)], HEADS)[0]
        assert [times[i] for i in at] == [float(v) for v in jt[:len(first)]]
        idx = np.rint(jt[:len(first) + 1] / 0.02).astype(int)
        ref = AO.window_words([eng.token_text(t) for t in first], idx, 0)
        got = words[:len(ref)]
        assert [(w[0], w[1], w[2], w[3], w[4]) for w in got] == [(float(a), float(b), t, at[f], n) for a, b, t, f, n in ref]
    assert any("," in w[2] and "ab" in w[2] for w in on[0][6]), on[0][6]       # the merge and the continuation happened


def test_recording_and_host_wrapper_shift_words_by_the_chunk_offset(engine):
    from crispy_amd.asr import transcribe_batch, transcribe_recording, transcribe_with_timestamps
    eng, sp = engine
    clips = _clips()
    rec = np.concatenate([clips[2], clips[0]])                      # two chunks: 30 s + 13 s
    full = transcribe_recording(eng, rec, timestamps=True, with_result=True, with_words=True, dtw=True, dtw_heads=HEADS)
    per = transcribe_batch(eng, [clips[2], clips[0]], timestamps=True, with_segments=True, with_words=True, dtw=True,
                           dtw_heads=HEADS)
    n0 = len(per[0][1])
    off = np.float32(30.0)
    want_words = per[0][6] + [(off + np.float32(a), off + np.float32(b), t, n0 + f, n) for a, b, t, f, n in per[1][6]]
    assert [(float(a), float(b), t, f, n) for a, b, t, f, n in full[6]] == [(float(a), float(b), t, f, n) for a, b, t, f, n in want_words]
    want_t = per[0][5] + [t if t < 0 else float(off + np.float32(t)) for t in per[1][5]]
    assert full[5] == want_t
    got = transcribe_with_timestamps(eng, clips[0], 60.0, words=True, dtw_heads=HEADS)
    assert got and got == [(60.0 + a, 60.0 + b, t) for a, b, t, _f, _n in eng.last_words]
    assert [w[2] for w in eng.last_words] == [w[2] for w in per[1][6]]

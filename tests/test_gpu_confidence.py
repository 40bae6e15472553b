"""Confidence on the GPU (crispy_asr_set_confidence and its accessors): the stage entry points against the float64 oracle
(tests/confidence_oracle.py) in precision modes 0 and 1, on a scripted model whose probabilities underflow, across prompt-step
layouts and batch compositions, at width 768 (dense, resident q5_0); the language distribution for the three vocabulary
layouts; and the seek loop with the switch on -- everything else unchanged, p_forced equal to the stage pass, word means,
plog the addends of avg_logprob for greedy / temperature-ladder / beam winners, batch and recording merges.

The bound on a log-probability is 2 x the bar the project holds for a decoder logit in the mode: a log-probability is a logit
minus a log-sum-exp, and each of the two moves by at most the largest logit error.  Mode 0: 2.5e-4 of the logit scale
(tests/test_gpu_pipeline.py: forced_picks(..., rel=2.5e-4)); mode 1: 5e-4 of it at the worst value
(tests/test_gpu_whisper.py::test_mode_1_decoder_matches_the_f16_arithmetic_oracle).  Scale = the largest |logit| of the row
among the ids the soft-max runs over."""
import dataclasses
import os

import numpy as np
import pytest

from tests import confidence_oracle as CO

pytestmark = pytest.mark.gpu

LOGIT_REL = {0: 2.5e-4, 1: 5e-4}
HEADS = [(2, 2), (3, 0), (3, 2), (3, 3), (3, 4), (3, 5)]


def _sp(hp):
    from oracle import whisper_oracle as WO
    return WO.special_tokens(hp.n_vocab)


def _p32(logp):
    """A probability as the library publishes it: the exponential in double, rounded once to f32."""
    return np.exp(np.asarray(logp, np.float32).astype(np.float64)).astype(np.float32)


def _check(got, ref, ref_logits, eot, mode, what):
    """got f32 / ref f64 log-probabilities of one clip, ref_logits the oracle's rows; returns the largest error in bars."""
    n = len(ref)
    bar = np.array([2 * LOGIT_REL[mode] * np.abs(ref_logits[i][:eot]).max() for i in range(n)])
    err = np.abs(np.asarray(got[:n], np.float64) - ref)
    print(f"{what}: |d log p| / bound per token: {np.round(err / bar, 3).tolist()}")
    assert np.isfinite(got[:n]).all(), (what, got[:n])
    assert (err <= bar).all(), (what, int(np.argmax(err / bar)), err.max(), bar.tolist())
    return float((err / bar).max())


# ---- the stage entry against the oracle, targets and maxima on the edges of the cropped row ----
@pytest.fixture(scope="module")
def tiny():
    """Random-init Whisper-tiny with two embedding rows moved so that the reduction's edges are hit: the row of
    <|notimestamps|> has its maximum below <|endoftext|> in the LAST column of the crop (id eot - 1), the row behind it has its
    largest logit of all at a special (<|startoflm|>, an id >= eot), which must not enter the sum.  Clip 0's text holds id 0
    and -- last, so that no earlier row sees its moved embedding -- id eot - 1.
    The encoder outputs are scaled as tests/test_gpu_align.py scales them (x 0.02: the score range of a trained model).  At
    x 0.5 the sharpened cross-attention of these weights is ill-conditioned -- the f16-operand oracle and the exact one are
    2.6e-2 of the logit scale apart on single tokens (3.5e-1 at x 0.8), one f16 rounding moved by the order of accumulation
    changes a log-probability by several bounds, and no implementation of the mode could meet its own oracle there."""
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    from oracle import whisper_oracle as WO
    from tests.test_gpu_align import _rows
    hp = HParams.tiny()
    sp = _sp(hp)
    eot = sp["eot"]
    W = synthetic_whisper_weights(hp, 0, sensitive=True)
    rng = np.random.default_rng(21)
    enc = (rng.standard_normal((2, hp.n_audio_ctx, hp.n_audio_state)) * 0.02).astype(np.float32)
    rows = [_rows(hp, 17, 1), _rows(hp, 9, 2)]
    rows[0][4 + 5] = 0
    rows[0][4 + 16] = eot - 1
    rows[1][4 + 3] = 0
    dc = WO.DecoderCache(W, hp, enc[0].astype(np.float64))
    for t in rows[0][:3]:
        dc.step(t)
    t_a = int(np.argmax(dc.step(rows[0][3])[:eot]))          # the <|notimestamps|> row
    t_b = int(np.argmax(dc.step(rows[0][4])[:eot]))          # the row of the first text token
    E = W["decoder.token_embedding.weight"].copy()
    E[eot - 1] = 2 * E[t_a]
    E[sp["solm"]] = 3 * E[t_b]
    W["decoder.token_embedding.weight"] = E
    m = WhisperModel(hp, W)
    ref = {}
    for mode in (0, 1):
        ref[mode] = [CO.token_logprobs(W, hp, enc[b], rows[b], 3, f16=mode == 1, with_logits=True) for b in range(2)]
    yield hp, W, m, rows, enc, ref
    m.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_stage_entry_matches_the_oracle_on_the_edges_of_the_crop(tiny, mode):
    import torch
    hp, W, m, rows, enc, ref = tiny
    sp = _sp(hp)
    eot = sp["eot"]
    lp0, lg0 = ref[mode][0]
    # the fixture did what it says, in this mode's oracle
    assert int(np.argmax(lg0[0][:eot])) == eot - 1                                  # maximum in the last column of the crop
    assert int(np.argmax(lg0[1])) == sp["solm"] and sp["solm"] >= eot               # the row's largest logit is outside it
    bar1 = 2 * LOGIT_REL[mode] * np.abs(lg0[1][:eot]).max()
    wrong = CO.log_softmax_at(lg0[1], hp.n_vocab, rows[0][5])                       # ... had the special entered the sum
    assert abs(wrong - lp0[1]) > 100 * bar1, (wrong, lp0[1], bar1)
    assert rows[0][4 + 5] == 0 and rows[0][4 + 16] == eot - 1 and rows[1][4 + 3] == 0
    d_enc = torch.from_numpy(enc).cuda()
    torch.cuda.synchronize()
    m.set_precision(mode)
    try:
        got = m.token_probs_device(d_enc.data_ptr(), rows, 3)
    finally:
        m.set_precision(0)
    for b in range(2):
        n = len(rows[b]) - 5
        lp, lg = ref[mode][b]
        assert lp.shape == (n,) and np.isnan(got[b, n:]).all()
        worst = _check(got[b], lp, lg, eot, mode, f"mode {mode} clip {b}")
        print(f"mode {mode} clip {b}: max |d log p| {np.abs(got[b, :n] - lp).max():.2e} = {worst:.3f} of the bound; "
              f"log p {lp.min():.2f} .. {lp.max():.2f}")


# ---- probabilities that underflow: a scripted model at gain 100 ----
@pytest.mark.parametrize("mode", [0, 1])
def test_scripted_model_gain_100_has_finite_logs_where_p_underflows(mode):
    import torch
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import HParams
    from tests.scripted_model import script_rows, scripted_whisper_weights
    hp = HParams.tiny()
    sp = _sp(hp)
    script = [1001, 1002, 1003, 1004, 1005, 1006]
    W = scripted_whisper_weights(hp, script_rows(3, script), gain=100.0)     # row 3 = <|notimestamps|> predicts the first text token
    text = [1001, 2001, 1003, 2002, 1005, 1006]
    row = [sp["sot"], sp["lang0"], sp["transcribe"], sp["not_"]] + text + [sp["eot"]]
    rng = np.random.default_rng(3)
    enc = (rng.standard_normal((1, hp.n_audio_ctx, hp.n_audio_state)) * 0.5).astype(np.float32)
    lp, lg = CO.token_logprobs(W, hp, enc[0], row, 3, f16=mode == 1, with_logits=True)
    m = WhisperModel(hp, W)
    try:
        m.set_precision(mode)
        d_enc = torch.from_numpy(enc).cuda()
        torch.cuda.synchronize()
        got = m.token_probs_device(d_enc.data_ptr(), [row], 3)[0, :len(text)]
    finally:
        m.close()
    worst = _check(got, lp, lg, sp["eot"], mode, f"scripted mode {mode}")
    print(f"scripted mode {mode}: log p {got.tolist()} ({worst:.3f} of the bound)")
    for i, (t, s) in enumerate(zip(text, script)):
        bar = 2 * LOGIT_REL[mode] * np.abs(lg[i][:sp["eot"]]).max()
        if t == s:
            assert abs(got[i]) <= bar, (i, got[i], bar)                  # the scripted token: log p within the bar of 0
        else:
            assert np.isfinite(got[i]) and got[i] < -100.0, (i, got[i])   # everything else: far below, and finite
    p = _p32(got)
    assert not np.isnan(p).any()
    assert all(v == 0.0 or v < np.finfo(np.float32).tiny for v, t, s in zip(p, text, script) if t != s), p


# ---- row layout: prompt steps of several P, the sequential prefill, left padding ----
@pytest.mark.parametrize("mode", [0, 1])
def test_a_rows_bits_do_not_depend_on_the_prompt_steps_or_the_batch(tiny, mode):
    import torch
    from tests.test_gpu_align import _rows
    hp, W, m, _, enc, _ = tiny
    mid = _rows(hp, 220, 11)                                   # 225 rows: alone one step of P = 225; of three clips P = 170, then 55
    rows3 = [_rows(hp, 57, 12), mid, _rows(hp, 131, 13)]
    g = np.random.default_rng(8)
    e3 = (g.standard_normal((3, hp.n_audio_ctx, hp.n_audio_state)) * 0.5).astype(np.float32)
    d3 = torch.from_numpy(e3).cuda()
    d1 = d3[1:2].contiguous()
    torch.cuda.synchronize()
    m.set_precision(mode)
    old = os.environ.pop("CRISPY_ASR_PREFILL", None)
    try:
        alone = m.token_probs_device(d1.data_ptr(), [mid], 3)[0]
        three = m.token_probs_device(d3.data_ptr(), rows3, 3)
        os.environ["CRISPY_ASR_PREFILL"] = "seq"
        seq = m.token_probs_device(d1.data_ptr(), [mid], 3)[0]
        seq3 = m.token_probs_device(d3.data_ptr(), rows3, 3)
    finally:
        os.environ.pop("CRISPY_ASR_PREFILL", None)
        if old is not None:
            os.environ["CRISPY_ASR_PREFILL"] = old
        m.set_precision(0)
    assert np.isfinite(alone[:220]).all() and np.isnan(alone[220:]).all() and len(set(alone[:220].tolist())) > 200
    assert np.array_equal(alone[:220], seq[:220])
    assert np.array_equal(alone[:220], three[1, :220])
    assert np.array_equal(three, seq3, equal_nan=True)
    assert np.isfinite(three[0, :57]).all() and np.isnan(three[0, 57:]).all() and np.isfinite(three[2, :131]).all()


# ---- width 768: dense in mode 1, resident q5_0 == the same file inflated ----
@pytest.fixture(scope="module")
def small():
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    from tests.test_gpu_align_shapes import _rows
    hp = HParams.small()
    rng = np.random.default_rng(31)
    enc = (rng.standard_normal((1, hp.n_audio_ctx, hp.n_audio_state)) * 0.5).astype(np.float32)
    return hp, synthetic_whisper_weights(hp, 0), _rows(hp, 12, 1), enc


def test_d768_dense_mode_1(small):
    import torch
    from crispy_amd.asr import WhisperModel
    hp, W, row, enc = small
    lp, lg = CO.token_logprobs(W, hp, enc[0], row, 3, f16=True, with_logits=True)
    m = WhisperModel(hp, W)
    try:
        m.set_precision(1)
        d_enc = torch.from_numpy(enc).cuda()
        torch.cuda.synchronize()
        got = m.token_probs_device(d_enc.data_ptr(), [row], 3)[0]
    finally:
        m.close()
    worst = _check(got, lp, lg, _sp(hp)["eot"], 1, "d768 dense")
    print(f"d 768 dense mode 1: max |d log p| {np.abs(got[:len(lp)] - lp).max():.2e} = {worst:.3f} of the bound")


def test_d768_resident_q5_0_equals_the_inflated_engine(small, tmp_path):
    import torch
    from crispy_amd.asr import WhisperEngine
    from crispy_amd.ggml_io import synthetic_vocab, write_ggml_quantized
    from crispy_amd.mel_filters import whisper_mel_filters
    hp, W, row, enc = small
    path = str(tmp_path / "small-q5_0.bin")
    Wq = write_ggml_quantized(path, hp, W, whisper_mel_filters(hp.n_mels), synthetic_vocab(hp.n_vocab), "q5_0")
    lp, lg = CO.token_logprobs(Wq, hp, enc[0], row, 3, f16=True, with_logits=True)
    d_enc = torch.from_numpy(enc).cuda()
    torch.cuda.synchronize()
    got = []
    for resident in (True, False):
        eng = WhisperEngine(path, resident=resident)
        try:
            eng.set_precision(1)
            got.append(eng.token_probs_device(d_enc.data_ptr(), [row], 3)[0])
        finally:
            eng.close()
    assert np.array_equal(got[0], got[1], equal_nan=True)
    worst = _check(got[0], lp, lg, _sp(hp)["eot"], 1, "d768 resident q5_0")
    print(f"d 768 resident q5_0: max |d log p| {np.abs(got[0][:len(lp)] - lp).max():.2e} = {worst:.3f} of the bound")


# ---- the language distribution ----
@pytest.mark.parametrize("n_vocab,mode", [(51865, 0), (51865, 1), (51866, 1), (51864, 0)])
def test_language_distribution(n_vocab, mode):
    import torch
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    from oracle import whisper_oracle as WO
    hp = dataclasses.replace(HParams.tiny(), n_vocab=n_vocab)
    sp = _sp(hp)
    W = synthetic_whisper_weights(hp, 0, sensitive=True)
    rng = np.random.default_rng(n_vocab)
    enc = (rng.standard_normal((3, hp.n_audio_ctx, hp.n_audio_state)) * 0.5).astype(np.float32)
    m = WhisperModel(hp, W)
    try:
        m.set_precision(mode)
        d_enc = torch.from_numpy(enc).cuda()
        torch.cuda.synchronize()
        tok, pr = m.detect_language_probs_device(d_enc.data_ptr(), 3)
        if n_vocab == 51864:                                   # English-only: nothing to weigh, and that is not an error
            assert pr.shape == (3, 0) and tok.tolist() == [0, 0, 0]
            return
        n_lang = n_vocab - 51865 + 99
        assert pr.shape == (3, n_lang) and np.isfinite(pr).all()
        assert np.array_equal(tok, m.detect_language_device(d_enc.data_ptr(), 3))
        assert np.array_equal(tok, sp["lang0"] + pr.argmax(-1))
        for b in range(3):
            assert abs(float(pr[b].astype(np.float64).sum()) - 1.0) <= 1e-6         # 100 addends of f32
            lg = WO.DecoderCache(W, hp, enc[b].astype(np.float64), f16=mode == 1).step(sp["sot"])
            ref = CO.lang_probs(lg, n_vocab)
            # a probability moves by at most p x (its logit's error + the log-sum-exp's): the log-probability bound, times p <= 1
            bar = 2 * LOGIT_REL[mode] * np.abs(lg[sp["lang0"]:sp["lang0"] + n_lang]).max()
            err = np.abs(pr[b] - ref).max()
            print(f"vocab {n_vocab} mode {mode} clip {b}: max |dp| {err:.2e} (bound {bar:.2e}), top {ref.max():.3f}")
            assert err <= bar, (b, err, bar)
    finally:
        m.close()


# ---- the seek loop ----
@pytest.fixture(scope="module")
def engine(tmp_path_factory):
    from tests.test_gpu_align import make_engine
    eng, sp = make_engine(str(tmp_path_factory.mktemp("ggml_conf")))
    yield eng, sp
    eng.close()


def _clips():
    from tests.test_gpu_align import _clips as clips
    return clips()


def _same_but_confidence(a, b):
    """Two results of transcribe_batch(with_segments, with_words): text, tokens, language, segments, windows[] (floats compared
    as arrays), token times, words."""
    assert a[0] == b[0] and a[2] == b[2]
    assert np.array_equal(np.array(a[1]), np.array(b[1]))
    assert [s[2] for s in a[3]] == [s[2] for s in b[3]]
    assert np.array_equal(np.array([s[:2] for s in a[3]], np.float32), np.array([s[:2] for s in b[3]], np.float32))
    assert len(a[4]) == len(b[4])
    for wa, wb in zip(a[4], b[4]):
        assert list(wa) == list(wb)
        assert np.array_equal(np.array([wa[k] for k in wa], np.float64), np.array([wb[k] for k in wb], np.float64), equal_nan=True)
    assert np.array_equal(np.array(a[5], np.float32), np.array(b[5], np.float32))
    assert [w[2:] for w in a[6]] == [w[2:] for w in b[6]]
    assert np.array_equal(np.array([w[:2] for w in a[6]], np.float32), np.array([w[:2] for w in b[6]], np.float32))


def _conf_equal(a, b):
    for k in ("plog", "p_forced", "word_probs", "lang_probs"):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert a[k].dtype == np.float32 and np.array_equal(a[k], b[k]), k


def test_switch_changes_nothing_else_and_the_numbers_are_the_stage_pass(engine):
    import torch
    from crispy_amd.asr import transcribe_batch
    eng, sp = engine
    clips = _clips()[:3]
    kw = dict(language_token=sp["lang0"], timestamps=True, with_segments=True, with_words=True, dtw=True, dtw_heads=HEADS,
              with_confidence=True)
    eng.set_confidence(False)
    off = transcribe_batch(eng, clips, **kw)
    eng.set_confidence(True)
    try:
        on = transcribe_batch(eng, clips, **kw)
        solo = [transcribe_batch(eng, [c], **kw)[0] for c in clips]
    finally:
        eng.set_confidence(False)
    enc = torch.from_numpy(eng.encode(clips)).cuda()
    torch.cuda.synchronize()
    for c in range(len(clips)):
        _same_but_confidence(on[c], off[c])
        _same_but_confidence(on[c], solo[c])
        _conf_equal(on[c][7], solo[c][7])                         # one clip alone == the middle / an end of three
        tokens, wins, words, cf = on[c][1], on[c][4], on[c][6], on[c][7]
        # switch off: plog is there (timestamp mode), the gated arrays are not; the language was given
        assert off[c][7]["p_forced"] is None and off[c][7]["word_probs"] is None and off[c][7]["lang_probs"] is None
        assert np.array_equal(off[c][7]["plog"], cf["plog"]) and cf["lang_probs"] is None
        assert cf["n"] == len(tokens) == len(cf["plog"]) == len(cf["p_forced"]) and cf["n_words"] == len(words) == len(cf["word_probs"])
        assert all((p == -1.0) == (t >= sp["eot"]) for t, p in zip(tokens, cf["p_forced"]))
        assert np.isfinite(cf["p_forced"]).all() and np.isfinite(cf["word_probs"]).all()
        # the first window: p_forced = exp of the stage entry on that window's rows
        n0 = wins[0]["n_tokens"]
        at = [i for i, t in enumerate(tokens[:n0]) if t < sp["eot"]]
        first = [tokens[i] for i in at]
        row = [sp["sot"], sp["lang0"], sp["transcribe"], sp["not_"]] + first + [sp["eot"]]
        lp = eng.token_probs_device(enc[c:c + 1].data_ptr(), [row], 3)[0, :len(first)]
        assert np.isfinite(lp).all()
        assert np.array_equal(cf["p_forced"][at], _p32(lp))
        print(f"clip {c}: p_forced of the first window {cf['p_forced'][at].tolist()}, word probabilities {cf['word_probs'].tolist()}")
        # word probabilities: the oracle's means on the library's own p_forced, exactly
        ref = CO.word_probs([eng.token_text(t) for t in first], cf["p_forced"][at])
        assert [w[2] for w in words[:len(ref)]] == [w[0] for w in ref]
        assert np.array_equal(cf["word_probs"][:len(ref)], np.array([w[3] for w in ref], np.float32))


def test_a_published_p_forced_that_underflows_is_zero_or_denormal_not_nan(tmp_path_factory):
    """A script with a timestamp pair in the middle of a window's text: "<|0.00|> a <|2.00|><|2.00|> b c d <|6.00|><|6.00|>".
    The alignment pass drops the pair, so `c` and `d` sit two positions earlier than where the script says them: the row of `a`
    points at a timestamp (outside the crop: `b` competes with the crowd only), so does the row of `b`, and the row of `c`
    points at `b` -- at gain 100 `d` has a log-probability near -384 there, and its published probability underflows."""
    from crispy_amd import synth_audio
    from crispy_amd.asr import WhisperEngine, transcribe_batch
    from crispy_amd.whisper_weights import HParams
    from tests.scripted_model import script_rows, scripted_whisper_weights
    from tests.test_gpu_decision import _engine_file
    hp = HParams.tiny()
    sp = _sp(hp)
    BEG, EOT = sp["beg"], sp["eot"]
    script = [BEG, 1001, BEG + 100, BEG + 100, 1002, 1003, 1004, BEG + 300, BEG + 300, EOT]
    W = scripted_whisper_weights(hp, script_rows(2, script), gain=100.0)
    eng = WhisperEngine(_engine_file(tmp_path_factory, hp, W, "conf-underflow"))
    try:
        eng.set_precision(1)
        eng.set_confidence(True)
        x = synth_audio.clip16k_np(80, 16000 * 7)
        r = transcribe_batch(eng, [x], language_token=sp["lang0"], timestamps=True, with_segments=True, with_words=True, dtw=True,
                             dtw_heads=HEADS, with_confidence=True)[0]
    finally:
        eng.close()
    tokens, wins, cf = r[1], r[4], r[7]
    n0 = wins[0]["n_tokens"]
    assert tokens[:n0] == script[:-1], (tokens, wins)
    pf = cf["p_forced"][:n0]
    print(f"p_forced of the window: {pf.tolist()}; word probabilities {cf['word_probs'].tolist()}")
    assert not np.isnan(cf["p_forced"]).any() and not np.isnan(cf["word_probs"]).any()
    assert pf[[0, 2, 3, 7, 8]].tolist() == [-1.0] * 5                      # the timestamp tokens
    assert abs(float(pf[1]) - 1.0) < 1e-3                                  # `a`: the scripted token of its row
    assert 0.0 <= float(pf[6]) < np.finfo(np.float32).tiny                 # `d`: underflow -- 0 or a denormal
    assert 0.0 <= float(pf[4]) < 1e-3 and 0.0 <= float(pf[5]) < 1e-3       # `b`, `c`: one of the crowd each


def _plog_is_avg_logprob(tokens, wins, plog, eot, what):
    """Every window whose kept tokens are all in `tokens` (no <|endoftext|> among them) and were ranked: float(sum of plog in
    double / count) == avg_logprob, exactly.  Returns (windows checked, windows left out)."""
    assert len(tokens) == len(plog), what
    # A window that ends on <|endoftext|> before any timestamp above <|0.00|> keeps that <|endoftext|> (result_len counts it,
    # `tokens` never holds it): it takes the whole rest of the audio, so it is the clip's last window with tokens -- the one
    # window whose kept tokens are fewer than result_len, left out below.
    extra = sum(w["n_tokens"] for w in wins) - len(tokens)
    assert extra in (0, 1), (what, extra)
    last = max((i for i, w in enumerate(wins) if w["n_tokens"] > 0), default=-1)
    pos, done, skipped = 0, 0, 0
    for i, w in enumerate(wins):
        n = w["n_tokens"] - (1 if extra and i == last else 0)
        seg = plog[pos:pos + n]
        pos += n
        if n == 0 or not np.isfinite(w["avg_logprob"]) or (extra and i == last):      # dropped as silence / never ranked / see above
            skipped += 1
            continue
        s = 0.0
        for v in seg:
            s += float(v)
        assert np.float32(s / n) == np.float32(w["avg_logprob"]), (what, w, seg.tolist())
        done += 1
    assert pos == len(tokens), what
    return done, skipped


def test_plog_are_the_addends_of_avg_logprob_greedy_ladder_and_beam(engine, tmp_path_factory):
    from crispy_amd import synth_audio
    from crispy_amd.asr import WhisperEngine, transcribe_batch
    from crispy_amd.whisper_weights import HParams
    from tests import oracle_cases as OC
    from tests.test_gpu_decision import _engine_file
    eng, sp = engine
    kw = dict(language_token=sp["lang0"], timestamps=True, with_segments=True, with_confidence=True)
    left_out = 0
    for c, r in enumerate(transcribe_batch(eng, _clips(), **kw)):      # greedy, several windows per clip
        done, skipped = _plog_is_avg_logprob(r[1], r[4], r[5]["plog"], sp["eot"], f"greedy clip {c}")
        assert done >= 1 or len(r[4]) == 1, (c, r[4])
        left_out += skipped
    hp = HParams.tiny()
    lad = WhisperEngine(_engine_file(tmp_path_factory, hp, OC.ladder_model(hp), "conf-ladder"))
    try:
        x = synth_audio.clip16k_np(80, 16000 * 13)
        for name, extra in (("ladder", {}), ("beam", dict(beam_size=3))):
            for mode in (0, 1):
                lad.set_precision(mode)
                r = transcribe_batch(lad, [x[:16000 * 7], x], **kw, **extra)[1]
                assert any(w["temperature"] > 0 for w in r[4]), name      # a window accepted above temperature 0
                done, skipped = _plog_is_avg_logprob(r[1], r[4], r[5]["plog"], sp["eot"], f"{name} mode {mode}")
                assert done == len(r[4]) - skipped and done >= 2
                left_out += skipped
    finally:
        lad.close()
    print(f"plog == avg_logprob addends: {left_out} windows left out (not ranked, dropped, or keeping an <|endoftext|>)")


def test_recording_concatenates_and_keeps_the_first_chunks_language(engine):
    from crispy_amd.asr import transcribe_batch, transcribe_recording
    eng, sp = engine
    clips = _clips()
    rec = np.concatenate([clips[2], clips[0]])                      # two chunks: 30 s + 13 s
    kw = dict(timestamps=True, with_words=True, dtw=True, dtw_heads=HEADS, with_confidence=True)
    eng.set_confidence(True)
    try:
        full = transcribe_recording(eng, rec, with_result=True, **kw)
        per = transcribe_batch(eng, [clips[2], clips[0]], with_segments=True, **kw)
    finally:
        eng.set_confidence(False)
    cf = full[7]
    for k in ("plog", "p_forced", "word_probs"):
        assert np.array_equal(cf[k], np.concatenate([per[0][7][k], per[1][7][k]])), k
    assert cf["n"] == len(full[1]) == len(per[0][1]) + len(per[1][1]) and cf["n_words"] == len(full[6])
    n_lang = sp["n_lang"]
    assert cf["lang_probs"].shape == (n_lang,) and np.array_equal(cf["lang_probs"], per[0][7]["lang_probs"])
    assert abs(float(cf["lang_probs"].astype(np.float64).sum()) - 1.0) <= 1e-6
    assert full[2] == sp["lang0"] + int(cf["lang_probs"].argmax())


def test_what_is_present_without_timestamps_and_without_dtw(engine):
    from crispy_amd.asr import transcribe_batch
    eng, sp = engine
    x = _clips()[1]
    eng.set_confidence(True)
    try:
        plain = transcribe_batch(eng, [x], timestamps=False, with_confidence=True)[0][3]
        nodtw = transcribe_batch(eng, [x], timestamps=True, with_confidence=True)[0]
    finally:
        eng.set_confidence(False)
    # no_timestamps: the plain arg-max takes no log-soft-max -- no plog (status OK); the language distribution is there
    assert plain["plog"] is None and plain["n"] == 0 and plain["p_forced"] is None and plain["word_probs"] is None
    assert plain["lang_probs"] is not None and plain["lang_probs"].shape == (sp["n_lang"],)
    # the switch on, no dtw_token_timestamps: plog and the language distribution, nothing teacher-forced
    cf = nodtw[3]
    assert cf["p_forced"] is None and cf["word_probs"] is None and cf["n_words"] == 0
    assert cf["plog"] is not None and len(cf["plog"]) == len(nodtw[1]) > 0 and cf["lang_probs"] is not None
    assert nodtw[2] == sp["lang0"] + int(cf["lang_probs"].argmax())


def test_words_with_confidence_wrapper_and_a_random_init_engine(tmp_path_factory):
    """A random-init engine (the weights of tests/test_gpu_decision.py), language auto-detected: the switch changes nothing else,
    every window's plog sums to its avg_logprob, and the host wrapper returns (t0, t1, word, prob)."""
    from crispy_amd import synth_audio
    from crispy_amd.asr import WhisperEngine, transcribe_batch, transcribe_words_with_confidence
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    from tests.test_gpu_decision import _engine_file
    hp = HParams.tiny()
    sp = _sp(hp)
    W = synthetic_whisper_weights(hp, 0, sensitive=True)
    W["decoder.ln.weight"] = W["decoder.ln.weight"] * np.float32(4.0)
    eng = WhisperEngine(_engine_file(tmp_path_factory, hp, W, "conf-random"))
    try:
        eng.set_precision(1)
        x = synth_audio.clip16k_np(83, 16000 * 9)
        kw = dict(timestamps=True, with_segments=True, with_words=True, dtw=True, with_confidence=True, max_new_tokens=24, fallback=False)
        off = transcribe_batch(eng, [x], **kw)[0]
        eng.set_confidence(True)
        on = transcribe_batch(eng, [x], **kw)[0]
        eng.set_confidence(False)
        _same_but_confidence(on, off)
        cf = on[7]
        assert np.array_equal(cf["plog"], off[7]["plog"]) and off[7]["lang_probs"] is None
        assert on[2] == sp["lang0"] + int(cf["lang_probs"].argmax())
        text = np.array(on[1]) < sp["eot"]
        if cf["p_forced"] is not None and text.any() and on[6]:
            assert ((cf["p_forced"][text] >= 0) & (cf["p_forced"][text] <= 1)).all() and (cf["p_forced"][~text] == -1).all()
        got = transcribe_words_with_confidence(eng, x, 60.0, max_new_tokens=24)
        assert eng.last_confidence["word_probs"] is not None
        assert [(a, b, w) for a, b, w, _p in got] == [(60.0 + a, 60.0 + b, w) for a, b, w, _f, _n in eng.last_words]
        assert [p for *_x, p in got] == [float(v) for v in eng.last_confidence["word_probs"]]
    finally:
        eng.close()

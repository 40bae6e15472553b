"""The confidence oracle (tests/confidence_oracle.py): its teacher-forced log-probabilities against HF transformers'
WhisperForConditionalGeneration on the seeded Whisper-tiny weights (the model of tests/golden/whisper_tiny_golden.npz), the
word mean and its order with merge_punctuations on a written vocabulary, the language soft-max."""
import os
import sys

import numpy as np
import pytest

from tests import confidence_oracle as CO

GOLD = os.path.join(os.path.dirname(__file__), "golden", "whisper_tiny_golden.npz")


@pytest.fixture(scope="module")
def tiny():
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams.tiny()
    return hp, synthetic_whisper_weights(hp, 0)


def test_teacher_forced_logprobs_match_transformers(tiny):
    """float64 oracle against f32 torch.  The bar: tests/test_oracle_whisper.py holds the oracle's decoder logits to HF's
    within 5e-5 (absolute, these weights); a log-probability is a logit minus a log-sum-exp, and each of the two moves by at
    most the largest logit difference: 1e-4."""
    pytest.importorskip("transformers")
    import torch
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from hf_names import hf_name
    from oracle import whisper_oracle as WO
    hp, W = tiny
    model = WhisperForConditionalGeneration(WhisperConfig()).eval()      # WhisperConfig() defaults are the tiny dims
    sd = model.state_dict()
    for n, v in W.items():
        sd[hf_name(n)].copy_(torch.from_numpy(v))
    sd["proj_out.weight"].copy_(torch.from_numpy(W["decoder.token_embedding.weight"]))
    model.load_state_dict(sd)
    sp = WO.special_tokens(hp.n_vocab)
    rng = np.random.default_rng(5)
    enc = (rng.standard_normal((hp.n_audio_ctx, hp.n_audio_state)) * 0.5).astype(np.float32)
    greedy = np.load(GOLD)["greedy_tokens"].tolist()
    text = [t for t in greedy if t < sp["eot"]][:6] + [0, sp["eot"] - 1] + rng.integers(0, sp["eot"], 5).tolist()
    row = [sp["sot"], sp["lang0"], sp["transcribe"], sp["not_"]] + text + [sp["eot"]]
    got = CO.token_logprobs(W, hp, enc, row, 3)
    with torch.no_grad():
        lg = model(encoder_outputs=(torch.from_numpy(enc)[None],), decoder_input_ids=torch.tensor([row[:-1]])).logits[0]
        ref = lg[3:, :sp["eot"]].float().log_softmax(-1).numpy()      # openai: logits[len(sot):, :eot].softmax(-1)
    want = np.array([ref[i, t] for i, t in enumerate(text)], np.float64)
    assert got.shape == want.shape == (len(text),)
    err = np.abs(got - want).max()
    print(f"oracle vs transformers: max |d log p| {err:.2e} over {len(text)} tokens (log p {want.min():.2f} .. {want.max():.2f})")
    assert err < 1e-4


def test_word_mean_is_taken_before_the_punctuation_merge():
    """The written vocabulary of test_word_split_and_punctuation_merge_on_a_written_vocabulary: a word's probability is the
    mean over ITS tokens as split; the marks merged into it afterwards add tokens to it and leave the probability alone."""
    euro = "€".encode()
    pieces = [b" Hello", b",", b" wor", b"ld", b" (", b"costs", b" 5", euro[:2], euro[2:], b")", b".", b" \"", b"ok", b"\""]
    p = np.array([0.9, 0.001, 0.5, 0.25, 0.8, 0.4, 0.6, 0.3, 0.9, 0.002, 0.003, 0.7, 0.1, 0.004], np.float32)
    ww = CO.word_probs(pieces, p)
    assert [w[0] for w in ww] == [" Hello,", " world", " (costs", " 5€).", " \"ok\""]
    assert [(w[1], w[2]) for w in ww] == [(0, 2), (2, 2), (4, 2), (6, 5), (11, 3)]
    mean = lambda a: np.float32(sum(float(v) for v in a) / len(a))
    assert ww[0][3] == mean(p[0:1])            # " Hello" alone: the comma's 0.001 is not in it
    assert ww[1][3] == mean(p[2:4])
    assert ww[2][3] == mean(p[4:6])            # " (" + "costs" were ONE word before the merge
    assert ww[3][3] == mean(p[6:9])            # " 5" + the two halves of the euro sign; ")" and "." merged in later
    assert ww[4][3] == mean(p[11:13])
    assert all(w[3].dtype == np.float32 for w in ww)
    # every unit a word of its own (languages written without spaces): the means are the tokens' own
    uu = CO.word_probs([b"\xe4\xbd", b"\xa0", b"\xe5\xa5\xbd"], np.array([0.5, 0.25, 0.125], np.float32), unicode_only=True)
    assert [(w[0], float(w[3])) for w in uu] == [("你", 0.375), ("好", 0.125)]


@pytest.mark.parametrize("n_vocab,n_lang", [(51865, 99), (51866, 100), (51864, 0)])
def test_language_softmax(n_vocab, n_lang):
    from oracle import whisper_oracle as WO
    rng = np.random.default_rng(n_vocab)
    lg = rng.standard_normal(n_vocab) * 30.0
    sp = WO.special_tokens(n_vocab)
    lg[sp["sot"]] = 1e4                       # outside the language range: must not enter
    pr = CO.lang_probs(lg, n_vocab)
    assert pr.shape == (n_lang,)
    if n_lang:
        assert abs(pr.sum() - 1.0) < 1e-12 and pr.min() >= 0
        assert int(pr.argmax()) == int(lg[sp["lang0"]:sp["lang0"] + n_lang].argmax())


def test_log_softmax_stays_finite_where_the_probability_underflows():
    lg = np.zeros(1000)
    lg[7] = 2000.0
    assert CO.log_softmax_at(lg, 1000, 7) == 0.0
    assert CO.log_softmax_at(lg, 1000, 8) == -2000.0
    assert CO.log_softmax_at(lg, 7, 3) == pytest.approx(-np.log(7.0))      # column 7 is outside the crop

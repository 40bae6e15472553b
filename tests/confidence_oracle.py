"""Oracle of the confidence numbers (crispy_asr_set_confidence): float64 numpy on oracle/whisper_oracle.py's decoder.

  token_logprobs(...)   openai-whisper's text_token_probs in the log domain [UPSTREAM-RECALL: whisper/timing.py find_alignment:
                        `logits[len(sot):, :eot].softmax(-1)` gathered at the text tokens]: the teacher-forced decoder over
                        sot sequence + <|notimestamps|> + text + <|endoftext|>, log-soft-max over the ids below <|endoftext|>
                        of the unfiltered logits.  f16=True: the oracle's f16-operand arithmetic (precision mode 1).
  word_probs(...)       the mean of the token probabilities over a word's tokens as split, BEFORE merge_punctuations; a word
                        that absorbed a punctuation mark keeps its own mean (tests/align_oracle.py: split_words,
                        merge_punctuations -- merge_punctuations merges .word and .tokens only)
  lang_probs(...)       whisper.cpp's whisper_lang_auto_detect: soft-max of the <|startoftranscript|> logits over the language
                        tokens only
"""
import numpy as np

from oracle import whisper_oracle as WO
from tests import align_oracle as AO


def log_softmax_at(logits, n_cols, target):
    """log soft-max over logits[:n_cols], at `target` (float64)."""
    lg = np.asarray(logits, np.float64)[:n_cols]
    m = lg.max()
    return float(lg[target] - (m + np.log(np.exp(lg - m).sum())))


def token_logprobs(weights, hp, enc_out, row, n_sot, f16=False, with_logits=False):
    """row = sot sequence (n_sot ids), <|notimestamps|>, text tokens, <|endoftext|>.  Returns logp [len(row) - n_sot - 2]:
    entry i = log p(row[n_sot + 1 + i] | row[:n_sot + 1 + i]); with_logits also the logits rows those were read from."""
    eot = WO.special_tokens(hp.n_vocab)["eot"]
    dc = WO.DecoderCache(weights, hp, np.asarray(enc_out, np.float64), f16=f16)
    out, rows = [], []
    for q, t in enumerate(row[:-2]):
        lg = dc.step(t)
        if q >= n_sot:
            out.append(log_softmax_at(lg, eot, row[q + 1]))
            rows.append(lg)
    out = np.asarray(out, np.float64)
    return (out, np.stack(rows)) if with_logits else out


def word_probs(pieces, p_tokens, unicode_only=False):
    """pieces: the window's text tokens as byte strings; p_tokens: their probabilities (float32, as published).  Returns
    [(word, first, n, prob float32)] of the words kept after merge_punctuations: prob = float32(sum in float64, token order,
    / n) of the word AS SPLIT."""
    ws = AO.split_words(pieces, unicode_only)
    full = []
    for t, f, n in ws:
        s = 0.0
        for i in range(n):
            s += float(np.float32(p_tokens[f + i]))
        full.append([t, f, n, np.float32(s / n)])
    return [(t, f, n, p) for t, f, n, p in AO.merge_punctuations(full)]


def lang_probs(logits, n_vocab):
    """logits of the <|startoftranscript|> position -> soft-max over the language tokens [n_lang] (float64)."""
    sp = WO.special_tokens(n_vocab)
    lg = np.asarray(logits, np.float64)[sp["lang0"]:sp["lang0"] + sp["n_lang"]]
    if lg.size == 0:
        return lg
    e = np.exp(lg - lg.max())
    return e / e.sum()

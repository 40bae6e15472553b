"""The oracle side of tests/test_gpu_long_audio.py: whisper_full's seek loop past 30 s.

  * the two scripted models of the loop test (the decoder ignores the audio; tests/scripted_model.py) -- about 2 s of
    oracle each, computed in the test;
  * the clip on which the audio matters: random-init tiny, ~44 s, the numpy log-mel of the whole clip
    (tests/long_logmel_oracle.py) as `mel_window`, the real float64 encoder per window.  That is tens of seconds of numpy,
    so its result is committed through tests/oracle_cache.py; `python -m tests.long_audio_cases` writes the entry
    (tests/golden/oracle_cache/long_audio_real.json), `... search` tries seeds until one meets the three conditions the
    test asserts."""
import numpy as np

N_LONG = 1123457            # 70.2 s: not a multiple of 160, nor of a 64-frame tile
REAL_SEED, REAL_N, REAL_MAX_NEW = 92, 700001, 10
WIN_KEYS = ("seek", "seek_advance", "temperature", "decoder", "failed", "is_no_speech", "tokens", "prompt", "no_speech_prob",
            "avg_logprob", "entropy")


def bare_script(hp):
    """(A) every window on the bare prompt says "<|0.00|> w1 w2 <|22.00|><|22.00|> EOT": the seek advances by 2200 frames."""
    from tests.oracle_cases import wcpp_masks
    from tests.scripted_model import script_rows, scripted_whisper_weights
    sp, _, _ = wcpp_masks(hp)
    BEG, EOT = sp["beg"], sp["eot"]
    return scripted_whisper_weights(hp, script_rows(2, [BEG, 1001, 1002, BEG + 1100, BEG + 1100, EOT]), gain=100.0)


def past_script(hp):
    """(B) the same five picks after a prompt of 3 tokens and after <|startofprev|> + 5 k tokens of text so far + 3
    (generation then starts at position 3 + 5 k).  The first pick of those later windows is a two-token row
    [(EOT, 1.0), (<|0.00|>, 0.9)]: inside a window (the position after the previous window's fifth pick) EOT wins and ends
    it; at a window's first position suppress_blank masks EOT and <|0.00|> wins."""
    from tests.oracle_cases import wcpp_masks
    from tests.scripted_model import script_rows, scripted_whisper_weights
    sp, _, _ = wcpp_masks(hp)
    BEG, EOT = sp["beg"], sp["eot"]
    five = [BEG, 1001, 1002, BEG + 1100, BEG + 1100]
    rows = script_rows(2, five + [EOT])
    for k in (1, 2, 3):
        rows.update(script_rows(3 + 5 * k, [[(EOT, 1.0), (BEG, 0.9)]] + five[1:]))
    rows.update(script_rows(3 + 5 * 4, [EOT]))
    return scripted_whisper_weights(hp, rows, gain=100.0)


def slim(wins):
    """What the tests compare of the oracle's windows (the rest -- every iteration, every decoder -- is working state)."""
    out = []
    for w in wins:
        d = {k: w[k] for k in WIN_KEYS}
        d["min_margin"] = float(min(w["margins"])) if w["margins"] else float("inf")
        out.append(d)
    return out


def real_inputs(seed=REAL_SEED, n=REAL_N):
    from crispy_amd import synth_audio
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams.tiny()
    return hp, synthetic_whisper_weights(hp, 0), synth_audio.clip16k_np(seed, n)


def real_case(seed=REAL_SEED, n=REAL_N):
    """The oracle's whisper_full over the whole clip, and the last window's avg_logprob when that window is fed the mel of
    window 0 instead of its own (the prompt and everything before it unchanged)."""
    from crispy_amd.ggml_io import synthetic_vocab
    from oracle import whisper_oracle as WO
    from tests import long_logmel_oracle as LO
    from tests.oracle_cases import wcpp_masks
    hp, W, x = real_inputs(seed, n)
    sp, sup, sup_first = wcpp_masks(hp)
    vocab = synthetic_vocab(hp.n_vocab)
    r = LO.raw(x, hp.n_mels)
    encs = {}

    def enc_of(seek):
        if seek not in encs:
            encs[seek] = WO.encoder_forward(W, hp, LO.window(r, seek))
        return encs[seek]

    def run(mel_window):
        return WO.transcribe_timestamps(W, hp, mel_window, x.size, [sp["sot"], sp["lang0"], sp["transcribe"]], WO.RULES_WCPP,
                                        lambda t: vocab[t], n_max=REAL_MAX_NEW, suppress=sup, suppress_first=sup_first,
                                        max_windows=64, encoder=enc_of)

    segs, kept, wins = run(lambda seek: seek)                     # (`encoder` receives what `mel_window` returns: the seek)
    last = wins[-1]["seek"]
    _, _, wrong = run(lambda seek: 0 if seek == last else seek)
    assert wrong[-1]["seek"] == last and wrong[-1]["prompt"] == wins[-1]["prompt"]
    return {"segs": segs, "kept": kept, "wins": slim(wins), "wrong_last_avg_logprob": float(wrong[-1]["avg_logprob"])}


def real_fingerprint(seed=REAL_SEED, n=REAL_N):
    from tests.oracle_cache import fingerprint
    hp, W, x = real_inputs(seed, n)
    return fingerprint("long_audio_real", seed, n, REAL_MAX_NEW, x, W["decoder.token_embedding.weight"], W["encoder.conv1.weight"])


def real_ref():
    from tests.oracle_cache import cached
    return cached("long_audio_real", real_fingerprint(), real_case)


def conditions(ref, bar=1e-4):
    """The three things the clip must do for the test to mean something (tests/test_gpu_long_audio.py asserts each)."""
    wins = ref["wins"]
    return (any(w["seek"] > 3000 for w in wins), min(w["min_margin"] for w in wins),
            abs(ref["wrong_last_avg_logprob"] - wins[-1]["avg_logprob"]) / bar)


if __name__ == "__main__":
    import os
    import sys
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        for seed in range(int(sys.argv[2]) if len(sys.argv) > 2 else 91, 140):
            ref = real_case(seed)
            past, margin, moved = conditions(ref)
            print(seed, [w["seek"] for w in ref["wins"]], [len(w["prompt"]) for w in ref["wins"]], f"margin {margin:.2e} moved {moved:.0f} bars", flush=True)
            if past and margin > 3e-3 and moved > 10:
                break
    else:
        os.environ["CRISPY_ORACLE_CACHE"] = "write"
        ref = real_ref()
        print([w["seek"] for w in ref["wins"]], conditions(ref))

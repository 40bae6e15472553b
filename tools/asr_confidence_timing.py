"""What `crispy_asr_set_confidence` costs: `crispy_asr_transcribe_batch` with `dtw_token_timestamps`, seeded random-init
weights, precision mode 1, the switch off and then on -- and the same call without the alignment, so that the alignment's own
cost stands beside what the switch adds to it.

  --dims tiny     Whisper-tiny
  --dims d1280    width 1280 / 20 heads / 4 decoder layers / vocabulary 51866 (large-v3-turbo's decoder); the encoder cut to 4
                  layers -- the switch adds work to the decoder's alignment pass only, and 32 random encoder layers are 3 GB of
                  weights to make and write for nothing

Prints one JSON line: per configuration the wall times in ms of --repeat calls (each ends in a device synchronise; one
warm-up call first), the windows of the call and how many of them were aligned (kept text).  A library without the switch
(an older build picked through CRISPY_HIP_LIB, for the A/B of the switch-off call) reports the first two rows only.
Nothing gates on these numbers.

    python tools/asr_confidence_timing.py [--dims tiny] [--batch 64] [--repeat 5] [--max-new-tokens 0]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from crispy_amd import synth_audio  # noqa: E402
from crispy_amd.asr import WhisperEngine, transcribe_batch  # noqa: E402
from crispy_amd.ggml_io import synthetic_vocab, write_ggml  # noqa: E402
from crispy_amd.mel_filters import whisper_mel_filters  # noqa: E402
from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights  # noqa: E402


def timed(fn, repeat):
    out = fn()                            # warm-up: workspaces grown, code objects loaded, decode steps captured
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return [round(v, 3) for v in times], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", choices=["tiny", "d1280"], default="tiny")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max-new-tokens", type=int, default=0)
    a = ap.parse_args()
    hp = HParams.tiny() if a.dims == "tiny" else HParams(n_vocab=51866, n_audio_state=1280, n_audio_head=20, n_audio_layer=4,
                                                         n_text_state=1280, n_text_head=20, n_text_layer=4, n_mels=128)
    clips = [synth_audio.clip16k_np(300 + i, 480000) for i in range(a.batch)]
    d = tempfile.mkdtemp()
    path = os.path.join(d, "ggml-synth.bin")
    write_ggml(path, hp, synthetic_whisper_weights(hp, 0), whisper_mel_filters(hp.n_mels), synthetic_vocab(hp.n_vocab), f16=False)
    eng = WhisperEngine(path)
    eng.set_precision(1)
    has_switch = hasattr(eng._L, "crispy_asr_set_confidence")

    def call(dtw, conf):
        if has_switch:
            eng._ck(eng._L.crispy_asr_set_confidence(eng._h, 1 if conf else 0))
        r = transcribe_batch(eng, clips, a.max_new_tokens, timestamps=True, with_segments=True, with_words=dtw, dtw=dtw)
        eng.synchronize()
        wins = [w for c in r for w in c[4]]
        return {"windows": len(wins), "windows_with_text": sum(1 for w in wins if w["n_tokens"] > 0 and not w["no_speech"]),
                "tokens": sum(len(c[1]) for c in r), "words": sum(len(c[6]) for c in r) if dtw else 0}

    out = {"dims": a.dims, "batch": a.batch, "precision_mode": 1, "library": os.environ.get("CRISPY_HIP_LIB", "built tree"),
           "has_switch": has_switch}
    rows = [("dtw_off", False, False), ("dtw_on_switch_off", True, False)] + ([("dtw_on_switch_on", True, True)] if has_switch else [])
    for name, dtw, conf in rows:
        ms, info = timed(lambda: call(dtw, conf), a.repeat)
        out[name] = {"ms": ms, "min_ms": min(ms), **info}
    if has_switch:
        eng._ck(eng._L.crispy_asr_set_confidence(eng._h, 0))
        n = max(1, out["dtw_on_switch_on"]["windows_with_text"])
        out["alignment_ms"] = round(out["dtw_on_switch_off"]["min_ms"] - out["dtw_off"]["min_ms"], 3)
        out["switch_adds_ms"] = round(out["dtw_on_switch_on"]["min_ms"] - out["dtw_on_switch_off"]["min_ms"], 3)
        out["switch_adds_ms_per_aligned_window"] = round(out["switch_adds_ms"] / n, 4)
    print(json.dumps(out))
    eng.close()
    shutil.rmtree(d)


if __name__ == "__main__":
    main()

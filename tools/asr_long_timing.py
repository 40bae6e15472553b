"""One long recording, two ways through the library, Whisper-tiny (seeded random-init weights), precision mode 1:

  crispy_asr_transcribe            ONE whisper_full over the whole audio: the log-mel of all of it, then 30 s windows one
                                   after the other, each starting where the last closed timestamp pair ended and carrying the
                                   text so far -- serial by construction
  crispy_asr_transcribe_recording  run_transcription's hard 30 s cuts, the chunks decoded side by side

Prints one JSON line with both wall times (each the best of --repeat calls that end in a device synchronise, after one
warm-up call) and the number of windows each made.  Nothing gates on these numbers: they say what continuity costs.

    python tools/asr_long_timing.py [--minutes 10] [--repeat 3] [--max-new-tokens 0]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from crispy_amd import synth_audio  # noqa: E402
from crispy_amd.asr import WhisperEngine, transcribe_recording  # noqa: E402
from crispy_amd.ggml_io import synthetic_vocab, write_ggml  # noqa: E402
from crispy_amd.mel_filters import whisper_mel_filters  # noqa: E402
from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights  # noqa: E402


def best_of(fn, repeat):
    fn()                                  # warm-up: workspaces grown, code objects loaded, decode steps captured
    times = []
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-new-tokens", type=int, default=0)
    a = ap.parse_args()
    hp = HParams.tiny()
    n = int(a.minutes * 60 * 16000)
    x = np.concatenate([synth_audio.clip16k_np(200 + i, min(480000, n - at)) for i, at in enumerate(range(0, n, 480000))])
    d = tempfile.mkdtemp()
    path = os.path.join(d, "ggml-tiny-synth.bin")
    write_ggml(path, hp, synthetic_whisper_weights(hp, 0), whisper_mel_filters(hp.n_mels), synthetic_vocab(hp.n_vocab), f16=False)
    eng = WhisperEngine(path)
    eng.set_precision(1)

    def one_call():
        eng.transcribe(x, a.max_new_tokens, timestamps=True)
        return len(eng.last_windows)

    def chunked():
        return len(transcribe_recording(eng, x, a.max_new_tokens, timestamps=True, with_result=True)[4])

    t_full, w_full = best_of(one_call, a.repeat)
    t_rec, w_rec = best_of(chunked, a.repeat)
    print(json.dumps({"seconds_of_audio": n / 16000.0, "precision_mode": 1, "model": "tiny (random-init)",
                      "transcribe_s": round(t_full, 4), "transcribe_windows": w_full,
                      "transcribe_recording_s": round(t_rec, 4), "transcribe_recording_windows": w_rec,
                      "ratio": round(t_full / t_rec, 2)}))
    eng.close()
    shutil.rmtree(d)


if __name__ == "__main__":
    main()

"""Developer tool: what word-level timestamps (crispy_asr_opts::dtw_token_timestamps) cost.

  python tools/prof_align.py [--out profiles/r07_align.json] [--reps 3] [--no-medium]
      wall time of crispy_asr_transcribe_batch with the option off and on: 64 x 30 s clips of a seeded Whisper-tiny file
      (precision mode 1, whisper.cpp's default options) and one 30 s chunk of a seeded medium q4_1 file (resident);
      medians of --reps calls after one warm-up, written as JSON.
  rocprofv3 --kernel-trace --stats -d <dir> -o align -- python tools/prof_align.py --trace-only
      one 64-clip call with the option on, for the kernel statistics (align_rowstats_kernel, align_matrix_kernel,
      align_dtw_kernel next to the decoder's kernels)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from crispy_amd import synth_audio  # noqa: E402
from crispy_amd.asr import WhisperEngine, transcribe_batch  # noqa: E402
from crispy_amd.ggml_io import synthetic_vocab, write_ggml, write_ggml_quantized  # noqa: E402
from crispy_amd.mel_filters import whisper_mel_filters  # noqa: E402
from crispy_amd.whisper_weights import HParams, LazyWeights, synthetic_whisper_weights  # noqa: E402


def timed(eng, clips, reps, **kw):
    transcribe_batch(eng, clips, timestamps=True, **kw)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = transcribe_batch(eng, clips, timestamps=True, **kw)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r07_align.json")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-medium", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    hp = HParams.tiny()
    path = os.path.join(tmp, "tiny.bin")
    write_ggml(path, hp, synthetic_whisper_weights(hp, 0), whisper_mel_filters(80), synthetic_vocab(hp.n_vocab), f16=False)
    eng = WhisperEngine(path)
    eng.set_precision(1)
    clips = [synth_audio.clip16k_np(100 + i, 480000) for i in range(64)]
    if a.trace_only:
        transcribe_batch(eng, clips, timestamps=True, dtw=True)
        eng.close()
        return
    rec = {}
    off, r_off = timed(eng, clips, a.reps)
    on, r_on = timed(eng, clips, a.reps, dtw=True)
    assert [r[:2] for r in r_on] == [r[:2] for r in r_off]
    rec["tiny_64x30s"] = {"off_ms": off, "on_ms": on, "added": on / off - 1.0,
                          "tokens": int(sum(len(r[1]) for r in r_off))}
    eng.close()
    if not a.no_medium:
        hpm = HParams.medium()
        pm = os.path.join(tmp, "medium-q4_1.bin")
        write_ggml_quantized(pm, hpm, LazyWeights(hpm, 0, sensitive=True), whisper_mel_filters(hpm.n_mels),
                             synthetic_vocab(hpm.n_vocab), "q4_1", keep=False)
        em = WhisperEngine(pm, resident=True)
        x = [synth_audio.clip16k_np(7, 480000)]
        off, _ = timed(em, x, a.reps)
        on, _ = timed(em, x, a.reps, dtw=True)
        rec["medium_q4_1_1x30s"] = {"off_ms": off, "on_ms": on, "added": on / off - 1.0}
        em.close()
    print(json.dumps(rec, indent=1))
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

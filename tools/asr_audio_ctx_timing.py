"""What `crispy_asr_set_audio_ctx` buys: the encoder, one decoded position and a whole `crispy_asr_transcribe_batch` call at
reduced audio contexts, seeded random-init weights, precision mode 1.

  --dims tiny     Whisper-tiny
  --dims d1024    two layers of width 1024 / 16 heads (medium's width: the matrix-vector decode step), one encoder layer

Rows of the one JSON line it prints (every list: the --repeat timed runs after one warm-up run of the same shape, in ms):
  encode          `crispy_asr_encode_device` of --clips clips on a stream of the tool's own, DEVICE time between two events
                  recorded around the call, at n = 1500 (not set), 750, 375, 128
  position        one decoded position at 1 row and at 512 rows: host clock around `crispy_asr_decode_greedy_device` (the call
                  returns tokens to the host, so it ends synchronised) with 33 new tokens minus the same with 1, over 32
  transcribe      `crispy_asr_transcribe_batch` of --clips clips of 7 s, timestamps on, not set against n = 384; host clock, the
                  call ends in a device synchronise
A library without the setter (an older build: run this file from that tree) reports the not-set rows only -- the A/B of "not
set costs nothing".  Nothing gates on these numbers.

    python tools/asr_audio_ctx_timing.py [--dims tiny] [--clips 64] [--repeat 7]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from crispy_amd import synth_audio  # noqa: E402
from crispy_amd.asr import WhisperEngine, transcribe_batch  # noqa: E402
from crispy_amd.ggml_io import synthetic_vocab, write_ggml  # noqa: E402
from crispy_amd.mel_filters import whisper_mel_filters  # noqa: E402
from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights  # noqa: E402

CONTEXTS = (1500, 750, 375, 128)


def spread(ms):
    return {"ms": [round(v, 3) for v in ms], "min_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3),
            "max_ms": round(max(ms), 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", choices=["tiny", "d1024"], default="tiny")
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    hp = HParams.tiny() if a.dims == "tiny" else HParams(n_audio_state=1024, n_audio_head=16, n_audio_layer=1, n_text_state=1024,
                                                         n_text_head=16, n_text_layer=2)
    d = tempfile.mkdtemp()
    path = os.path.join(d, "ggml-synth.bin")
    write_ggml(path, hp, synthetic_whisper_weights(hp, 0), whisper_mel_filters(hp.n_mels), synthetic_vocab(hp.n_vocab), f16=False)
    eng = WhisperEngine(path)
    eng.set_precision(1)
    has_setter = hasattr(eng._L, "crispy_asr_set_audio_ctx")
    set_ctx = (lambda n: eng._ck(eng._L.crispy_asr_set_audio_ctx(eng._h, 0 if n == hp.n_audio_ctx else n))) if has_setter else (lambda n: None)
    contexts = CONTEXTS if has_setter else CONTEXTS[:1]
    out = {"dims": a.dims, "clips": a.clips, "precision_mode": 1, "repeat": a.repeat, "has_setter": has_setter,
           "encode": {}, "position": {}, "transcribe": {}}
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)

    # ---- the encoder: device time between events on the tool's stream ----
    B = a.clips
    melt = torch.zeros(B, 3002, hp.n_mels, device=dev)
    melt[:, 1:3001] = (torch.rand(B, 3000, hp.n_mels, generator=g) * 2.5 - 1.0).to(dev)      # rows 0 and 3001: the padding
    enc = torch.empty(B, hp.n_audio_ctx, hp.n_audio_state, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    for n in contexts:
        set_ctx(n)
        ms = []
        for i in range(a.repeat + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            eng.encode_device(melt.data_ptr(), B, enc.data_ptr(), stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
        out["encode"][str(n)] = spread(ms)
    del melt

    # ---- one decoded position ----
    prompt = [50258, 50259, 50359, 50363]
    for rows in (1, 512):
        d_enc = (torch.randn(rows, hp.n_audio_ctx, hp.n_audio_state, generator=g) * 0.8).to(dev)
        torch.cuda.synchronize()
        for n in contexts:
            set_ctx(n)
            view = d_enc.view(-1)[:rows * n * hp.n_audio_state]              # [rows][n][d]: the first rows * n * d floats
            per = []
            for i in range(a.repeat + 1):
                t = {}
                for n_new in (1, 33):
                    t0 = time.perf_counter()
                    eng.decode_greedy_device(view.data_ptr(), rows, prompt, n_new)
                    t[n_new] = (time.perf_counter() - t0) * 1e3
                if i:
                    per.append((t[33] - t[1]) / 32.0)
            out["position"][f"rows{rows}_n{n}"] = spread(per)
        del d_enc

    # ---- a whole transcribe call ----
    clips = [synth_audio.clip16k_np(300 + i, 16000 * 7) for i in range(a.clips)]
    for n in ((hp.n_audio_ctx, 384) if has_setter else (hp.n_audio_ctx,)):
        set_ctx(n)
        ms, info = [], {}
        for i in range(a.repeat + 1):
            t0 = time.perf_counter()
            r = transcribe_batch(eng, clips, 0, timestamps=True, with_segments=True)
            eng.synchronize()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
            info = {"windows": sum(len(c[4]) for c in r), "tokens": sum(len(c[1]) for c in r)}
        out["transcribe"]["unset" if n == hp.n_audio_ctx else f"n{n}"] = {**spread(ms), **info}
    set_ctx(hp.n_audio_ctx)
    print(json.dumps(out))
    eng.close()
    shutil.rmtree(d)


if __name__ == "__main__":
    main()

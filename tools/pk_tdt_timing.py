"""Timing of Parakeet's TDT decoder (crispy_pk_tdt_*, include/crispy_hip.h) on the MI355X, for NOTEBOOK section 36: the catalog
widths (D 640, L 2, V 8193, 5 durations, H 1024) with seeded random weights (tests/pk_tdt_oracle.py) on 64 clips of 375 seeded frames
(30 s each) in one call.  The blank bias is set so that about one step in five emits a token, duration 0 is biased away (a random
network otherwise stays at one frame until the budget ends), and the realised rate is reported.

  * device time of crispy_pk_tdt_decode_device by events around the call: the trimmed mean (a tenth off each end) of --reps calls
    after warm-up, with the step count (the longest clip's) and the time per step;
  * that time by stage -- projector, prediction network, joint, advance -- from events the developer build records around every
    launch (CRISPY_PK_TDT_TIMELINE, libcrispy_hip_dev.so; a second handle in this process);
  * the group size: the same call of the developer build with CRISPY_PK_TDT_GROUP steps between two reads of the counter;
  * the comparison: the float32 torch loop of tests/pk_tdt_oracle.py on this machine's host threads over a few of the clips, scaled
    up -- a STAND-IN for ONNX Runtime on the CPU, which is not installed;
  * as a sanity check of the run, whether the device's steps on those clips equal that loop's.

    python tools/pk_tdt_timing.py [--clips 64] [--frames 375] [--blank-bias 8.7] [--reps 20] [--threads 16] [--host-clips 2] [--json OUT]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pk_tdt_oracle as TO      # noqa: E402

STAGES = ("projector", "prediction", "joint", "advance")


def timeline(dec, frames):
    """one call of the developer build with the stage split it prints to stderr"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            dec.decode_device(frames)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode("utf-8", "replace")
    m = re.findall(r"crispy_pk_tdt timeline: (\d+) steps enqueued, projector ([\d.]+) ms, prediction ([\d.]+) ms, joint ([\d.]+) ms, advance ([\d.]+) ms", text)
    if not m:
        raise RuntimeError(f"the developer build printed no timeline: {text[-1000:]}")
    return int(m[-1][0]), dict(zip(STAGES, (float(v) for v in m[-1][1:])))


def timed(dec, frames, reps):
    import torch
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = dec.decode_device(frames, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    cut = len(ms) // 10
    kept = ms[cut:len(ms) - cut]
    return sum(kept) / len(kept), ms[0], ms[-1], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=375)
    ap.add_argument("--blank-bias", type=float, default=8.7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-clips", type=int, default=2, help="clips the host stand-in computes (its time is scaled up)")
    ap.add_argument("--groups", default="8,16,32,64,128")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from crispy_amd import _native as N
    from crispy_amd.parakeet import ParakeetTDT
    cfg = TO.CATALOG_TDT
    w = TO.make_tdt_weights(cfg, 1, blank_bias=a.blank_bias, duration_bias=(-30.0, 1.5, 0.5, 0.0, 0.0))
    clips = [TO.frames(a.frames, cfg.hidden, 1000 + c) for c in range(a.clips)]
    frames = [torch.from_numpy(x).cuda() for x in clips]

    dev = ParakeetTDT(0, lib=N.load_variant("dev"))
    dev.load(cfg.as_dict(), w)
    dev.decode_device(frames[:1])
    dev.decode_device(frames)                   # the workspace at its full size
    groups = {}
    for g in (int(x) for x in a.groups.split(",")):
        os.environ["CRISPY_PK_TDT_GROUP"] = str(g)      # read by the developer build only
        groups[g] = timed(dev, frames, max(5, a.reps // 2))[0]
    del os.environ["CRISPY_PK_TDT_GROUP"]
    os.environ["CRISPY_PK_TDT_TIMELINE"] = "1"
    timeline(dev, frames)
    enqueued, stage = timeline(dev, frames)
    del os.environ["CRISPY_PK_TDT_TIMELINE"]
    dev.close()

    dec = ParakeetTDT(0)
    dec.load(cfg.as_dict(), w)
    dec.decode_device(frames[:1])      # warm-up: code objects
    dec.decode_device(frames)          # ... and the workspace at its full size
    mean, lo, hi, out = timed(dec, frames, a.reps)
    steps = [s.cpu().numpy() for s in out]
    dec.close()
    n_steps = max(len(s) for s in steps)
    total = sum(len(s) for s in steps)
    tokens = sum(int((s[:, 0] != cfg.blank).sum()) for s in steps)
    predict_steps = len({int(i) for s in steps for i in np.nonzero(s[:, 0] != cfg.blank)[0]})      # steps at which any clip emitted

    torch.set_num_threads(a.threads)
    host = TO.Tdt(cfg, w, torch.float32)
    host.decode(clips[0][:8])
    sub = min(a.host_clips, a.clips)
    t0 = time.perf_counter()
    ref = [host.decode(x) for x in clips[:sub]]
    torch_ms = 1e3 * (time.perf_counter() - t0) * a.clips / sub
    same = [bool(r.shape == s.shape and np.array_equal(r, s)) for r, s in zip(ref, steps)]
    res = {"device": torch.cuda.get_device_name(0), "config": cfg.as_dict(), "clips": a.clips, "frames_per_clip": a.frames,
           "blank_bias": a.blank_bias, "call_ms_trimmed_mean": mean, "call_ms_min": lo, "call_ms_max": hi, "reps": a.reps,
           "steps_of_the_longest_clip": n_steps, "steps_enqueued_dev_build": enqueued, "us_per_step": 1e3 * mean / n_steps,
           "steps_all_clips": total, "tokens_all_clips": tokens, "token_rate": tokens / total, "steps_with_a_prediction": predict_steps,
           "stage_ms_dev_build": stage, "call_ms_by_group_dev_build": groups, "torch_f32_ms_scaled": torch_ms, "torch_threads": a.threads,
           "torch_clips_run": sub, "device_steps_equal_torch_f32": same}
    print(f"{a.clips} clips x {a.frames} frames: crispy_pk_tdt_decode_device {mean:.2f} ms (trimmed mean of {a.reps}; {lo:.2f} - {hi:.2f}), "
          f"{n_steps} steps of the longest clip, {1e3 * mean / n_steps:.1f} us per step; {tokens} tokens in {total} steps of all clips "
          f"(rate {tokens / total:.2f}), a prediction at {predict_steps} steps; developer build by stage over {enqueued} enqueued steps: "
          + ", ".join(f"{k} {stage[k]:.2f}" for k in STAGES) + " ms; by group size: " + ", ".join(f"{g}: {v:.2f}" for g, v in groups.items())
          + f" ms; float32 torch loop on {a.threads} threads {torch_ms:.0f} ms (from {sub} clips); device steps equal it: {same}", flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

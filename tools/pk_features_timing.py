"""Timing of Parakeet's log-mel front end and of the whole arm (crispy_pk_features*, crispy_pk_transcribe*, include/crispy_hip.h) on the
MI355X, for NOTEBOOK section 37: 64 clips of 30 s of seeded noise (192 000 rows at 128 mel bins) in one call.

  * device time of crispy_pk_features_device by events around the call: the trimmed mean (a tenth off each end) of --reps calls after
    warm-up, and the bytes the call has to move (samples read once; rows before normalisation written once and read twice, by the
    partial sums and by the normalisation; rows written once) with the fraction of the HBM rate that is;
  * that time by launch -- frame kernel, statistics, normalisation -- from events the developer build records
    (CRISPY_PK_MEL_TIMELINE, libcrispy_hip_dev.so; a second handle in this process);
  * crispy_pk_transcribe_device at the catalog widths with seeded random weights (tests/pk_oracle.py, tests/pk_tdt_oracle.py), beside
    the three stages called one after the other (--layers 0 skips this part);
  * the comparison: the float32 torch restatement of tests/pk_mel_oracle.py on this machine's host threads over a few of the clips,
    scaled up;
  * as a sanity check of the run, the largest distance between the device's rows and that restatement's on those clips.

    python tools/pk_features_timing.py [--clips 64] [--seconds 30] [--reps 20] [--layers 24] [--threads 16] [--host-clips 4] [--json OUT]
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

from tests import pk_mel_oracle as MO      # noqa: E402
from tests import pk_oracle as PO          # noqa: E402
from tests import pk_tdt_oracle as TO      # noqa: E402

STAGES = ("frames", "statistics", "normalise")
HBM_GBS = 8000.0      # MI355X


def timeline(enc, pcm, M):
    """one call of the developer build with the split it prints to stderr"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            enc.features_device(pcm, mel_bins=M)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode("utf-8", "replace")
    m = re.findall(r"crispy_pk_mel timeline: \d+ rows in \d+ tiles, frames ([\d.]+) ms, statistics ([\d.]+) ms, normalise ([\d.]+) ms", text)
    if not m:
        raise RuntimeError(f"the developer build printed no timeline: {text[-1000:]}")
    return dict(zip(STAGES, (float(v) for v in m[-1])))


def timed(call, reps):
    """trimmed mean, min and max of `reps` calls by events on torch's stream; call(stream) -> result"""
    import torch
    ms, out = [], None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = call(torch.cuda.current_stream().cuda_stream)
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
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--mel-bins", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=24, help="encoder blocks of the transcribe part; 0 skips it")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-clips", type=int, default=4, help="clips the host restatement computes (its time is scaled up)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from crispy_amd import _native as N
    from crispy_amd.parakeet import Parakeet, ParakeetEncoder
    M, n = a.mel_bins, int(a.seconds * 16000)
    clips = [MO.noise(n, 2000 + c) for c in range(a.clips)]
    pcm = [torch.from_numpy(x).cuda() for x in clips]
    rows = a.clips * MO.rows(n)
    moved = 4 * (a.clips * n + 4 * rows * M)      # samples; rows before normalisation written, read twice; rows written

    os.environ["CRISPY_PK_MEL_TIMELINE"] = "1"      # read by the developer build only
    dev = ParakeetEncoder(0, lib=N.load_variant("dev"))
    dev.features_device(pcm[:1], mel_bins=M)
    timeline(dev, pcm, M)                           # the workspace at its full size
    stage = timeline(dev, pcm, M)
    dev.close()
    del os.environ["CRISPY_PK_MEL_TIMELINE"]

    enc = ParakeetEncoder(0)
    enc.features_device(pcm[:1], mel_bins=M)      # warm-up: code objects, tables
    enc.features_device(pcm, mel_bins=M)          # ... and the workspace at its full size
    mean, lo, hi, out = timed(lambda s: enc.features_device(pcm, mel_bins=M, stream=s), a.reps)
    sub = min(a.host_clips, a.clips)
    got = [o.cpu().numpy() for o in out[:sub]]
    enc.close()

    torch.set_num_threads(a.threads)
    fb = MO.slaney_filters(M)
    MO.features(clips[0][:4000], fb, torch.float32)
    t0 = time.perf_counter()
    ref = [MO.features(x, fb, torch.float32)[0] for x in clips[:sub]]
    torch_ms = 1e3 * (time.perf_counter() - t0) * a.clips / sub
    worst = max(float(np.abs(g - r).max()) for g, r in zip(got, ref))
    floor_ms = moved / (HBM_GBS * 1e9) * 1e3
    res = {"device": torch.cuda.get_device_name(0), "clips": a.clips, "samples_per_clip": n, "mel_bins": M, "rows": rows, "reps": a.reps,
           "features_ms_trimmed_mean": mean, "features_ms_min": lo, "features_ms_max": hi, "stage_ms_dev_build": stage, "bytes_moved": moved,
           "hbm_floor_ms": floor_ms, "fraction_of_hbm_rate": floor_ms / mean, "torch_f32_ms_scaled": torch_ms, "torch_threads": a.threads,
           "torch_clips_run": sub, "worst_row_diff_to_torch_f32": worst}
    print(f"{a.clips} clips x {a.seconds:g} s ({rows} rows, M {M}): crispy_pk_features_device {mean:.3f} ms (trimmed mean of {a.reps}; {lo:.3f} - {hi:.3f}); "
          f"developer build by launch: " + ", ".join(f"{k} {stage[k]:.3f}" for k in STAGES) + f" ms; {moved / 1e9:.3f} GB moved, {floor_ms:.3f} ms at "
          f"{HBM_GBS:g} GB/s ({100 * floor_ms / mean:.0f} % of the HBM rate); float32 torch restatement on {a.threads} threads {torch_ms:.0f} ms (from "
          f"{sub} clips); worst |device - torch f32| row value {worst:.2e}", flush=True)

    if a.layers > 0:
        cfg, tcfg = PO.with_flags(PO.CATALOG_V3, layers=a.layers, mel_bins=M), TO.CATALOG_TDT
        state = {"encoder." + k: v for k, v in PO.make_weights(cfg, 1).items()}
        state.update(TO.make_tdt_weights(tcfg, 1, blank_bias=8.7, duration_bias=(-30.0, 1.5, 0.5, 0.0, 0.0)))
        pk = Parakeet(0)
        pk.load(cfg.as_dict(), tcfg.as_dict(), state)
        del state
        pk.transcribe_device(pcm[:1])
        pk.transcribe_device(pcm)
        reps = max(3, a.reps // 5)
        whole = timed(lambda s: pk.transcribe_device(pcm, stream=s), reps)
        own = timed(lambda s: pk.transcribe_device(pcm), reps)      # the handles' own streams, ordered by the event
        f_ms = timed(lambda s: pk.encoder.features_device(pcm, stream=s), reps)
        e_ms = timed(lambda s: pk.encoder.encode_device(f_ms[3], stream=s), reps)
        d_ms = timed(lambda s: pk.decoder.decode_device(e_ms[3], stream=s), reps)
        same = all(bool(np.array_equal(x["steps"].cpu().numpy(), y.cpu().numpy())) for x, y in zip(whole[3], d_ms[3]))
        steps = sum(len(x["steps"]) for x in whole[3])
        pk.close()
        res.update({"layers": a.layers, "transcribe_ms_trimmed_mean": whole[0], "transcribe_ms_min": whole[1], "transcribe_ms_max": whole[2],
                    "transcribe_own_streams_ms": own[0], "stage_call_ms": {"features": f_ms[0], "encode": e_ms[0], "decode": d_ms[0]},
                    "stage_sum_ms": f_ms[0] + e_ms[0] + d_ms[0], "transcribe_steps_equal_stages": same, "steps_all_clips": steps, "transcribe_reps": reps})
        print(f"crispy_pk_transcribe_device ({a.layers} blocks): {whole[0]:.1f} ms on one stream ({whole[1]:.1f} - {whole[2]:.1f}), {own[0]:.1f} ms on the "
              f"handles' own streams; the stages alone: features {f_ms[0]:.2f}, encode {e_ms[0]:.1f}, decode {d_ms[0]:.1f}, sum "
              f"{f_ms[0] + e_ms[0] + d_ms[0]:.1f} ms; {steps} steps; transcribe's steps equal the stages': {same}", flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

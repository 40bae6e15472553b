"""Timing of the segmentation network (crispy_diar_seg_*, include/crispy_hip.h) on the MI355X, for NOTEBOOK and the README row:
a 1 h recording of i16 -- 57.6 M samples, 361 windows of 10 s -- in one call, with seeded weights (tests/seg_oracle.py).

  * device time of crispy_diar_seg_scores_device by events around the call, after warm-up (the call returns when its work is
    complete, so the events bracket every launch of its turns and the final synchronisation);
  * that time by kernel family -- front (windows, instance-norm statistics, the three convolutions), projections, recurrence,
    head -- from events the developer build records between the families (CRISPY_DIAR_SEG_TIMELINE, libcrispy_hip_dev.so), in
    a child process of its own so that the timed calls above run the release library undisturbed;
  * wall time of crispy_diar_seg_scores (host in, host out: 115 MB of samples in, 6 MB of scores out);
  * the comparison: the float32 torch oracle of tests/seg_oracle.py on this machine's host threads over a subset of the windows,
    scaled up -- a STAND-IN for ONNX Runtime on the CPU, which is not installed;
  * as a sanity check of the run, the largest distance between the device's scores and that oracle's on the subset.

    python tools/diar_seg_timing.py [--windows 361] [--threads 16] [--host-windows 16] [--json OUT]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import seg_oracle as SO      # noqa: E402

WIN = 160000


def recording(n_windows):
    """(n_windows - 1) * 10 s of i16: noise whose level changes every 2.5 s"""
    rng = np.random.default_rng(3)
    n = (n_windows - 1) * WIN
    level = np.repeat(rng.uniform(0.002, 0.3, n // 40000 + 1), 40000)[:n].astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * level
    return (np.clip(x, -1, 1) * np.float32(32767.0)).astype(np.int16)


def child(a):
    """one timed call in the developer build: the library prints the family split to stderr"""
    import torch
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    d.load_segmentation(SO.make_weights(1))
    d_pcm = torch.from_numpy(recording(a.windows)).cuda()
    d.segmentation_scores_device(d_pcm[:WIN])
    d.segmentation_scores_device(d_pcm)
    d.segmentation_scores_device(d_pcm)
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=361)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-windows", type=int, default=16, help="windows the host stand-in computes (its time is scaled up)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    # the family split first, in a process of its own (this one has not touched the device yet)
    env = dict(os.environ, CRISPY_HIP_LIB=os.path.join(ROOT, "crispy_amd", "libcrispy_hip_dev.so"), CRISPY_DIAR_SEG_TIMELINE="1")
    cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--windows", str(a.windows)], env=env, capture_output=True,
                        text=True, timeout=600)
    lines = re.findall(r"crispy_diar_seg timeline: front ([\d.]+) ms, projections ([\d.]+) ms, recurrence ([\d.]+) ms, head ([\d.]+) ms", cp.stderr)
    if cp.returncode != 0 or not lines:
        raise RuntimeError(f"the timeline child failed ({cp.returncode}): {cp.stderr[-2000:]}")
    family = dict(zip(("front", "projections", "recurrence", "head"), (float(v) for v in lines[-1])))

    import torch
    from crispy_amd.diarize import Diarizer
    w = SO.make_weights(1)
    pcm = recording(a.windows)
    d = Diarizer(0)
    d.load_segmentation(w)
    d_pcm = torch.from_numpy(pcm).cuda()
    d.segmentation_scores_device(d_pcm[:WIN])      # warm-up: code objects
    scores = d.segmentation_scores_device(d_pcm)   # ... and the scratch at its full size
    assert scores.shape == (a.windows, 589, 7)
    dev_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        scores = d.segmentation_scores_device(d_pcm, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        host_scores = d.segmentation_scores(pcm)
        host_ms.append(1e3 * (time.perf_counter() - t))
    assert np.array_equal(host_scores.view(np.uint32), scores.cpu().numpy().view(np.uint32))
    d.close()

    torch.set_num_threads(a.threads)
    sub = min(a.host_windows, a.windows)
    net = SO.PyanNet(w, torch.float32)
    windows = SO.segmentation_windows(pcm[:sub * WIN])[:sub]
    net.scores(windows[:1])
    t = time.perf_counter()
    ref = net.scores(windows)
    torch_ms = 1e3 * (time.perf_counter() - t) * a.windows / sub
    worst = float(np.abs(host_scores[:sub] - ref).max())
    res = {"device": torch.cuda.get_device_name(0), "windows": a.windows, "samples": int(pcm.size), "windows_per_workgroup": 1,
           "device_call_ms": dev_ms, "family_ms_dev_build": family, "host_call_ms": host_ms, "torch_f32_ms_scaled": torch_ms,
           "torch_threads": a.threads, "torch_windows_run": sub, "worst_score_diff_to_torch_f32": worst}
    print(f"{a.windows} windows ({pcm.size} samples): crispy_diar_seg_scores_device {min(dev_ms):.1f} - {max(dev_ms):.1f} ms by events "
          f"(developer build, by family: front {family['front']:.1f}, projections {family['projections']:.1f}, recurrence "
          f"{family['recurrence']:.1f}, head {family['head']:.1f} ms); crispy_diar_seg_scores (host in and out) {min(host_ms):.0f} ms; "
          f"float32 torch stand-in on {a.threads} threads {torch_ms:.0f} ms (from {sub} windows); worst |device - torch f32| score "
          f"{worst:.2e}", flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

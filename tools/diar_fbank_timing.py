"""Timing of the diarization fbank (crispy_diar_fbank*, include/crispy_hip.h) on the MI355X, for NOTEBOOK and the README row:
a 2 h recording's worth of chunks -- 1800 chunks x 64000 samples of i16, 398 frames each -- in one call.

  * device time of crispy_diar_fbank_device by events around the call, after warm-up (the call returns when its work is
    complete, so the events bracket the descriptor upload, both kernels and the final synchronisation);
  * wall time of crispy_diar_fbank (host in, host out: by byte count 0.23 GB in, 0.23 GB of rows out);
  * the comparison: the float32 numpy restatement of tests/fbank_oracle.py over the same chunks on this machine's host
    threads -- a STAND-IN for knf-rs / kaldi-native-fbank, which cannot be built here;
  * as a sanity check of the run, the largest distance between the device's mel energies (the exponential of its rows
    before the mean subtraction) and that restatement's, as a fraction of the frame's largest energy.

    python tools/diar_fbank_timing.py [--chunks 1800] [--samples 64000] [--threads 16] [--json OUT]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import fbank_oracle as O      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=1800)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-chunks", type=int, default=160, help="chunks the host stand-in transforms (its time is scaled up)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from crispy_amd.diarize import Diarizer

    rng = np.random.default_rng(3)
    n = a.chunks * a.samples
    pcm = O.f32_to_i16((0.1 * rng.standard_normal(n, dtype=np.float32)))
    chunks = [(c * a.samples, a.samples) for c in range(a.chunks)]
    d = Diarizer(0)
    d_pcm = torch.from_numpy(pcm).cuda()
    d.fbank_device(d_pcm, chunks[:4], 1.0)      # warm-up: tables, code objects
    feats, off = d.fbank_device(d_pcm, chunks, 1.0)
    dev_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        feats, off = d.fbank_device(d_pcm, chunks, 1.0, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    host_ms = []
    for _ in range(2):
        t = time.perf_counter()
        rows = d.fbank(pcm, chunks, 1.0)
        host_ms.append(1e3 * (time.perf_counter() - t))
    sub = min(a.host_chunks, a.chunks)

    def one(c):
        m = O.mel_energies(pcm[c * a.samples:(c + 1) * a.samples], 1.0, np.float32)
        return m, O.subtract_mean(np.log(np.maximum(m, np.float32(O.EPS))))
    t = time.perf_counter()
    with ThreadPoolExecutor(a.threads) as ex:
        ref = list(ex.map(one, range(sub)))
    numpy_ms = 1e3 * (time.perf_counter() - t) * a.chunks / sub
    _f, raw, roff = d.fbank_device(d_pcm, chunks[:sub], 1.0, raw=True)
    raw = raw.cpu().numpy().astype(np.float64)
    worst = 0.0
    for c in range(sub):
        m = ref[c][0].astype(np.float64)
        worst = max(worst, float((np.abs(np.exp(raw[roff[c]:roff[c + 1]]) - m) / m.max(1, keepdims=True)).max()))
    assert len(rows) == a.chunks and all(r.shape == (O.n_frames(a.samples), 80) for r in rows)
    res = {"device": torch.cuda.get_device_name(0), "chunks": a.chunks, "samples": a.samples, "rows": int(off[-1]),
           "bytes_in": int(pcm.nbytes), "bytes_rows": int(off[-1]) * 320, "device_call_ms": dev_ms, "host_call_ms": host_ms,
           "numpy_f32_ms_scaled": numpy_ms, "numpy_threads": a.threads, "numpy_chunks_run": sub, "worst_energy_diff_to_numpy_f32_of_frame_max": worst}
    print(f"{a.chunks} chunks x {a.samples} samples ({int(off[-1])} rows): crispy_diar_fbank_device {min(dev_ms):.2f} - {max(dev_ms):.2f} ms "
          f"by events; crispy_diar_fbank (host in and out) {min(host_ms):.0f} ms; numpy float32 stand-in on {a.threads} threads "
          f"{numpy_ms:.0f} ms (from {sub} chunks); worst |device - numpy f32| mel energy {worst:.2e} of the frame maximum", flush=True)
    d.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

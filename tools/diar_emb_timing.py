"""Timing of the embedding network (crispy_diar_emb_*, crispy_diar_embed*, include/crispy_hip.h) on the MI355X, for NOTEBOOK and
the README row: one hour of speech as 900 chunks of 64000 samples of i16 (398 feature rows, 199 positions each) in one call,
with seeded weights (tests/emb_oracle.py).

  * device time of crispy_diar_embed_device by events around the call, after warm-up (the call returns when its work is
    complete, so the events bracket the fbank, every launch of the network's turns and the final synchronisation);
  * that time by kernel family -- head, tdnn, dense GEMMs (linear1 of the 52 layers), CAM (gates plus local convolution),
    transits, pooling plus dense -- from events the developer build records between the families (CRISPY_DIAR_EMB_TIMELINE,
    libcrispy_hip_dev.so), in a child process of its own so that the timed calls above run the release library undisturbed;
    the dense-GEMM family's achieved TFLOP/s against the 157 TF f32 matrix peak;
  * wall time of crispy_diar_embed (host in, host out);
  * the comparison: the float32 torch oracle of tests/emb_oracle.py on this machine's host threads over a subset of the chunks,
    scaled up -- a STAND-IN for ONNX Runtime on the CPU, which is not installed;
  * as a sanity check of the run, the largest distance between the device's embeddings and that oracle's on the subset.

    python tools/diar_emb_timing.py [--chunks 900] [--threads 16] [--host-chunks 8] [--json OUT]
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

from tests import emb_oracle as EO      # noqa: E402

CHUNK = 64000
FAMILIES = ("head", "tdnn", "dense gemms", "cam", "transits", "pooling")


def recording(n_chunks):
    """n_chunks * 4 s of i16: noise whose level changes every 0.5 s"""
    rng = np.random.default_rng(3)
    n = n_chunks * CHUNK
    level = np.repeat(rng.uniform(0.002, 0.3, n // 8000 + 1), 8000)[:n].astype(np.float32)
    x = rng.standard_normal(n, dtype=np.float32) * level
    return (np.clip(x, -1, 1) * np.float32(32767.0)).astype(np.int16)


def plan(n_chunks):
    return [(c * CHUNK, CHUNK) for c in range(n_chunks)]


def gemm_flop(t2):
    """multiply-adds x 2 of linear1 over the 52 dense layers for t2 positions"""
    flop, c = 0, EO.INIT_CH
    for n_layers, _d in EO.BLOCKS:
        for i in range(n_layers):
            flop += 2 * t2 * (c + i * EO.GROWTH) * EO.BN_CH
        c = (c + n_layers * EO.GROWTH) // 2
    return flop


def child(a):
    """one timed call in the developer build: the library prints the family split to stderr"""
    import torch
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    d.load_embedding(EO.make_weights(1))
    d_pcm = torch.from_numpy(recording(a.chunks)).cuda()
    d.embed_chunks_device(d_pcm, plan(1))
    d.embed_chunks_device(d_pcm, plan(a.chunks))
    d.embed_chunks_device(d_pcm, plan(a.chunks))
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=900)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-chunks", type=int, default=8, help="chunks the host stand-in computes (its time is scaled up)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    # the family split first, in a process of its own (this one has not touched the device yet)
    env = dict(os.environ, CRISPY_HIP_LIB=os.path.join(ROOT, "crispy_amd", "libcrispy_hip_dev.so"), CRISPY_DIAR_EMB_TIMELINE="1")
    cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--chunks", str(a.chunks)], env=env, capture_output=True,
                        text=True, timeout=600)
    lines = re.findall(r"crispy_diar_emb timeline: head ([\d.]+) ms, tdnn ([\d.]+) ms, dense gemms ([\d.]+) ms, cam ([\d.]+) ms, "
                       r"transits ([\d.]+) ms, pooling ([\d.]+) ms", cp.stderr)
    if cp.returncode != 0 or not lines:
        raise RuntimeError(f"the timeline child failed ({cp.returncode}): {cp.stderr[-2000:]}")
    family = dict(zip(FAMILIES, (float(v) for v in lines[-1])))
    t2 = EO.emb_frames(1 + (CHUNK - 400) // 160)
    gemm_tflops = gemm_flop(t2) * a.chunks / (family["dense gemms"] * 1e-3) / 1e12

    import torch
    from crispy_amd.diarize import Diarizer
    w = EO.make_weights(1)
    pcm = recording(a.chunks)
    chunks = plan(a.chunks)
    d = Diarizer(0)
    d.load_embedding(w)
    d_pcm = torch.from_numpy(pcm).cuda()
    d.embed_chunks_device(d_pcm, chunks[:1])      # warm-up: code objects
    emb = d.embed_chunks_device(d_pcm, chunks)    # ... and the scratch at its full size
    assert emb.shape == (a.chunks, 512)
    dev_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        emb = d.embed_chunks_device(d_pcm, chunks, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    host_ms = []
    for _ in range(3):
        t = time.perf_counter()
        host_emb = d.embed_chunks(pcm, chunks)
        host_ms.append(1e3 * (time.perf_counter() - t))
    assert np.array_equal(host_emb.view(np.uint32), emb.cpu().numpy().view(np.uint32))
    sub = min(a.host_chunks, a.chunks)
    rows = d.fbank(pcm, chunks[:sub])
    d.close()

    torch.set_num_threads(a.threads)
    net = EO.CAMPPlus(w, torch.float32)
    net.embed(rows[0])
    t = time.perf_counter()
    ref = np.stack([net.embed(r) for r in rows])
    torch_ms = 1e3 * (time.perf_counter() - t) * a.chunks / sub
    worst = float(np.abs(host_emb[:sub] - ref).max())
    res = {"device": torch.cuda.get_device_name(0), "chunks": a.chunks, "samples": int(pcm.size), "device_call_ms": dev_ms,
           "family_ms_dev_build": family, "dense_gemm_tflops": gemm_tflops, "f32_matrix_peak_tflops": 157.3, "host_call_ms": host_ms,
           "torch_f32_ms_scaled": torch_ms, "torch_threads": a.threads, "torch_chunks_run": sub, "worst_embedding_diff_to_torch_f32": worst}
    print(f"{a.chunks} chunks ({pcm.size} samples): crispy_diar_embed_device {min(dev_ms):.1f} - {max(dev_ms):.1f} ms by events (developer "
          f"build, by family: " + ", ".join(f"{k} {family[k]:.1f}" for k in FAMILIES) + f" ms; dense GEMMs {gemm_tflops:.1f} TFLOP/s of 157 peak); "
          f"crispy_diar_embed (host in and out) {min(host_ms):.0f} ms; float32 torch stand-in on {a.threads} threads {torch_ms:.0f} ms (from {sub} "
          f"chunks); worst |device - torch f32| embedding {worst:.2e}", flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

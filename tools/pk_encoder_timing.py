"""Timing of the Parakeet FastConformer encoder (crispy_pk_*, include/crispy_hip.h) on the MI355X, for NOTEBOOK and the README row:
the catalog config (H 1024, 24 blocks, 8 heads, ffn 4096, K 9, C 256, M 128) with seeded random weights (tests/pk_oracle.py) on
64 clips of 3000 feature rows, which is what the 30 s chunker hands the engine, in one call.

  * device time of crispy_pk_encode_device by events around the call, after warm-up (the call returns when its work is complete);
  * that time by stage -- subsampling, GEMMs, attention, depthwise convolution, LayerNorm -- from events the developer build
    records between the stages (CRISPY_PK_TIMELINE, libcrispy_hip_dev.so; a second handle in this process), and the GEMM stage's
    and the whole call's achieved TFLOP/s against the 157 TF f32 matrix peak;
  * the comparison: the float32 torch oracle of tests/pk_oracle.py on this machine's host threads over a few of the clips,
    scaled up -- a STAND-IN for ONNX Runtime on the CPU, which is not installed;
  * as a sanity check of the run, the largest distance between the device's frames and that oracle's on those clips.

    python tools/pk_encoder_timing.py [--clips 64] [--rows 3000] [--layers 24] [--threads 16] [--host-clips 1] [--json OUT]
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

from tests import pk_oracle as PO      # noqa: E402

STAGES = ("subsampling", "gemms", "attention", "convolution", "layernorm")
PEAK_TFLOPS = 157.3


def flop(cfg, t, n_clips):
    """(GEMM, attention) floating-point operations of a call of n_clips clips of t frames each, multiply-adds x 2; the attention's
    count is what the kernel does per 32 x 32 tile pair: scores, the 64-column band product and P . V"""
    H, F = cfg.hidden, cfg.ffn
    frames = t * n_clips
    gemm = 2 * frames * (cfg.sub_channels * (cfg.mel_bins // 8) * H + cfg.layers * (4 * H * F + 7 * H * H))
    gemm += 2 * cfg.layers * (2 * t - 1) * H * H      # R = relative_k_proj(pos), once per block and call
    tiles = -(-t // 32)
    attn = 2 * cfg.layers * n_clips * cfg.heads * tiles * tiles * (32 * 32 * 128 + 32 * 64 * 128 + 32 * 32 * 128)
    return gemm, attn


def timeline(enc, feats):
    """one call of the developer build with the stage split it prints to stderr"""
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            enc.encode_device(feats)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode("utf-8", "replace")
    m = re.findall(r"crispy_pk timeline: subsampling ([\d.]+) ms, gemms ([\d.]+) ms, attention ([\d.]+) ms, convolution ([\d.]+) ms, "
                   r"layernorm ([\d.]+) ms", text)
    if not m:
        raise RuntimeError(f"the developer build printed no timeline: {text[-1000:]}")
    return dict(zip(STAGES, (float(v) for v in m[-1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-clips", type=int, default=1, help="clips the host stand-in computes (its time is scaled up)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch
    from crispy_amd import _native as N
    from crispy_amd.parakeet import ParakeetEncoder
    cfg = PO.with_flags(PO.CATALOG_V3, layers=a.layers)
    w = PO.make_weights(cfg, 1)
    rng = np.random.default_rng(2)
    clips = [rng.standard_normal((a.rows, cfg.mel_bins), dtype=np.float32) for _ in range(a.clips)]
    feats = [torch.from_numpy(x).cuda() for x in clips]
    t = PO.frames(a.rows)
    gemm_flop, attn_flop = flop(cfg, t, a.clips)

    os.environ["CRISPY_PK_TIMELINE"] = "1"      # read by the developer build only
    dev = ParakeetEncoder(0, lib=N.load_variant("dev"))
    dev.load(cfg.as_dict(), w)
    dev.encode_device(feats[:1])
    timeline(dev, feats)                        # the workspace at its full size
    stage = timeline(dev, feats)
    dev.close()

    enc = ParakeetEncoder(0)
    enc.load(cfg.as_dict(), w)
    enc.encode_device(feats[:1])      # warm-up: code objects
    out = enc.encode_device(feats)    # ... and the workspace at its full size
    dev_ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = enc.encode_device(feats, stream=torch.cuda.current_stream().cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    sub = min(a.host_clips, a.clips)
    got = [o.cpu().numpy() for o in out[:sub]]
    enc.close()

    torch.set_num_threads(a.threads)
    net = PO.Encoder(cfg, w, torch.float32)
    net.forward([clips[0][:64]])
    t0 = time.perf_counter()
    ref = net.forward(clips[:sub])
    torch_ms = 1e3 * (time.perf_counter() - t0) * a.clips / sub
    worst = max(float(np.abs(g - r[0]).max()) for g, r in zip(got, ref))
    best = min(dev_ms)
    res = {"device": torch.cuda.get_device_name(0), "config": cfg.as_dict(), "clips": a.clips, "rows": a.rows, "frames_per_clip": t,
           "device_call_ms": dev_ms, "stage_ms_dev_build": stage, "gemm_tflop": gemm_flop / 1e12, "attention_tflop": attn_flop / 1e12,
           "gemm_stage_tflops": gemm_flop / (stage["gemms"] * 1e-3) / 1e12, "attention_stage_tflops": attn_flop / (stage["attention"] * 1e-3) / 1e12,
           "call_tflops": (gemm_flop + attn_flop) / (best * 1e-3) / 1e12, "f32_matrix_peak_tflops": PEAK_TFLOPS,
           "torch_f32_ms_scaled": torch_ms, "torch_threads": a.threads, "torch_clips_run": sub, "worst_frame_diff_to_torch_f32": worst}
    print(f"{a.clips} clips x {a.rows} rows ({t} frames each, {a.layers} blocks): crispy_pk_encode_device {min(dev_ms):.1f} - {max(dev_ms):.1f} ms by "
          f"events; developer build by stage: " + ", ".join(f"{k} {stage[k]:.1f}" for k in STAGES) + f" ms; GEMM stage "
          f"{res['gemm_stage_tflops']:.1f} TFLOP/s, attention {res['attention_stage_tflops']:.1f}, whole call {res['call_tflops']:.1f} of "
          f"{PEAK_TFLOPS} peak ({100 * res['call_tflops'] / PEAK_TFLOPS:.0f} %); float32 torch stand-in for ONNX Runtime on {a.threads} threads "
          f"{torch_ms:.0f} ms (from {sub} clips); worst |device - torch f32| frame value {worst:.2e}", flush=True)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

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

  * with --precision 1 the same in precision mode 1 (f16 operands in the GEMMs, against the 2.5 PF f16 roof), with --alternate both
    modes call by call in one session; the bytes of A and C the GEMM stage moves per second; the memory mode 1's copies take;
  * with --attention-precision 1 the attention's three products on f16 operands (crispy_pk_set_attention_precision), and with
    --alternate attention both attention modes call by call in one session, the GEMMs fixed in precision mode 1.

    python tools/pk_encoder_timing.py [--clips 64] [--rows 3000] [--layers 24] [--threads 16] [--host-clips 1] [--precision {0,1}]
                                      [--attention-precision {0,1}] [--alternate [precision|attention]] [--json OUT]
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
PEAK_F16_TFLOPS = 2500.0      # the dense f16 matrix roof, mode 1's GEMMs


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
    ap.add_argument("--precision", type=int, choices=(0, 1), default=0, help="crispy_pk_set_precision: 0 f32 operands, 1 f16 operands in the GEMMs")
    ap.add_argument("--attention-precision", type=int, choices=(0, 1), default=0,
                    help="crispy_pk_set_attention_precision: 0 f32 operands, 1 f16 operands in the attention's three products")
    ap.add_argument("--alternate", nargs="?", const="precision", default=None, choices=("precision", "attention"),
                    help="alternate call by call in this one session: both precision modes (the default), or with `attention` both attention "
                         "modes with the GEMMs in precision mode 1")
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

    # a mode is (precision, attention precision); its label is the precision alone unless the attention is in mode 1 or alternates
    if a.alternate == "attention":
        modes = [(1, 0), (1, 1)]
    else:
        modes = [(g, a.attention_precision) for g in ([0, 1] if a.alternate else [a.precision])]
    label = lambda m: str(m[0]) if a.alternate != "attention" and not a.attention_precision else f"{m[0]}, attention {m[1]}"
    peak = {0: PEAK_TFLOPS, 1: PEAK_F16_TFLOPS}

    def select(e, m):
        e.set_precision(m[0])
        e.set_attention_precision(m[1])

    os.environ["CRISPY_PK_TIMELINE"] = "1"      # read by the developer build only
    dev = ParakeetEncoder(0, lib=N.load_variant("dev"))
    dev.load(cfg.as_dict(), w)
    stage = {}
    for _ in range(2):                          # the first round sizes the workspace and packs mode 1's copies; the second is reported
        for mode in modes:
            select(dev, mode)
            dev.encode_device(feats[:1])
            stage[mode] = timeline(dev, feats)
    dev.close()

    enc = ParakeetEncoder(0)
    enc.load(cfg.as_dict(), w)
    added = 0
    dev_ms, out = {m: [] for m in modes}, {}
    for mode in modes:
        free0 = torch.cuda.mem_get_info()[0]
        select(enc, mode)
        if mode[0] == 1 and not added:
            added = free0 - torch.cuda.mem_get_info()[0]      # the f16 copies of the GEMM weights, packed by this call
        enc.encode_device(feats[:1])      # warm-up: code objects
        enc.encode_device(feats)          # ... and the workspace at its full size
    for _ in range(a.reps):
        for mode in modes:                # the modes alternate inside one session
            select(enc, mode)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out[mode] = enc.encode_device(feats, stream=torch.cuda.current_stream().cuda_stream)
            e1.record()
            torch.cuda.synchronize()
            dev_ms[mode].append(e0.elapsed_time(e1))
    sub = min(a.host_clips, a.clips)
    got = {m: [o.cpu().numpy() for o in out[m][:sub]] for m in modes}
    enc.close()

    torch_ms, worst = None, {}
    if sub > 0:
        torch.set_num_threads(a.threads)
        net = PO.Encoder(cfg, w, torch.float32)
        net.forward([clips[0][:64]])
        t0 = time.perf_counter()
        ref = net.forward(clips[:sub])
        torch_ms = 1e3 * (time.perf_counter() - t0) * a.clips / sub
        worst = {m: max(float(np.abs(g - r[0]).max()) for g, r in zip(got[m], ref)) for m in modes}
    # bytes of A read and C written by the GEMMs of a call, each once: what the stage moves at the least besides the weights
    H, F = cfg.hidden, cfg.ffn
    frames = t * a.clips
    ac_bytes = 4 * frames * (cfg.sub_channels * (cfg.mel_bins // 8) + H + cfg.layers * (2 * (H + F) + 2 * (F + 2 * H) + (H + 3 * H) + 3 * H + (H + H) + 3 * H))
    res = {"device": torch.cuda.get_device_name(0), "config": cfg.as_dict(), "clips": a.clips, "rows": a.rows, "frames_per_clip": t,
           "gemm_tflop": gemm_flop / 1e12, "attention_tflop": attn_flop / 1e12, "gemm_a_and_c_gbytes": ac_bytes / 1e9,
           "f16_weight_copies_bytes": int(added), "torch_f32_ms_scaled": torch_ms, "torch_threads": a.threads, "torch_clips_run": sub, "modes": {}}
    for m in modes:
        best = min(dev_ms[m])
        r = {"device_call_ms": dev_ms[m], "stage_ms_dev_build": stage[m], "gemm_stage_tflops": gemm_flop / (stage[m]["gemms"] * 1e-3) / 1e12,
             "attention_stage_tflops": attn_flop / (stage[m]["attention"] * 1e-3) / 1e12, "call_tflops": (gemm_flop + attn_flop) / (best * 1e-3) / 1e12,
             "matrix_peak_tflops": peak[m[0]], "precision": m[0], "attention_precision": m[1], "gemm_a_and_c_tbytes_per_s": ac_bytes / (stage[m]["gemms"] * 1e-3) / 1e12,
             "worst_frame_diff_to_torch_f32": worst.get(m)}
        res["modes"][label(m)] = r
        print(f"precision {label(m)}: {a.clips} clips x {a.rows} rows ({t} frames each, {a.layers} blocks): crispy_pk_encode_device {min(dev_ms[m]):.1f} - "
              f"{max(dev_ms[m]):.1f} ms by events; developer build by stage: " + ", ".join(f"{k} {stage[m][k]:.1f}" for k in STAGES) + f" ms; GEMM stage "
              f"{r['gemm_stage_tflops']:.1f} TFLOP/s of {peak[m[0]]:g} peak ({100 * r['gemm_stage_tflops'] / peak[m[0]]:.0f} %), its A and C at "
              f"{r['gemm_a_and_c_tbytes_per_s']:.2f} TB/s; attention {r['attention_stage_tflops']:.1f} TFLOP/s"
              + (f"; worst |device - torch f32| frame value {worst[m]:.2e}" if m in worst else ""), flush=True)
    if torch_ms is not None:
        print(f"float32 torch stand-in for ONNX Runtime on {a.threads} threads {torch_ms:.0f} ms (from {sub} clips)")
    if added:
        print(f"mode 1's f16 copies of the GEMM weights: {added / 1e9:.2f} GB of device memory")
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

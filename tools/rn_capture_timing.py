"""Developer tool (GPU box): what the capture callback's first statement costs on the device, and what the device's own
sample format saves a host-fed handle.

  rn_capture_kernel       per format, B streams x N_FRAMES frames x CHANNELS channels, rows on a 16-byte pitch (the 16-byte
                          loads) and on an odd stride (the fallback): device events around a crispy_rn_capture_device on a
                          bypassed handle whose resampler runs at 4.8 GHz, so that it emits one sample and the second kernel of
                          the call is an empty launch; bytes moved and GB/s
  crispy_rn_capture       host-fed, i16 mono and i16 stereo, 100 ms of audio at 44.1 kHz: wall time of the whole call
  the route it replaces   the same audio converted and downmixed with numpy on the host, crispy_rn_level, crispy_rn_push, on a
                          second handle in the same process and run

Medians after warm-up.  B=4096 N_FRAMES=4410 CHANNELS=2 STEPS=9."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from crispy_amd import synthetic_weights
from crispy_amd.denoise import DenoiseState

B = int(os.environ.get("B", 4096))
N_FRAMES = int(os.environ.get("N_FRAMES", 4410))
CHANNELS = int(os.environ.get("CHANNELS", 2))
STEPS = int(os.environ.get("STEPS", 9))
COPY_GBS = 6290.0            # float4 copy on this part, measured (HBM3E: 8 TB/s spec)
DTYPES = {"f32": np.float32, "i16": np.int16, "u16": np.uint16}

w = synthetic_weights(0)
stream = torch.cuda.current_stream()
sp = stream.cuda_stream
rng = np.random.default_rng(1)
res = {"streams": B, "n_frames": N_FRAMES, "channels": CHANNELS, "kernel": {}, "host_fed": {}}


def raw(fmt, n_elems):
    if fmt == "f32":
        return rng.uniform(-0.5, 0.5, size=(B, n_elems)).astype(np.float32)
    lo, hi = (-16384, 16384) if fmt == "i16" else (16384, 49152)
    return rng.integers(lo, hi, size=(B, n_elems)).astype(DTYPES[fmt])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


# ---- the kernel ---------------------------------------------------------------------------------------------------------
kern_h = DenoiseState(w, B, 0)
kern_h.bypass_configure(4.8e9)
d_out = torch.zeros(B, 8, device="cuda")
d_mono = torch.zeros(B, N_FRAMES + 3 & ~3, device="cuda")
for fmt, dtype in DTYPES.items():
    item = np.dtype(dtype).itemsize
    n_elems = N_FRAMES * CHANNELS
    x = raw(fmt, n_elems)
    for form, stride in (("aligned", (n_elems * item + 15) // 16 * 16 // item), ("odd_stride", n_elems + 1 + n_elems % 2)):
        rows = np.zeros((B, stride), dtype=dtype)
        rows[:, :n_elems] = x
        d_in = torch.from_numpy(rows.view(np.uint8)).cuda()

        def capture():
            kern_h.capture_device(d_in.data_ptr(), stride, N_FRAMES, CHANNELS, fmt, d_out.data_ptr(), 8, d_mono.data_ptr(),
                                  d_mono.shape[1], stream=sp)

        for _ in range(3):
            capture()
        torch.cuda.synchronize()
        ms = statistics.median(timed(capture) for _ in range(STEPS))
        moved = B * N_FRAMES * (CHANNELS * item + 4)
        res["kernel"][f"{fmt}_{form}"] = {"ms": round(ms, 4), "bytes": moved, "gbs": round(moved / ms / 1e6, 1),
                                         "of_copy": round(moved / ms / 1e6 / COPY_GBS, 3)}
        print(f"rn_capture_kernel {fmt} x {CHANNELS} ch, {form}: {ms:.4f} ms, {moved / 1e9:.3f} GB, {moved / ms / 1e6:.0f} GB/s "
              f"({100 * moved / ms / 1e6 / COPY_GBS:.0f} % of the {COPY_GBS:.0f} GB/s copy rate)")
kern_h.close()

# ---- host-fed: one capture against the route it replaces ---------------------------------------------------------------
for channels in (1, 2):
    cap_h, ref_h = DenoiseState(w, B, 0), DenoiseState(w, B, 0)
    cap_h.adapter_configure(44100.0, 1.0)
    ref_h.adapter_configure(44100.0, 1.0)
    blocks = [raw("i16", 4410 * channels) for _ in range(3 + STEPS)]
    t_cap, t_ref, t_conv = [], [], []
    for k, x in enumerate(blocks):
        t0 = time.perf_counter()
        out_c, rms_c = cap_h.capture(x, channels)
        t1 = time.perf_counter()
        f = x.astype(np.float32) / np.float32(32768)
        mono = f if channels == 1 else (np.float32(0) + f[:, 0::2] + f[:, 1::2]) / np.float32(2)
        mono = np.ascontiguousarray(mono)
        t2 = time.perf_counter()
        rms_r = ref_h.level(mono)
        out_r = ref_h.push(mono)
        t3 = time.perf_counter()
        assert out_c.tobytes() == out_r.tobytes() and rms_c.tobytes() == rms_r.tobytes()
        if k >= 3:
            t_cap.append((t1 - t0) * 1e3)
            t_conv.append((t2 - t1) * 1e3)
            t_ref.append((t3 - t1) * 1e3)
    ms_cap, ms_ref, ms_conv = statistics.median(t_cap), statistics.median(t_ref), statistics.median(t_conv)
    up_cap, up_ref = B * 4410 * channels * 2, B * 4410 * 4 * 2          # the route uploads the f32 mono twice: level, push
    res["host_fed"][f"i16_{channels}ch"] = {"capture_ms": round(ms_cap, 3), "replaced_route_ms": round(ms_ref, 3),
                                            "of_which_numpy_ms": round(ms_conv, 3), "capture_upload_bytes": up_cap,
                                            "replaced_route_upload_bytes": up_ref, "route_over_capture": round(ms_ref / ms_cap, 3)}
    print(f"host-fed i16 x {channels} ch, {B} streams x 100 ms at 44.1 kHz: crispy_rn_capture {ms_cap:.2f} ms ({up_cap / 1e6:.1f} MB up); "
          f"numpy + crispy_rn_level + crispy_rn_push {ms_ref:.2f} ms ({up_ref / 1e6:.1f} MB up, {ms_conv:.2f} ms of it numpy): x{ms_ref / ms_cap:.2f}")
    cap_h.close(), ref_h.close()
print(json.dumps(res))

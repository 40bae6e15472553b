"""Developer tool (GPU box): what the capture-rate adapter costs on top of the denoiser.

  crispy_rn_push_device     B streams at RATE Hz, one push of FRAMES frames' worth per step (the BASELINE cfg 2 step: 4096 x 100)
  crispy_rn_process_device  the same frames (the push's d_frames48), on a second handle of the same commit and machine
  the two adapter kernels   on their own (crispy_rn_set_timing + crispy_rn_last_push_ms), with their bytes moved and GB/s

Steps are timed with device events on the stream the work is enqueued on, after warm-up, push and process alternating; the
figure reported is the median.  B=4096 RATE=44100 FRAMES=100 STEPS=9."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from crispy_amd import synthetic_weights
from crispy_amd.denoise import DenoiseState

B = int(os.environ.get("B", 4096))
RATE = float(os.environ.get("RATE", 44100))
FRAMES = int(os.environ.get("FRAMES", 100))
STEPS = int(os.environ.get("STEPS", 9))
COPY_GBS = 6290.0            # float4 copy on this part, measured (HBM3E: 8 TB/s spec)

n48 = FRAMES * 480
n_in = round(n48 * RATE / 48000.0)     # capture samples that make FRAMES frames (one sample more or less now and then)
cap = n48 + 480
g = torch.Generator(device="cuda").manual_seed(1)
t = torch.arange(n_in, device="cuda", dtype=torch.float32) / RATE
f0 = 80.0 + 320.0 * torch.rand(B, 1, device="cuda", generator=g)
x = 0.3 * torch.sin(2 * np.pi * f0 * t) + 0.05 * torch.randn(B, n_in, device="cuda", generator=g)
d_out = torch.zeros(B, cap, device="cuda")
d_frames = torch.zeros(B, cap, device="cuda")
d_y = torch.zeros(B, n48, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream

w = synthetic_weights(0)
push_h, proc_h = DenoiseState(w, B, 0), DenoiseState(w, B, 0)
push_h.adapter_configure(RATE, 0.8)


def push():
    return push_h.push_device(x.data_ptr(), n_in, n_in, d_out.data_ptr(), cap, d_frames.data_ptr(), cap, stream=sp)


def process():
    proc_h.process_device(d_f100.data_ptr(), d_y.data_ptr(), FRAMES, layout="btf", stream=sp)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


torch.cuda.synchronize()
n_outs = [push() for _ in range(3)]          # warm-up; from the second push on every push completes FRAMES frames
torch.cuda.synchronize()
FRAMES = n_outs[-1] // 480                   # what a push in steady state completes (the nominal count, give or take one)
n48 = FRAMES * 480
d_f100 = d_frames[:, :n48].contiguous()      # the frames of the last push as a [B][FRAMES][480] tensor
for _ in range(2):
    process()
torch.cuda.synchronize()
t_push, t_proc = [], []
for _ in range(STEPS):
    t_push.append(timed(push))
    t_proc.append(timed(process))
ms_push, ms_proc = statistics.median(t_push), statistics.median(t_proc)

# the adapter kernels on their own, in runs of their own (the events sit between the kernels of the step)
push_h.set_timing(True)
k_in, k_out = [], []
for _ in range(STEPS):
    push()
    torch.cuda.synchronize()
    a, b = push_h.last_push_ms()
    k_in.append(a)
    k_out.append(b)
push_h.set_timing(False)
ms_in, ms_out = statistics.median(k_in), statistics.median(k_out)
bytes_in = B * (n_in + 2 * n48) * 4 + 8 * n48        # capture samples read; staging rows and d_frames48 written; the (idx, t) table
bytes_out = B * 2 * n48 * 4                           # frame-kernel output read, d_out written
res = {
    "streams": B, "rate_hz": RATE, "frames_per_push": FRAMES, "n_in": n_in, "n_out_last": n_outs[-1],
    "push_ms": round(ms_push, 4), "process_ms": round(ms_proc, 4), "push_over_process": round(ms_push / ms_proc, 4),
    "push_ms_min_max": [round(min(t_push), 4), round(max(t_push), 4)], "process_ms_min_max": [round(min(t_proc), 4), round(max(t_proc), 4)],
    "adapt_in_ms": round(ms_in, 4), "adapt_in_bytes": bytes_in, "adapt_in_gbs": round(bytes_in / ms_in / 1e6, 1),
    "adapt_in_of_copy": round(bytes_in / ms_in / 1e6 / COPY_GBS, 3),
    "adapt_out_ms": round(ms_out, 4), "adapt_out_bytes": bytes_out, "adapt_out_gbs": round(bytes_out / ms_out / 1e6, 1),
    "adapt_out_of_copy": round(bytes_out / ms_out / 1e6 / COPY_GBS, 3),
}
print(f"{B} streams, {RATE:.0f} Hz, {FRAMES} frames per push ({n_in} capture samples): push {ms_push:.3f} ms, process {ms_proc:.3f} ms, "
      f"ratio {ms_push / ms_proc:.3f}")
print(f"rn_adapt_in_kernel  {ms_in:.3f} ms, {bytes_in / 1e9:.2f} GB, {res['adapt_in_gbs']:.0f} GB/s ({100 * res['adapt_in_of_copy']:.0f} % of the {COPY_GBS:.0f} GB/s copy rate)")
print(f"rn_adapt_out_kernel {ms_out:.3f} ms, {bytes_out / 1e9:.2f} GB, {res['adapt_out_gbs']:.0f} GB/s ({100 * res['adapt_out_of_copy']:.0f} % of the copy rate)")
print(json.dumps(res))

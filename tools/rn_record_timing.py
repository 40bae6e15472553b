"""Developer tool (GPU box): what the recording leg costs on the device, beside the playback pull as the yardstick.

  crispy_rn_record_app_push_device   B streams, one second of CHANNELS-channel app audio: downmix + ring append
  crispy_rn_level_device             B streams, the capture block of the push: the callback's level meter
  crispy_rn_record_drain_device      B streams, every frame that is ready (41 of 1152 samples), s16 stereo or f32
  crispy_rn_pull_device              the same number of output frames from the playback ring, 48 kHz -> 48 kHz, i16 x 2:
                                     rn_pull_kernel, the streaming pass this handle already had

Every round pushes a 100-frame block (which fills the mic ring and the playback ring), then runs the four calls, each timed
with device events on the caller's stream it is enqueued on; the figures are medians after warm-up and include the upload of
the drain's / the pull's per-frame table.  GB/s is against the bytes each pass must move: the drain reads two f32 rings and
writes one 32-bit word per stereo frame.  B=4096 RING=48000 CHANNELS=2 FMT=i16 STEPS=11."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from crispy_amd import synthetic_weights
from crispy_amd.denoise import DenoiseState

B = int(os.environ.get("B", 4096))
RING = int(os.environ.get("RING", 48000))
CHANNELS = int(os.environ.get("CHANNELS", 2))
STEPS = int(os.environ.get("STEPS", 11))
FMT = os.environ.get("FMT", "i16")
COPY_GBS = 6290.0            # float4 copy on this part, measured (HBM3E: 8 TB/s spec)
FRAME = DenoiseState.REC_FRAME

n_in = 100 * 480             # a 100-frame push; the very first returns 99 frames, the others 100
g = torch.Generator(device="cuda").manual_seed(1)
x = 0.3 * torch.rand(B, n_in, device="cuda", generator=g) - 0.15
app = 0.3 * torch.rand(B, n_in * CHANNELS, device="cuda", generator=g) - 0.15
d_out = torch.zeros(B, n_in, device="cuda")
d_rms = torch.zeros(B, device="cuda")
n_frames = min(RING, n_in) // FRAME
n_s = n_frames * FRAME
elem = 4 if FMT == "f32" else 2
per = 1 if FMT == "f32" else 2
d_pcm = torch.zeros(B, n_s * per * elem // 2, dtype=torch.int16, device="cuda")
d_pull = torch.zeros(B, n_s * 2, dtype=torch.int16, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream

h = DenoiseState(synthetic_weights(0), B, 0)
h.adapter_configure(48000.0, 1.0)
h.playback_configure(48000.0)
h.record_configure(RING)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def drain():
    got = h.record_drain_device(1 << 40, d_pcm.data_ptr(), n_s * per, fmt=FMT, stream=sp)
    assert got == n_frames, (got, n_frames)


def pull():
    live = h.pull_device(n_s, d_pull.data_ptr(), n_s * 2, channels=2, fmt="i16", stream=sp)
    assert live == n_s, (live, n_s)


ts = {"app": [], "level": [], "drain": [], "pull": []}
for step in range(STEPS + 3):
    h.record_configure(RING)                  # start_recording: both rings empty, so that every round is the same work
    h.push_device(x.data_ptr(), n_in, n_in, d_out.data_ptr(), n_in, stream=sp)
    t = {"app": timed(lambda: h.record_app_push_device(app.data_ptr(), n_in * CHANNELS, n_in, CHANNELS, stream=sp)),
         "level": timed(lambda: h.level_device(x.data_ptr(), n_in, n_in, d_rms.data_ptr(), stream=sp)),
         "drain": timed(drain), "pull": timed(pull)}
    if step >= 3:
        for k, v in t.items():
            ts[k].append(v)
torch.cuda.synchronize()

n_app = min(RING, n_in)
bytes_moved = {"app": B * (n_app * CHANNELS * 4 + n_app * 4), "level": B * (n_in * 4 + 4),
               "drain": B * (2 * n_s * 4 + n_s * per * elem) + 8 * n_frames, "pull": B * (n_s * 4 + n_s * 4) + 8 * n_s}
res = {"streams": B, "ring_samples": RING, "channels": CHANNELS, "format": FMT, "frames_per_drain": n_frames}
for k in ("app", "level", "drain", "pull"):
    ms = statistics.median(ts[k])
    gbs = bytes_moved[k] / ms / 1e6
    res[k] = {"ms": round(ms, 4), "ms_min_max": [round(min(ts[k]), 4), round(max(ts[k]), 4)], "bytes": bytes_moved[k], "gbs": round(gbs, 1),
              "of_copy": round(gbs / COPY_GBS, 3)}
    print(f"{k:>5}: {ms:.4f} ms ({bytes_moved[k] / 1e6:.1f} MB, {gbs:.0f} GB/s, {100 * gbs / COPY_GBS:.0f} % of the {COPY_GBS:.0f} GB/s copy rate)")
res["drain_of_pull_bandwidth"] = round(res["drain"]["gbs"] / res["pull"]["gbs"], 3)
res["app_of_pull_bandwidth"] = round(res["app"]["gbs"] / res["pull"]["gbs"], 3)
res["level_of_pull_bandwidth"] = round(res["level"]["gbs"] / res["pull"]["gbs"], 3)
print(json.dumps(res))

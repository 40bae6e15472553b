"""Developer tool (GPU box): what one playback callback costs on the device.

  crispy_rn_pull_device   B streams, FRAMES output frames per pull, 48 kHz -> OUT_RATE Hz, i16, CHANNELS interleaved channels

The ring is filled once by a push of a second's worth; every pull after that is fully live.  Pulls are timed with device
events on the caller's stream they are enqueued on, after warm-up; the figure reported is the median, which includes the
upload of the (offset, fraction) table.  B=4096 FRAMES=480 OUT_RATE=44100 CHANNELS=2 STEPS=21."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from crispy_amd import synthetic_weights
from crispy_amd.denoise import DenoiseState

B = int(os.environ.get("B", 4096))
FRAMES = int(os.environ.get("FRAMES", 480))
OUT_RATE = float(os.environ.get("OUT_RATE", 44100))
CHANNELS = int(os.environ.get("CHANNELS", 2))
STEPS = int(os.environ.get("STEPS", 21))
FMT = os.environ.get("FMT", "i16")
COPY_GBS = 6290.0            # float4 copy on this part, measured (HBM3E: 8 TB/s spec)

n_in = 48000 + 480           # the first frame is dropped: one second returned, the ring full
g = torch.Generator(device="cuda").manual_seed(1)
x = 0.3 * torch.rand(B, n_in, device="cuda", generator=g) - 0.15
d_out = torch.zeros(B, 48000, device="cuda")
elem = 4 if FMT == "f32" else 2
stride = FRAMES * CHANNELS
d_pcm = torch.zeros(B, stride * elem // 2, dtype=torch.int16, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream

h = DenoiseState(synthetic_weights(0), B, 0)
h.adapter_configure(48000.0, 1.0)
h.playback_configure(OUT_RATE)
n_out = h.push_device(x.data_ptr(), n_in, n_in, d_out.data_ptr(), 48000, stream=sp)
torch.cuda.synchronize()
assert h.playback_buffered() == n_out == 48000


def pull():
    live = h.pull_device(FRAMES, d_pcm.data_ptr(), stride, channels=CHANNELS, fmt=FMT, stream=sp)
    assert live == FRAMES, "the ring ran dry: fewer STEPS or FRAMES"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


for _ in range(3):
    pull()
torch.cuda.synchronize()
ts = [timed(pull) for _ in range(STEPS)]
ms = statistics.median(ts)
# two ring samples read per frame (neighbouring frames share most of them: counted once each), the PCM written
step = 48000.0 / OUT_RATE
bytes_moved = B * (int(FRAMES * step) * 4 + stride * elem) + 8 * FRAMES
res = {"streams": B, "frames_per_pull": FRAMES, "output_rate_hz": OUT_RATE, "channels": CHANNELS, "format": FMT,
       "pull_ms": round(ms, 4), "pull_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "bytes": bytes_moved,
       "gbs": round(bytes_moved / ms / 1e6, 1), "of_copy": round(bytes_moved / ms / 1e6 / COPY_GBS, 3)}
print(f"{B} streams, {FRAMES} frames per pull, 48000 -> {OUT_RATE:.0f} Hz, {FMT} x {CHANNELS}: pull {ms:.4f} ms "
      f"({bytes_moved / 1e6:.1f} MB, {res['gbs']:.0f} GB/s, {100 * res['of_copy']:.0f} % of the {COPY_GBS:.0f} GB/s copy rate)")
print(json.dumps(res))

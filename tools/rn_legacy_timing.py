"""Developer tool (GPU box): what the callbacks cost on the device while the handle's model is a Legacy one
(crispy_rn_model_configure: CRISPY_NS_DUMMY / CRISPY_NS_NOISY).

  crispy_rn_push_device   B streams, N_IN capture samples per push at RATE Hz, playback and recording configured: the push
                          kernel (out + raw samples into the playback ring), the recording resampler, the mic ring append
  crispy_rn_pull_device   FRAMES output frames per pull, RATE -> OUT_RATE Hz, FMT, CHANNELS interleaved channels

Calls are timed with device events on the stream they are enqueued on, after warm-up; the figures reported are the median and
the spread, which include the uploads of the position tables.  The pushes are timed first, then the pulls back to back on
the ring they filled, so every pull is fully live.  B=4096 N_IN=4410 RATE=44100 OUT_RATE=48000 FRAMES=480 CHANNELS=2 FMT=i16 STEPS=21."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from crispy_amd import synthetic_weights
from crispy_amd.denoise import DenoiseState

B = int(os.environ.get("B", 4096))
N_IN = int(os.environ.get("N_IN", 4410))
RATE = float(os.environ.get("RATE", 44100))
OUT_RATE = float(os.environ.get("OUT_RATE", 48000))
FRAMES = int(os.environ.get("FRAMES", 480))
CHANNELS = int(os.environ.get("CHANNELS", 2))
STEPS = int(os.environ.get("STEPS", 21))
FMT = os.environ.get("FMT", "i16")
REC_RING = int(os.environ.get("REC_RING", 48000))      # a second of recording ring per stream: 2 x 0.8 GB at 4096 streams
COPY_GBS = 6290.0            # float4 copy on this part, measured (HBM3E: 8 TB/s spec)

g = torch.Generator(device="cuda").manual_seed(1)
x = 0.3 * torch.rand(B, N_IN, device="cuda", generator=g) - 0.15
d_out = torch.zeros(B, N_IN, device="cuda")
elem = 4 if FMT == "f32" else 2
stride = FRAMES * CHANNELS
d_pcm = torch.zeros(B, stride * elem // 2, dtype=torch.int16, device="cuda")
stream = torch.cuda.current_stream()
sp = stream.cuda_stream

h = DenoiseState(synthetic_weights(0), B, 0)
h.adapter_configure(RATE, 0.8)
h.playback_configure(OUT_RATE)
h.record_configure(REC_RING)


def push():
    assert h.push_device(x.data_ptr(), N_IN, N_IN, d_out.data_ptr(), N_IN, stream=sp) == N_IN


def pull():
    live = h.pull_device(FRAMES, d_pcm.data_ptr(), stride, channels=CHANNELS, fmt=FMT, stream=sp)
    assert live == FRAMES, "the ring ran dry: more N_IN or fewer FRAMES"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


n_rec = N_IN * 48000.0 / RATE if abs(RATE - 48000.0) >= 1.0 else N_IN
resampled = abs(RATE - 48000.0) >= 1.0
# push: the input read, the output and the ring written; the output read again by the resampler, its rows written and read
# again by the append, the mic ring written (a pass-through resampler: the output read once, the mic ring written)
push_bytes = B * 4 * (3 * N_IN + ((N_IN + 3 * n_rec) if resampled else 2 * N_IN)) + (8 * n_rec if resampled else 0)
# pull: two ring samples read per frame (neighbouring frames share most of them: counted once each), the PCM written
pull_bytes = B * (int(FRAMES * RATE / OUT_RATE) * 4 + stride * elem) + 8 * FRAMES
res = {"streams": B, "samples_per_push": N_IN, "capture_rate_hz": RATE, "frames_per_pull": FRAMES, "output_rate_hz": OUT_RATE,
       "channels": CHANNELS, "format": FMT, "push_bytes": int(push_bytes), "pull_bytes": int(pull_bytes)}
for model in ("dummy", "noisy"):
    h.model_configure(model)
    for _ in range(3 + -(-STEPS * FRAMES * int(RATE) // int(OUT_RATE) // N_IN)):      # warm-up, and samples for every timed pull
        push()
    for _ in range(3):
        pull()
    torch.cuda.synchronize()
    tp = [timed(push) for _ in range(STEPS)]
    tl = [timed(pull) for _ in range(STEPS)]         # back to back, as tools/rn_pull_timing.py times the RNNoise arm's
    for name, ts, nbytes in (("push", tp, push_bytes), ("pull", tl, pull_bytes)):
        ms = statistics.median(ts)
        res[f"{model}_{name}_ms"] = round(ms, 4)
        res[f"{model}_{name}_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
        res[f"{model}_{name}_gbs"] = round(nbytes / ms / 1e6, 1)
        print(f"{model} {name}: {ms:.4f} ms (min {min(ts):.4f}, max {max(ts):.4f}; {nbytes / 1e6:.1f} MB, {nbytes / ms / 1e6:.0f} GB/s, "
              f"{100 * nbytes / ms / 1e6 / COPY_GBS:.0f} % of the {COPY_GBS:.0f} GB/s copy rate)")
# what the raw samples' way into the playback ring costs: the same dummy push on a handle without one
h2 = DenoiseState(synthetic_weights(0), B, 0)
h2.adapter_configure(RATE, 0.8)
h2.record_configure(REC_RING)
h2.model_configure("dummy")


def push_no_ring():
    assert h2.push_device(x.data_ptr(), N_IN, N_IN, d_out.data_ptr(), N_IN, stream=sp) == N_IN


for _ in range(3):
    push_no_ring()
torch.cuda.synchronize()
ts = [timed(push_no_ring) for _ in range(STEPS)]
res["dummy_push_no_playback_ms"] = round(statistics.median(ts), 4)
res["dummy_push_no_playback_ms_min_max"] = [round(min(ts), 4), round(max(ts), 4)]
print(f"dummy push without a playback ring: {statistics.median(ts):.4f} ms (min {min(ts):.4f}, max {max(ts):.4f})")
print(json.dumps(res))

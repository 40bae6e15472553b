"""Developer tool: the pipeline grain of the RNNoise step settled inside ONE process -- several handles of one library, each
created with its own sub-chunk size, ramp and first-high-pass form (the developer knobs CRISPY_RN_SUB_FRAMES, CRISPY_RN_RAMP
and CRISPY_RN_HP_FIRST of libcrispy_hip_dev.so are read per handle when it is created), timed in interleaved repetitions.
    python tools/grain_sweep.py base=12/3,4,5,7,10 g16=16/3,4,6,9 g24=24/4,6,9 old=12/3,4,5,7,10/0
A row is name=GRAIN/RAMP[/HP_FIRST].  At most four rows per process: a fifth handle's streams share a hardware queue with
the first one's (NOTEBOOK section 28).  Each row runs the BASELINE cfg 2 step (4096 streams x 100 frames, device-resident)
REPS times, each time as STEPS steps enqueued back to back and one synchronize, the way bench.py times its headline (wall
clock per step: a step's first high-pass then stands behind the step before it, as in real use; a single step behind a
synchronize starts on an idle device and spreads three times as wide).  The first row is the yardstick: every other row's
median is given against it in per cent and in units of the first row's own spread (max - min)."""
import os, sys, statistics, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crispy_amd import _native as N, synthetic_weights, synth_audio
from crispy_amd.denoise import DenoiseState
B, T, REPS = int(os.environ.get("B", 4096)), int(os.environ.get("T", 100)), int(os.environ.get("REPS", 15))
STEPS = int(os.environ.get("STEPS", 20))
specs = [a.split("=", 1) for a in sys.argv[1:]]
if not 1 <= len(specs) <= 4:
    sys.exit("one to four rows: name=GRAIN/RAMP[/HP_FIRST]")
L = N.load_library(os.environ.get("CRISPY_HIP_LIB") or os.path.join(ROOT, "crispy_amd", "libcrispy_hip_dev.so"))
w = synthetic_weights(0)
x = synth_audio.batch_torch(B, T, torch.device("cuda:0")); y = torch.empty_like(x)
torch.cuda.synchronize()
KNOBS = ("CRISPY_RN_SUB_FRAMES", "CRISPY_RN_RAMP", "CRISPY_RN_HP_FIRST")
rows = []
for name, spec in specs:
    parts = spec.split("/")
    for k, v in zip(KNOBS, parts + [None] * (3 - len(parts))):
        os.environ.pop(k, None)
        if v:
            os.environ[k] = v
    ds = DenoiseState(w, B, 0, lib=L)
    for _ in range(3):
        ds.process_device(x.data_ptr(), y.data_ptr(), T)
    ds.synchronize()
    rows.append((name, spec, ds, []))
for k in KNOBS:
    os.environ.pop(k, None)
for r in range(REPS):
    order = rows if r % 2 == 0 else rows[::-1]          # no row always runs behind the same neighbour
    for name, spec, ds, ms in order:
        t0 = time.perf_counter()
        for _ in range(STEPS):
            ds.process_device(x.data_ptr(), y.data_ptr(), T)
        ds.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
ref = statistics.median(rows[0][3])
spread = max(rows[0][3]) - min(rows[0][3])
for name, spec, ds, ms in rows:
    m = statistics.median(ms)
    print(f"{name:8s} {spec:22s} step {m:7.3f} ms (min {min(ms):.3f} max {max(ms):.3f})"
          f"  {100 * (m / ref - 1):+5.2f}%  {(m - ref) / spread if spread else 0.:+6.1f} spreads of the first row", flush=True)

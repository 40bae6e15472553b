"""Developer tool: two 4096-stream RNNoise handles driven from two host threads at once, with the first sub-chunk's
high-pass as one deep launch (CRISPY_RN_HP_FIRST=1, the default) and in the split 32-register form (=0) -- the case where
ANOTHER handle's 120-register frame waves are resident when a call's first high-pass starts, so its 80-register waves
have to wait for a SIMD with room.  One process, libcrispy_hip_dev.so, four handles (two per form), the forms alternating;
per repetition both threads enqueue STEPS steps of 100 frames back to back and the wall time until both have drained is
taken.    python tools/two_handle_step.py  -> median ms per step of the pair, per form."""
import os, sys, statistics, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from crispy_amd import _native as N, synthetic_weights, synth_audio
from crispy_amd.denoise import DenoiseState
B, T, REPS, STEPS = int(os.environ.get("B", 4096)), int(os.environ.get("T", 100)), int(os.environ.get("REPS", 9)), int(os.environ.get("STEPS", 5))
L = N.load_library(os.environ.get("CRISPY_HIP_LIB") or os.path.join(ROOT, "crispy_amd", "libcrispy_hip_dev.so"))
w = synthetic_weights(0)
x = synth_audio.batch_torch(B, T, torch.device("cuda:0"))
ys = [torch.empty_like(x) for _ in range(2)]
torch.cuda.synchronize()
pairs = {}
for form in ("1", "0"):
    os.environ["CRISPY_RN_HP_FIRST"] = form
    pairs[form] = [DenoiseState(w, B, 0, lib=L) for _ in range(2)]
os.environ.pop("CRISPY_RN_HP_FIRST", None)


def drive(ds, y, n):
    for _ in range(n):
        ds.process_device(x.data_ptr(), y.data_ptr(), T)
    ds.synchronize()


def run_pair(form, n):
    th = [threading.Thread(target=drive, args=(ds, y, n)) for ds, y in zip(pairs[form], ys)]
    t0 = time.perf_counter()
    for t in th: t.start()
    for t in th: t.join()
    return (time.perf_counter() - t0) * 1e3 / n


for form in pairs:
    run_pair(form, 2)
ms = {form: [] for form in pairs}
for r in range(REPS):
    for form in (("1", "0") if r % 2 == 0 else ("0", "1")):
        ms[form].append(run_pair(form, STEPS))
ref = statistics.median(ms["0"])
for form, what in (("0", "split, 32 registers"), ("1", "one deep launch")):
    m = statistics.median(ms[form])
    print(f"first high-pass {what:22s}: {m:7.3f} ms per step of two handles (min {min(ms[form]):.3f} max {max(ms[form]):.3f})  {100 * (m / ref - 1):+5.2f}%", flush=True)

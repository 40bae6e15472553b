"""Developer tool, needs the GPU: how much of a frame-kernel launch its waves are resident for, from the enter / leave stamps
of the diagnostic build (make -C crispy_amd/csrc prof: counters 14 .. 19 of the profile area, see RN_PROF_DECL in
rn_kernels.hip).  Never quote this build's run time.
    python tools/launch_tail.py [out.json]          (PROF_LIB=... selects another diagnostic build, LIB_NOTE=... names it in the JSON)
The debug buffer goes to the last launch of a call only, so every call here is ONE launch: CRISPY_RN_RAMP=12 and T = 12
(the diagnostic build has the developer knobs compiled in).  B = 4096 streams, WARM calls back to back, then the measured one.
Printed and written as JSON:
  span            latest leave - earliest enter, in ticks of the 100 MHz constant-rate clock
  idle            (launch end - wave leave) / span per wave: mean, quantiles
  by_prio         the same by slot & 3 (the priority a wave holds for the whole launch under the fixed rule), with the
                  mean position of the wave's leave inside the span
  simd_spread     (latest - earliest leave among the waves of one SIMD) / span: mean, quantiles
  cu_spread       the same per CU
  clock_mhz       shader clock inside the launch: d s_memtime / d s_memrealtime x 100 MHz, median over waves"""
import json
import os
import sys

os.environ.setdefault("CRISPY_RN_RAMP", "12")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from crispy_amd import _native as N
N.LIB_PATH = os.environ.get("PROF_LIB") or os.path.join(os.path.dirname(N.LIB_PATH), "libcrispy_hip_prof.so")
from crispy_amd import synthetic_weights, synth_audio
from crispy_amd.denoise import DenoiseState

B, T, WARM = int(os.environ.get("B", 4096)), 12, int(os.environ.get("WARM", 40))
ds = DenoiseState(synthetic_weights(0), B, 0)
ds.debug_capture(True)
x = synth_audio.batch_torch(B, T, torch.device("cuda:0")); y = torch.empty_like(x)
torch.cuda.synchronize()
for _ in range(WARM + 1):
    ds.process_device(x.data_ptr(), y.data_ptr(), T)
ds.synchronize()
c = np.stack([ds.debug_read(b)[3824 + 14:3824 + 20].view(np.uint32) for b in range(B)]).astype(np.int64)
enter, leave, m0, m1, hw, xcc = c.T
def rel(v):       # the counters are the low 32 bits: differences to wave 0's enter, wrapped into [-2^31, 2^31)
    d = (v - c[0, 0]) & 0xffffffff
    return np.where(d >= 1 << 31, d - (1 << 32), d)


enter, leave = rel(enter), rel(leave)
first = enter.min()
enter, leave = enter - first, leave - first
span = int(leave.max())
idle = (span - leave) / span
slot, simd, cu, sh, se = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
cu_key = ((xcc & 15) << 8) | (se << 5) | (sh << 4) | cu
simd_key = (cu_key << 2) | simd


def dist(v):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()), "p10": float(np.quantile(v, .1)), "p50": float(np.quantile(v, .5)),
            "p90": float(np.quantile(v, .9)), "max": float(v.max())}


def spread(key):
    return dist([(leave[key == k].max() - leave[key == k].min()) / span for k in np.unique(key)])


res = {"lib": os.environ.get("LIB_NOTE") or os.path.basename(N.LIB_PATH),"streams": B, "frames": T, "warm_calls": WARM, "span_ticks": span, "span_us": span / 100.0,
       "enter_spread": float((enter.max() - enter.min()) / span), "resident": dist((leave - enter) / span), "idle": dist(idle),
       "by_prio": {str(p): {"waves": int((slot & 3 == p).sum()), "idle": dist(idle[slot & 3 == p]),
                            "leave_at": float((leave[slot & 3 == p] / span).mean())} for p in range(4)},
       "slots_seen": sorted(int(s) for s in np.unique(slot)), "simds": int(len(np.unique(simd_key))), "cus": int(len(np.unique(cu_key))),
       "waves_per_simd": dist(np.unique(simd_key, return_counts=True)[1]),
       "simd_spread": spread(simd_key), "cu_spread": spread(cu_key),
       "clock_mhz": float(np.median(((m1 - m0) & 0xffffffff) / np.maximum(1, (c[:, 1] - c[:, 0]) & 0xffffffff) * 100.0))}
print(json.dumps(res, indent=1))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")

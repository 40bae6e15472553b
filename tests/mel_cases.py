"""Signals, references and the error statistic of the log-mel precision tests (tests/test_mel_cases.py on the CPU,
tests/test_gpu_logmel_precision.py on the GPU), each defined once.  No GPU is needed to import or run anything here.

Two references of the values BEFORE the normalisation (log10 of the filter sums, crispy_amd/csrc/mel_kernels.hip):

    power(x, filters)      float64 throughout                       -> M [n_mel, T], Tp [T], r64 [n_mel, T]
    power_f32(x, filters)  a float32 front end as a kernel would    -> M32 (float64 sums of f32 powers), r32 (float32)
                           build it: f32 window table, f32 rfft,
                           f32 power, float64 filter sums, log10 in
                           float64 rounded once

over the frames that touch audio, T = live_frames(n); every later frame of a clip is zeros only and is the floor, -10.
Framing is the kernel's: frame t starts at sample 160 t - 200, a negative index s reads x[-s], an index >= n reads 0 --
for n < 201 too, where the reflection runs past the clip's end.

The statistic (`stat`): over the live elements, M >= 2e-10,  D = max |r - r64| sqrt(min(1, M / Tp)),  Tp[t] = sum_k P[t, k]
the frame's whole power.  An f32 transform promises a bin an absolute error proportional to the frame's amplitude, so a
filter sum's relative error -- its error in log10 -- grows as sqrt(Tp / M): the weight takes that out, and D of a correct
f32 front end is a few 1e-8 whatever the signal.  The GPU is held to FACTOR x D of `power_f32` on the same clip.
Elements with M <= 0.5e-10 must be exactly -10; those in between lie too close to the floor's switch at 1e-10 to be
either, and `band_share` bounds how many a case may have (BAND_CAP_LONG / BAND_CAP_SHORT)."""
from __future__ import annotations

import numpy as np

from crispy_amd.mel_filters import whisper_mel_filters

FACTOR = 4.0
FLOOR = -10.0
LIVE_MIN = 2e-10            # M >= this: compared under the statistic
DEAD_MAX = 0.5e-10          # M <= this: exactly -10
BAND_CAP_LONG = 0.01        # share of a clip's elements between the two, clips of >= 64 frames
BAND_CAP_SHORT = 0.04       # ... shorter clips
QUIET_MAX = -2.25           # quiet scaling: r64.max() below this, so that max - 8 < -10 and nothing clamps
MEL_FW_MAX = 1024           # crispy_amd/csrc/asr_common.h
LENGTHS = (1, 100, 199, 200, 201, 399, 401, 9880, 9881, 10040, 10041, 16000, 40123)
N_LONG = 485000
IMPULSE_OFFSETS = (1, 2, 199, 200, 201, 398, 399)
HANN64 = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(400) / 400.0))


def live_frames(n: int) -> int:
    """Frames whose 400 samples (from 160 t - 200) reach the clip."""
    return (n + 200 + 159) // 160


def frames(x: np.ndarray) -> np.ndarray:
    """[live_frames(n), 400] float32: the samples every frame sees, before the window."""
    x = np.asarray(x, dtype=np.float32)
    n = x.size
    s = 160 * np.arange(live_frames(n))[:, None] - 200 + np.arange(400)[None, :]
    s = np.abs(s)
    return np.where(s < n, x[np.minimum(s, n - 1)], np.float32(0.0)).astype(np.float32)


def power(x: np.ndarray, filters: np.ndarray):
    """The float64 reference -> (M [n_mel, T], Tp [T], r64 [n_mel, T])."""
    F = np.asarray(filters, dtype=np.float32).astype(np.float64)
    P = np.abs(np.fft.rfft(frames(x).astype(np.float64) * HANN64, axis=1)) ** 2
    M = (P @ F.T).T
    return M, P.sum(1), np.log10(np.maximum(M, 1e-10))


def bin_gains(rms: float, seed: int = 99) -> np.ndarray:
    """A faulty table for the teeth test: every FFT bin's gain off by `rms` rms."""
    return (1.0 + rms * np.random.default_rng(seed).standard_normal(201)).astype(np.float64)


def power_f32(x: np.ndarray, filters: np.ndarray, gains: np.ndarray | None = None):
    """The float32 reference -> (M32 [n_mel, T] float64, r32 [n_mel, T] float32)."""
    import torch
    F = np.asarray(filters, dtype=np.float32).astype(np.float64)
    xw = torch.from_numpy(frames(x)) * torch.from_numpy(HANN64.astype(np.float32))
    X = torch.fft.rfft(xw, dim=1)
    if gains is not None:
        X = X * torch.from_numpy(gains.astype(np.float32))
    P = (X.real * X.real + X.imag * X.imag).numpy()
    assert P.dtype == np.float32
    M = (P.astype(np.float64) @ F.T).T
    r = np.where(M > 1e-10, np.log10(np.maximum(M, 1e-300)), FLOOR).astype(np.float32)
    return M, r


def weight(M: np.ndarray, Tp: np.ndarray) -> np.ndarray:
    return np.sqrt(np.minimum(1.0, M / np.maximum(Tp, 1e-300)[None, :]))


def stat(r: np.ndarray, M: np.ndarray, Tp: np.ndarray, r64: np.ndarray, per_row: bool = False):
    """D over the live elements (0.0 if there is none); per_row: the maximum of every filter row, [n_mel]."""
    live = M >= LIVE_MIN
    d = np.where(live, np.abs(np.asarray(r, dtype=np.float64) - r64) * weight(M, Tp), 0.0)
    return d.max(1) if per_row else float(d.max())


def floor_ok(r: np.ndarray, M: np.ndarray) -> bool:
    """Every element with M <= 0.5e-10 is exactly -10."""
    return bool(np.all(np.asarray(r)[M <= DEAD_MAX] == np.float32(FLOOR)))


def band_share(M: np.ndarray) -> float:
    return float(((M > DEAD_MAX) & (M < LIVE_MIN)).mean())


def band_cap(n: int) -> float:
    return BAND_CAP_LONG if live_frames(n) >= 64 else BAND_CAP_SHORT


def quiet(x: np.ndarray, filters: np.ndarray):
    """-> (x 2^k as float32, k): k the largest integer with r64.max() < QUIET_MAX.  The scaling is exact in every
    arithmetic (M scales by 2^2k), so one float64 pass gives k; the result is checked."""
    x = np.asarray(x, dtype=np.float32)
    top = float(power(x, filters)[2].max())
    if top <= FLOOR:                                   # silence: nothing to scale
        return x, 0
    k = int(np.floor((QUIET_MAX - top) / (2.0 * np.log10(2.0))))
    for k in (k + 1, k, k - 1):                        # the estimate may sit one off at a rounding boundary
        xq = np.ldexp(x, k).astype(np.float32)
        if power(xq, filters)[2].max() < QUIET_MAX:
            break
    assert power(xq, filters)[2].max() < QUIET_MAX <= power(np.ldexp(xq, 1), filters)[2].max()
    assert np.array_equal(np.ldexp(xq.astype(np.float64), -k), x.astype(np.float64)), "the scaling left f32's normal range"
    return xq, k


def out_to_raw(out: np.ndarray) -> np.ndarray:
    """The frame kernel's floats from the public output of a quiet clip: for every f32 raw in [-10, -2), (raw + 4) / 4
    is exact in f32 (tests/test_mel_cases.py), and nothing clamps."""
    return (4.0 * np.asarray(out, dtype=np.float64) - 4.0).astype(np.float32)


def ulp32(v) -> np.ndarray:
    """Spacing of float32 in the binade of |v| (float64 in and out)."""
    e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))[1]
    return np.ldexp(1.0, np.maximum(e - 24, -149))


# ---- signals ----------------------------------------------------------------------------------------------------------
def signal(seed: int, n: int) -> np.ndarray:
    """White uniform noise at 0.25 plus three chirps between 100 and 7000 Hz at 0.15 each."""
    rng = np.random.default_rng(4000 + seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = 0.25 * rng.uniform(-1.0, 1.0, n)
    for _ in range(3):
        f0, f1 = rng.uniform(100.0, 7000.0, 2)
        x += 0.15 * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / max(t[-1], 1e-3)) + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)


SEEDS = {}      # (what, n) -> seed, where the first seed broke the band cap (none does today)


def edge_clip(n: int) -> np.ndarray:
    return signal(SEEDS.get(("edge", n), n % 1000), n)


def identity_bank(first_bin: int) -> np.ndarray:
    """128 rows, row m = 1.0 at bin first_bin + m: the power spectrum itself comes out."""
    F = np.zeros((128, 201), np.float32)
    F[np.arange(128), first_bin + np.arange(128)] = 1.0
    return F


IMPULSE_FRAME0, IMPULSE_STEP = 4, 5     # impulse i sits in frame 4 + 5 i: no frame sees two of them


def impulse_clip() -> np.ndarray:
    """One sample at offset j of an interior frame for every j of IMPULSE_OFFSETS.  An impulse at offset j of frame t is
    also seen by frame t - 1 at j + 160 and / or frame t + 1 at j - 160, all with a flat spectrum of power (a hann[j'])^2:
    after the quiet scaling 1.5e-11 (offsets 1 and 399: on the floor), 2.4e-10 (2 and 398: live) and 3e-5 and more."""
    n = 160 * (IMPULSE_FRAME0 + IMPULSE_STEP * len(IMPULSE_OFFSETS))
    x = np.zeros(n, np.float32)
    for i, j in enumerate(IMPULSE_OFFSETS):
        x[160 * (IMPULSE_FRAME0 + IMPULSE_STEP * i) - 200 + j] = 0.5
    return x


def tone_clips(n_samples: int = 1200) -> np.ndarray:
    """[201, n_samples]: clip k = 0.5 cos(2 pi k n / 400): its power sits in bins k - 1, k, k + 1 of the frames inside."""
    n = np.arange(n_samples, dtype=np.float64)
    return (0.5 * np.cos(2 * np.pi * np.arange(201)[:, None] * n[None, :] / 400.0)).astype(np.float32)


def limits_bank() -> np.ndarray:
    """128 rows at the sparse table's limits: row 0 spans exactly 64 taps from bin 0; row 1 is all zero; row 2 has zeros
    inside its span; row 127 ends at bin 200; the spans of all rows together are exactly MEL_FW_MAX taps."""
    rng = np.random.default_rng(17)
    F = np.zeros((128, 201), np.float32)
    F[0, :64] = rng.uniform(0.005, 0.03, 64)
    F[2, 100:111] = rng.uniform(0.005, 0.03, 11)
    F[2, [102, 105, 106]] = 0.0
    rows = list(range(3, 128))
    left = MEL_FW_MAX - 64 - 11
    lens = [left // len(rows) + (1 if i < left % len(rows) else 0) for i in range(len(rows))]
    for i, (m, ln) in enumerate(zip(rows, lens)):
        k0 = int(round(i * (201 - ln) / (len(rows) - 1)))
        F[m, k0:k0 + ln] = rng.uniform(0.005, 0.03, ln)
    assert bank_taps(F) == (MEL_FW_MAX, 64) and F[127, 200] != 0 and F[3, 0] != 0
    return F


def bank_taps(F: np.ndarray):
    """(taps of the whole bank, longest row) as crispy_mel_create counts them: a row's span from its first to its last
    non-zero weight."""
    spans = [int(nz[-1] - nz[0] + 1) if nz.size else 0 for nz in (np.flatnonzero(r) for r in F)]
    return sum(spans), max(spans)


def bank(name: str) -> np.ndarray:
    if name in ("80", "128"):
        return whisper_mel_filters(int(name))
    return {"id0": lambda: identity_bank(0), "id73": lambda: identity_bank(73), "limits": limits_bank}[name]()


def numeric_cases():
    """(case name, bank name, clip before the quiet scaling) of every case the GPU tests hold to FACTOR x D of the float32
    reference: (a) the edge lengths and the long clip, (b) the identity banks, (c) the tones."""
    for b in ("80", "128"):
        for n in LENGTHS + (N_LONG,):
            yield f"a/{b}/{n}", b, edge_clip(n)
    for b in ("id0", "id73"):
        yield f"b/{b}/signal", b, signal(5, 8000)
        yield f"b/{b}/impulses", b, impulse_clip()
    tones = tone_clips()
    for b in ("80", "128", "limits"):
        for k in range(201):
            yield f"c/{b}/{k}", b, tones[k]


class Ref:
    """Both references of one clip as it is given to the GPU, and D of the float32 one."""

    def __init__(self, x: np.ndarray, filters: np.ndarray):
        self.n = int(np.asarray(x).size)
        self.M, self.Tp, self.r64 = power(x, filters)
        self.M32, self.r32 = power_f32(x, filters)
        self.D32 = stat(self.r32, self.M, self.Tp, self.r64)
        self.T = self.M.shape[1]

    def D(self, r, per_row: bool = False):
        return stat(r, self.M, self.Tp, self.r64, per_row)


# ---- the clip maximum --------------------------------------------------------------------------------------------------
BURST_N = 11000                                    # 70 live frames: tile 0 and six frames of tile 1
BURST_FRAMES = {"frame 0": 0, "frame 3 of a 4-frame group": 3, "last frame of a wave's 16": 15, "last frame of tile 0": 63,
                "first frame of tile 1": 64, "clip end": None}


def burst_clip(where: str, hz: float, seed: int = 0) -> tuple[np.ndarray, int]:
    """-> (clip, frame that holds the clip's maximum).  The noise-plus-chirp signal at -40 dB with a 5 ms tone (80 samples,
    amplitude 0.5) centred on frame t's window, samples [160 t - 40, 160 t + 40) -- frame 0: [0, 40), which the reflection
    completes.  "clip end": the tone is the clip's last 80 samples, all inside the last live frame; that frame sees them
    under the window's rising edge only (a last live frame sees at most 160 samples), so the frame that holds the maximum
    is the one before it, the last but one live frame."""
    x = 0.01 * signal(900 + seed, BURST_N).astype(np.float64)
    t = BURST_FRAMES[where]
    if t is None:
        a, b = BURST_N - 80, BURST_N
        t = live_frames(BURST_N) - 2
        assert 160 * (t + 1) - 200 <= a, "the tone lies in the last live frame"
    else:
        a, b = max(0, 160 * t - 40), 160 * t + 40
    x[a:b] += 0.5 * np.cos(2 * np.pi * hz * (np.arange(a, b) - 160 * t) / 16000.0)
    return x.astype(np.float32), t


# ---- log10_to_float ----------------------------------------------------------------------------------------------------
def log10_inputs() -> tuple[np.ndarray, np.ndarray]:
    """-> (all inputs, sorted float64; the 10^5 values within 2^-10 of 1.0)."""
    rng = np.random.default_rng(23)
    parts = []
    exps = np.arange(-34, 41)
    mant = (np.arange(1 << 16, dtype=np.uint64) << np.uint64(36)) | rng.integers(0, 1 << 36, 1 << 16, dtype=np.uint64)
    for e in exps:                                 # 2^16 evenly spaced mantissas with random low bits, per exponent
        parts.append(((np.uint64(1023 + e) << np.uint64(52)) | mant).view(np.float64))
    r2 = np.float64(np.sqrt(2.0)).view(np.uint64) & np.uint64((1 << 52) - 1)
    around = (r2 + np.arange(-64, 65).astype(np.int64).astype(np.uint64)) & np.uint64((1 << 52) - 1)
    for e in exps:                                 # the m > sqrt 2 switch
        parts.append(((np.uint64(1023 + e) << np.uint64(52)) | around).view(np.float64))
    p2 = np.ldexp(1.0, np.arange(-33, 41))
    parts += [p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf)]
    f = np.float64(1e-10)
    near = [f]
    for _ in range(8):
        near = [np.nextafter(near[0], 0.0)] + near + [np.nextafter(near[-1], 1.0)]
    parts.append(np.array(near + [0.0, 1e-300, 0.5e-10, 0.99e-10, 1.01e-10, 2e-10]))
    parts.append(10.0 ** rng.uniform(-10.0, 6.0, 1000000))
    near1 = 1.0 + rng.uniform(-1.0, 1.0, 100000) * 2.0 ** -10
    parts.append(near1)
    s = np.sort(np.concatenate(parts))
    return s, near1

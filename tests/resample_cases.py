"""Edge cases of the 48 -> 16 kHz resampler (crispy_resampler_process_device): inputs and float64 expectations.

Pure numpy and importable without a GPU: tests/test_oracle_resample.py asserts this builder's own conditions on the CPU,
tests/test_gpu_resampler_edges.py runs the cases.  Run as a program it puts one named case set through the GPU and writes
every case's whole output buffer (padding included) to an .npz:

    python -m tests.resample_cases SET OUT.npz

which is how a case reaches the 256-row GEMM tile: CRISPY_ASR_TILE_ROWS is read once per process, so the caller starts a
fresh process with it set.

A case is `batch` streams of `n_in` valid samples in rows of `in_stride` floats.  The f16-pair form of the resampler
(the production form) serves an even output stride on an 8-byte aligned base, the f32 form every other layout: a case
picks its form through the parity of `out_stride`.  In the pair form a GEMM row is a window [previous block | block] of a
stream and the last window of every stream but the last is computed and dropped, so the row count of the GEMM is
M = batch * (n_blk + 1) - 1; gemm_hd_kernel (128-row tiles) runs below 1024 rows, gemm_hd2_kernel (192 | 256) from there.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import resample_oracle as RO  # noqa: E402

FFT_IN, FFT_OUT, CHUNK = RO.FFT_IN, RO.FFT_OUT, RO.CHUNK
SENTINEL = np.float32(-1234.5)
HD2_FROM_ROWS = 1024                       # gemm_hh: the 192 | 256-row kernel from this row count up


def out_len(n_in: int) -> int:
    return (-(-n_in // CHUNK) * CHUNK) // FFT_IN * FFT_OUT if n_in > 0 else 0


def pair_rows(batch: int, n_in: int) -> int:
    """M of the pair form's GEMM."""
    return batch * (out_len(n_in) // FFT_OUT + 1) - 1


@dataclass
class Case:
    name: str
    x: np.ndarray                          # float32 [batch][in_stride], as handed to the device
    n_in: int
    form: str                              # "pair" | "f32"
    out_pad: int                           # out_stride = out_len + out_pad
    want: np.ndarray                       # float64 [batch][out_len]; NaN where the output has to be NaN
    bar: object                            # absolute, on every finite expectation: one float, or one per stream
    mode: int = 0                          # wav_s16 of the API: 0 | 1 clamp | 2 clamp + s16 truncation
    scale: float = 1.0
    dense: bool = False                    # every stream is broadband signal: the expectation must not be near zero
    exact_zero: tuple = ()                 # streams that must come out as 0.0 exactly
    rows: int = field(init=False)          # M of the pair form

    def __post_init__(self):
        assert self.x.dtype == np.float32 and self.x.ndim == 2 and self.x.shape[1] >= self.n_in
        assert self.form in ("pair", "f32") and (self.out_stride % 2 == 0) == (self.form == "pair")
        assert self.want.shape == (self.batch, self.out_len) and self.want.dtype == np.float64
        self.rows = pair_rows(self.batch, self.n_in)

    @property
    def batch(self) -> int:
        return self.x.shape[0]

    @property
    def out_len(self) -> int:
        return out_len(self.n_in)

    @property
    def out_stride(self) -> int:
        return self.out_len + self.out_pad


def dense_bar(want: np.ndarray) -> np.ndarray:
    """The project's bar on an oracle comparison of the resampler (tests/test_gpu_pipeline.py): per stream, 1e-5 of
    max(1, the stream's peak)."""
    if not want.size:
        return np.full(want.shape[0], 1e-5)
    return 1e-5 * np.maximum(1.0, np.nanmax(np.abs(want), axis=1))


@lru_cache(maxsize=None)
def operator_g() -> np.ndarray:
    g = RO.operator_g()
    g.setflags(write=False)
    return g


def oracle_rows(x: np.ndarray, n_in: int) -> np.ndarray:
    return np.stack([RO.resample_48k_to_16k_f64(r[:n_in]) for r in x]) if out_len(n_in) else np.zeros((x.shape[0], 0))


# ---------------------------------------------------------------------------------------------------------------------
# A. impulse responses at operator precision
# ---------------------------------------------------------------------------------------------------------------------
IMPULSE_N_IN = 4096                        # 3 blocks; samples from 3078 on are never flushed
IMPULSE_POS = (0, 1, 341, 342, 512, 1023, 1024, 1025, 1026, 1027, 2051, 2052, 3077, 3078, 4095)
IMPULSE_BAR = 2.0 ** -24                   # |w - (w_hi + w_lo)| <= 2^-25, the f32 sum rounds by <= 2^-24 x 0.33 (see the GPU test)
# streams (the 15 positions repeated) -> M = 4 streams - 1: 59 rows = one 128-row tile of gemm_hd; 1079 rows = gemm_hd2
IMPULSE_REPEATS = {"hd": 1, "hd2": 18}


def impulse_expected(pos: int) -> np.ndarray:
    """The 1026 outputs of a unit impulse at `pos`, straight from the circulant: the own-block rows and the overlap rows."""
    g = operator_g()
    n_blk = out_len(IMPULSE_N_IN) // FFT_OUT
    y = np.zeros(n_blk * FFT_OUT)
    b, j = divmod(pos, FFT_IN)
    if b < n_blk:
        col = g[(3 * np.arange(2 * FFT_OUT) - j) % (2 * FFT_IN)]
        y[b * FFT_OUT:(b + 1) * FFT_OUT] = col[:FFT_OUT]
        if b + 1 < n_blk:
            y[(b + 1) * FFT_OUT:(b + 2) * FFT_OUT] = col[FFT_OUT:]
    return y


@lru_cache(maxsize=None)
def impulse_case(kernel: str, form: str) -> Case:
    rep = IMPULSE_REPEATS[kernel]
    pos = IMPULSE_POS * rep
    x = np.zeros((len(pos), IMPULSE_N_IN), np.float32)
    x[np.arange(len(pos)), pos] = 1.0
    want = np.stack([impulse_expected(p) for p in IMPULSE_POS] * rep)
    zero = tuple(i for i, p in enumerate(pos) if p >= out_len(IMPULSE_N_IN) // FFT_OUT * FFT_IN)
    return Case(f"impulse_{kernel}_{form}", x, IMPULSE_N_IN, form, 0 if form == "pair" else 1, want, IMPULSE_BAR, exact_zero=zero)


# ---------------------------------------------------------------------------------------------------------------------
# B. row-count edges: dense noise, pair form
# ---------------------------------------------------------------------------------------------------------------------
#            n_in  batch  M
ROW_TABLE = ((2048, 1, 1), (2048, 64, 127), (2048, 65, 129), (2048, 512, 1023), (2048, 513, 1025),
             (3072, 342, 1025), (3072, 171, 512),
             (4096, 97, 387), (4096, 385, 1539))


def noise(seed: int, n: int, rms: float = 0.1) -> np.ndarray:
    return (rms * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@lru_cache(maxsize=None)
def rows_case(n_in: int, batch: int) -> Case:
    x = np.stack([noise(1000 * n_in + b, n_in) for b in range(batch)])
    want = oracle_rows(x, n_in)
    return Case(f"rows_{n_in}x{batch}", x, n_in, "pair", 0, want, dense_bar(want), dense=True)


# ---------------------------------------------------------------------------------------------------------------------
# C. length and stride edges
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 1023, 1024, 1025, 1026, 1027, 2048, 2049, 2052, 3078, 3079)
IN_PAD = 37                                # floats behind the valid samples of every row: NaN


def length_case(n_in: int, form: str) -> Case:
    x = np.full((3, n_in + IN_PAD), np.nan, np.float32)
    for b in range(3):
        x[b, :n_in] = noise(7000 + 10 * n_in + b, n_in)
    want = oracle_rows(x, n_in)
    return Case(f"len_{n_in}_{form}", x, n_in, form, 2 if form == "pair" else 3, want, dense_bar(want), dense=out_len(n_in) > 0)


# ---------------------------------------------------------------------------------------------------------------------
# D. hand-off modes on crafted values
# ---------------------------------------------------------------------------------------------------------------------
HANDOFF_N = 2048
NAN_AT = FFT_IN + 500                      # block 1 of the second stream of the NaN cases


def crafted_values() -> np.ndarray:
    one = np.float32(1.0)
    v = [0.0, -0.0, 1.0, -1.0, np.nextafter(one, np.float32(0)), -np.nextafter(one, np.float32(0)),
         np.nextafter(one, np.float32(2)), -np.nextafter(one, np.float32(2)), 2.0, -2.0, 1e30, -1e30, np.inf, -np.inf,
         1e-5, -1e-5]
    for k in (1, 2, 16383, 16384, 32766, 32767):
        c = np.float32(k) / np.float32(32767.0)
        for w in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(2))):
            v += [w, -w]
    return np.array(v, np.float32)


@lru_cache(maxsize=None)
def crafted_stream() -> np.ndarray:
    """2048 samples: noise (rms 0.1) with the crafted values at seeded places inside the first block (the 1026 samples a
    2048-sample stream flushes)."""
    x = noise(31, HANDOFF_N)
    v = crafted_values()
    at = np.random.default_rng(32).choice(FFT_IN, v.size, replace=False)
    x[at] = v
    return x


def handoff_source(x: np.ndarray, mode: int) -> np.ndarray:
    """What the operator sees of f32 samples x (already scaled): the reference's hand-off in f32 numpy.  Mode 1 is
    `f32::clamp` (audio.rs:272: a NaN stays), mode 2 the s16 WAV (recording.rs:109-110: a NaN becomes 0)."""
    if mode == 1:
        return np.clip(x, np.float32(-1.0), np.float32(1.0))
    if mode == 2:
        return RO.wav_s16_roundtrip(x)
    return x


def handoff_case(mode: int, premultiplied: bool, form: str) -> Case:
    x = crafted_stream()[None, :]
    want = oracle_rows(handoff_source(x, mode), HANDOFF_N)
    with np.errstate(over="ignore"):
        dev = x * np.float32(32768.0) if premultiplied else x           # exact: a power of two (1e30 stays finite)
    assert not premultiplied or np.array_equal(dev * np.float32(1.0 / 32768.0), x)
    return Case(f"handoff_m{mode}_{'s' if premultiplied else 'u'}_{form}", dev.copy(), HANDOFF_N, form,
                0 if form == "pair" else 1, want, dense_bar(want), mode=mode, scale=1.0 / 32768.0 if premultiplied else 1.0,
                dense=True)


def nan_case(mode: int, form: str) -> Case:
    """4096 samples (3 blocks).  Stream 0: the crafted stream continued by noise (plain noise in mode 0, which has no clamp
    for the non-finite crafted values); stream 1: noise with one NaN in block 1.  Mode 2 reads the NaN as 0; modes 0 and 1
    carry it into everything block 1 feeds: its own 342 outputs and the 342 of the next block."""
    n = 4096
    x = np.stack([noise(41, n), noise(42, n)])
    if mode:
        x[0, :HANDOFF_N] = crafted_stream()
    x[1, NAN_AT] = np.nan
    src = handoff_source(x, mode)
    finite = np.where(np.isnan(src), np.float32(0.0), src)
    want = oracle_rows(finite, n)
    if mode != 2:
        b = NAN_AT // FFT_IN
        want[1, b * FFT_OUT:(b + 2) * FFT_OUT] = np.nan
    return Case(f"nan_m{mode}_{form}", x, n, form, 0 if form == "pair" else 1, want, dense_bar(want), mode=mode, dense=True)


# ---------------------------------------------------------------------------------------------------------------------
# E. quiet audio
# ---------------------------------------------------------------------------------------------------------------------
QUIET_N = 4096
# gain on the +-1 LSB signal -> what becomes of x = hi + lo in f16:
#   1            +-2^-15: an exact subnormal half, lo = 0
#   2^-6         +-2^-21 = 8 subnormal steps: still exact, lo = 0
#   0.7 x 2^-6   5.6 steps: hi rounds to 6, the rest (0.4 step < 2^-25) is below half a step of lo and is lost
QUIET_GAINS = {"lsb": 1.0, "lsb_2m6": 2.0 ** -6, "lsb_0p7_2m6": 0.7 * 2.0 ** -6}


def quiet_case(which: str, form: str) -> Case:
    rng = np.random.default_rng(51)
    x = (rng.integers(-1, 2, (2, QUIET_N)).astype(np.float32) / np.float32(32768.0) * np.float32(QUIET_GAINS[which]))
    want = oracle_rows(x, QUIET_N)
    if which == "lsb":
        bar = 1e-4 * float(np.abs(want).max())             # of the reference's own peak
    else:
        bar = 2.0 ** -25 * float(np.abs(operator_g()).sum())   # <= 2^-25 lost per sample, through sum |g|
    return Case(f"quiet_{which}_{form}", x, QUIET_N, form, 0 if form == "pair" else 1, want, bar)


# ---------------------------------------------------------------------------------------------------------------------
# case sets
# ---------------------------------------------------------------------------------------------------------------------
def _impulse():
    return [impulse_case(k, f) for k in ("hd", "hd2") for f in ("pair", "f32")]


def _rows():
    return [rows_case(n, b) for n, b, _ in ROW_TABLE]


def _lengths():
    return [length_case(n, f) for n in LENGTHS for f in ("pair", "f32")]


def _handoff():
    return ([handoff_case(m, s, f) for m in (1, 2) for s in (False, True) for f in ("pair", "f32")]
            + [nan_case(m, f) for m in (0, 1, 2) for f in ("pair", "f32")])


def _quiet():
    return [quiet_case(w, f) for w in QUIET_GAINS for f in ("pair", "f32")]


def _tile():
    """What a process with a pinned tile height runs: every pair-form case that reaches gemm_hd2_kernel, and the 3-block
    row cases whole."""
    return ([impulse_case("hd2", "pair")]
            + [rows_case(n, b) for n, b, m in ROW_TABLE if m >= HD2_FROM_ROWS or n == 4096])


SETS = {"impulse": _impulse, "rows": _rows, "lengths": _lengths, "handoff": _handoff, "quiet": _quiet, "tile": _tile}


@lru_cache(maxsize=None)
def case_set(name: str) -> tuple:
    return tuple(SETS[name]())


def run_cases(cases) -> dict:
    """Every case through one resampler handle on the current GPU: name -> the whole output buffer [batch][out_stride],
    prefilled with SENTINEL.  A call that fails raises."""
    import torch

    from crispy_amd.pipeline import Resampler48to16
    rs = Resampler48to16()
    outs = {}
    try:
        for c in cases:
            d_in = torch.from_numpy(c.x).cuda()
            d_out = torch.full((c.batch, c.out_stride), float(SENTINEL), device="cuda")
            assert d_out.data_ptr() % 8 == 0
            torch.cuda.synchronize()
            rs.process_device(d_in.data_ptr(), c.x.shape[1], c.n_in, c.batch, d_out.data_ptr(), c.out_stride,
                              scale=c.scale, handoff=c.mode)
            rs.synchronize()
            outs[c.name] = d_out.cpu().numpy()
    finally:
        rs.close()
    return outs


def check(c: Case, buf: np.ndarray) -> dict:
    """Asserts everything a case promises of its output buffer; returns the figures worth printing."""
    assert buf.shape == (c.batch, c.out_stride) and buf.dtype == np.float32, (c.name, buf.shape)
    assert np.all(buf[:, c.out_len:] == SENTINEL), (c.name, "written behind the rows")
    got = buf[:, :c.out_len].astype(np.float64)
    nan = np.isnan(c.want)
    assert np.array_equal(np.isnan(got), nan) and np.all(np.isfinite(got[~nan])), (c.name, "NaN / inf where none belongs, or none where one does")
    for b in c.exact_zero:
        assert np.all(got[b] == 0.0), (c.name, b, "a never-flushed sample reached the output")
    err = np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, c.want))
    bar = np.broadcast_to(np.asarray(c.bar, np.float64).reshape(-1, 1), err.shape)
    fig = {"case": c.name, "rows": c.rows, "worst": float(err.max()) if err.size else 0.0, "bar": float(bar.min()) if bar.size else 0.0,
           "rms": float(np.sqrt(np.mean(c.want[~nan] ** 2))) if (~nan).any() else 0.0}
    assert np.all(err <= bar), fig
    return fig


def main(argv) -> int:
    name, path = argv
    outs = run_cases(case_set(name))
    np.savez(path, **outs)
    print(f"{name}: {len(outs)} cases, CRISPY_ASR_TILE_ROWS={os.environ.get('CRISPY_ASR_TILE_ROWS', '')}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

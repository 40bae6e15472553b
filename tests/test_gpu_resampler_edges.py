"""GPU tests of the 48 -> 16 kHz resampler (crispy_resampler_process_device) where one absolute bar on speech cannot look:
the operator coefficient by coefficient, every GEMM kernel the pair form can take, block-count / length / stride edges,
the hand-off modes on crafted samples, and audio of one LSB.  Cases and float64 expectations: tests/resample_cases.py.

The pair form's GEMM (whisper_enc_f16.hip: gemm_hh, EPI_F32 with row groups and k-segments) is gemm_hd_kernel below 1024
rows and gemm_hd2_kernel on 192- or 256-row tiles from there; production (186 streams x 1405 slots) takes the 256-row
tile, every small size takes 192 by the cost rule.  CRISPY_ASR_TILE_ROWS pins the height, once per process: the `tile`
case set runs in two child processes (256, 192), started one after the other by one module fixture."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def RC():
    from tests import resample_cases
    return resample_cases


@pytest.fixture(scope="module")
def ran(RC):
    """name of a case set -> its outputs in this process (the tile height the cost rule picks), each set run once."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = RC.run_cases(RC.case_set(name))
        return done[name]
    return get


@pytest.fixture(scope="module")
def tile_runs(RC, tmp_path_factory):
    """The `tile` set in a process of its own per pinned tile height: {"256": outputs | error text, "192": ...}.  At most
    two children, each under its own time limit; after one that failed, none is started."""
    out = {}
    d = tmp_path_factory.mktemp("rs_tile")
    for rows in ("256", "192"):
        if any(isinstance(v, str) for v in out.values()):
            out[rows] = "not started: the child before it failed"
            continue
        path = str(d / f"tile{rows}.npz")
        env = dict(os.environ, CRISPY_ASR_TILE_ROWS=rows)
        try:
            r = subprocess.run([sys.executable, "-m", "tests.resample_cases", "tile", path], cwd=ROOT, env=env,
                               capture_output=True, text=True, timeout=180)
        except subprocess.TimeoutExpired as e:
            out[rows] = f"time limit: {e}"
            continue
        if r.returncode != 0 or not os.path.exists(path):
            out[rows] = f"exit {r.returncode}: {r.stderr[-2000:]}"
            continue
        with np.load(path) as z:
            out[rows] = {k: z[k] for k in z.files}
    return out


def show(tag, figs):
    for f in figs:
        print(f"resampler {tag} {f['case']}: M = {f['rows']}, worst error {f['worst']:.3e} (bar {f['bar']:.3e}), reference rms {f['rms']:.3e}")


def check_all(RC, tag, cases, outs):
    """Every case checked and printed before the first failure is raised."""
    figs, failed = [], []
    for c in cases:
        try:
            figs.append(RC.check(c, outs[c.name]))
        except AssertionError as e:
            failed.append(e)
            print(f"resampler {tag} {c.name}: FAILED {e}")
    show(tag, figs)
    assert not failed, failed[0]


def test_impulse_responses_at_operator_precision(RC, ran):
    """A. One unit impulse per stream (mode 0, scale 1, 4096 samples = 3 output blocks), expected output straight from
    the float64 circulant g, so own-block rows and overlap rows are both checked, coefficient by coefficient; impulses at
    3078 and 4095 are never flushed and must give exactly 0.0.  Bar 2^-24 absolute: x_hi = 1 and x_lo = 0 are exact, the
    output is f32(w_hi + w_lo) with |w - (w_hi + w_lo)| <= 2^-25 (w_lo at worst a subnormal half, spacing 2^-24) and the
    f32 sum rounds by at most 2^-24 x 0.33; the f32 form stores f32(w) and adds zeros.  Here: gemm_hd (M = 59) and
    gemm_hd2 at the cost rule's height (192 at this size), the f32 form through an odd output stride at the same sizes."""
    check_all(RC, "impulse", RC.case_set("impulse"), ran("impulse"))


@pytest.mark.parametrize("rows", ["256", "192"])
def test_pinned_tile_heights(RC, tile_runs, rows):
    """A and B on gemm_hd2_kernel with the tile height pinned: the impulses at M = 1079, dense noise at M = 1025 (one and
    two blocks per stream) and at the ragged M = 1539 = 8 x 192 + 3 = 6 x 256 + 3 (M = 387, gemm_hd, rides along)."""
    got = tile_runs[rows]
    assert isinstance(got, dict), got
    check_all(RC, f"tile {rows}", RC.case_set("tile"), got)


def test_row_count_edges(RC, ran):
    """B. Dense noise (rms 0.1, a seed per stream), pair form, every stream against the float64 oracle at 1e-5 max(1, peak).
    One block per stream (every second GEMM row dropped): M = 1, 127 | 129 around a 128-row tile, 1023 | 1025 around the
    switch of kernels; two blocks: 3-row groups across tile edges; three blocks: ragged last tiles, fewer than 8 row tiles
    and a count that is no multiple of 8 (the XCD swizzle pads the grid to eight and returns early)."""
    check_all(RC, "rows", RC.case_set("rows"), ran("rows"))


def test_length_and_stride_edges(RC, ran):
    """C. n_in around the 1024-sample chunk and the 1026-sample block, 3 streams each, 37 NaNs behind every input row, the
    output rows 2 (pair form) or 3 (f32 form) floats apart and prefilled with a sentinel: the oracle at the dense bar,
    every sentinel intact, everything finite; n_in <= 1024 produces nothing, returns CRISPY_OK and writes nothing."""
    cases = RC.case_set("lengths")
    outs = ran("lengths")              # a call that does not return CRISPY_OK raises in there
    for c in cases:
        if c.n_in <= 1024:
            assert c.out_len == 0 and np.all(outs[c.name] == RC.SENTINEL), c.name
    check_all(RC, "lengths", cases, outs)


def test_quiet_audio(RC, ran):
    """E. Samples from {-1, 0, +1} / 32768: exact f16 subnormals (x_lo = 0), so the error is the operator's 2^-25 per
    coefficient over at most 2052 terms of 3e-5, ~1e-10 against an output of ~1e-5; bar 1e-4 of the reference's own peak
    (a flushed subnormal operand gives zeros and misses it by four orders of magnitude).  The same signal x 2^-6 (2^-21 =
    8 subnormal steps, still exact) and x 0.7 x 2^-6 (5.6 steps: x_hi rounds, the rest is below half a step of x_lo):
    at most 2^-25 of a sample is lost, bar 2^-25 x sum |g| absolute."""
    check_all(RC, "quiet", RC.case_set("quiet"), ran("quiet"))


def test_handoff_modes_on_crafted_values(RC, ran):
    """D. Modes 1 (clamp) and 2 (clamp, s16 truncation) on 0, -0.0, +-1 and its f32 neighbours, +-2, +-1e30, +-inf, the
    three f32 values around +-k / 32767 at the truncation boundaries, +-1e-5, in noise; with scale 1 and with scale
    1 / 32768 on input multiplied by 32768; both forms.  The expected operator input is the reference's arithmetic in f32
    numpy (np.clip | wav_s16_roundtrip), then the float64 oracle at the dense bar.  A second stream carries one NaN in
    block 1: mode 2 reads it as 0 (Rust's `as i16`), modes 0 and 1 keep it (f32::clamp), which makes NaN of block 1's 342
    outputs and the next block's 342 and of nothing else."""
    check_all(RC, "handoff", RC.case_set("handoff"), ran("handoff"))

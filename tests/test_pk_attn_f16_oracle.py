"""Pins tests/pk_attn_f16_oracle.py (the definition of the Parakeet encoder's attention mode 1) and the new entry points' symbols; no
GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import pk_attn_f16_oracle as AO
from tests import pk_f16_oracle as FO
from tests import pk_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def operands(n, heads, seed, tmax=None):
    tmax = tmax or n
    rng = np.random.default_rng(seed)
    H = heads * AO.HEAD
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(n, 3 * H), f(2 * tmax - 1, H), 0.1 * f(H), 0.1 * f(H), tmax


@pytest.fixture(scope="module")
def weights():
    return PO.make_weights(PO.TINY, 1)


def test_both_switches_off_is_pk_oracle_bit_for_bit(weights):
    clips = [PO.clip(r, 128, 100 + r) for r in (9, 73)]
    for dtype in (torch.float64, torch.float32):
        a = AO.Encoder(PO.TINY, weights, dtype, attention=False, gemm=False).forward(clips)
        b = PO.Encoder(PO.TINY, weights, dtype).forward(clips)
        for x, y in zip(a, b):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and all(np.array_equal(s, t) for s, t in zip(x[2], y[2]))


def test_gemm_flag_alone_is_pk_f16_oracle(weights):
    clips = [PO.clip(73, 128, 173)]
    a = AO.Encoder(PO.TINY, weights, torch.float64, attention=False, gemm=True).forward(clips)
    b = FO.Encoder(PO.TINY, weights, torch.float64).forward(clips)
    assert np.array_equal(a[0][0], b[0][0])


def test_attention_switch_changes_block_0_and_hooks_are_independent(weights):
    clips = [PO.clip(73, 128, 173)]
    exact = PO.Encoder(PO.TINY, weights, torch.float64).forward(clips)[0][2][0]
    att = AO.Encoder(PO.TINY, weights, torch.float64).forward(clips)[0][2][0]
    both = AO.Encoder(PO.TINY, weights, torch.float64, gemm=True).forward(clips)[0][2][0]
    gemm = FO.Encoder(PO.TINY, weights, torch.float64).forward(clips)[0][2][0]
    assert 1e-6 < rms(att - exact) < 1e-2 and 1e-6 < rms(both - gemm) < 1e-2 and rms(both - att) > 1e-6


@pytest.mark.parametrize("n", [33, 65, 129, 257])
def test_the_key_tile_is_part_of_the_definition(n):
    """tile 32 and tile 64 of the same definition differ by more than 4 x the float32 form's distance to the float64 one"""
    qkv, r, u, v, tmax = operands(n, 2, 7 + n)
    a32 = AO.stage(qkv, r, u, v, [n], 2, tmax, 32)
    a64 = AO.stage(qkv, r, u, v, [n], 2, tmax, 64)
    yard = max(rms(AO.stage(qkv, r, u, v, [n], 2, tmax, t, torch.float32) - a) for t, a in ((32, a32), (64, a64)))
    print(f"pk attn f16 oracle n {n}: tile 32 vs 64 {rms(a32 - a64):.3e}, float32 form {yard:.3e} (ratio {rms(a32 - a64) / yard:.1f})")
    assert rms(a32 - a64) > 4.0 * yard


def test_tiles_agree_within_one_tile():
    qkv, r, u, v, tmax = operands(32, 1, 3)
    assert np.array_equal(AO.stage(qkv, r, u, v, [32], 1, tmax, 32), AO.stage(qkv, r, u, v, [32], 1, tmax, 64))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_key_gives_f16_v_exactly(dtype):
    qkv, r, u, v, tmax = operands(1, 2, 5, tmax=9)
    out = AO.stage(qkv, r, u, v, [1], 2, tmax, 32, dtype)
    want = qkv[:, 2 * 256:].astype(np.float16).astype(np.float64)
    assert np.array_equal(out.astype(np.float64), want)


@pytest.mark.parametrize("n", [2, 33, 100])
def test_zero_scores_give_the_exact_mean_of_f16_v(n):
    qkv, r, u, v, tmax = operands(n, 1, 11 + n)
    qkv[:, :128] = 0.0
    out = AO.stage(qkv, 0 * r, 0 * u, 0 * v, [n], 1, tmax, 32)
    want = qkv[:, 256:].astype(np.float16).astype(np.float64).sum(0) / n
    assert np.array_equal(out, np.broadcast_to(want, out.shape))


def test_a_clip_does_not_depend_on_its_neighbours():
    qkv, r, u, v, tmax = operands(50, 1, 21, tmax=40)
    both = AO.stage(qkv, r, u, v, [10, 40], 1, tmax, 32)
    assert np.array_equal(both[:10], AO.stage(qkv[:10], r, u, v, [10], 1, tmax, 32))
    assert np.array_equal(both[10:], AO.stage(qkv[10:], r, u, v, [40], 1, tmax, 32))


def test_symbols_abi_and_constants():
    from crispy_amd import _native as N
    L = N.lib()
    for s in ("crispy_pk_set_attention_precision", "crispy_pk_attention_precision", "crispy_pk_stage_attention_device"):
        assert s in N.ALL_SYMBOLS and hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "crispy_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    assert int(re.search(r"#define CRISPY_ABI_VERSION (\d+)", header).group(1)) == 6 == N.ABI_VERSION == L.crispy_abi_version()
    assert int(re.search(r"pub const CRISPY_ABI_VERSION: c_int = (\d+);", rust).group(1)) == 6
    assert int(re.search(r"#define CRISPY_PK_ATTN_KEY_TILE (\d+)", header).group(1)) == N.PK_ATTN_KEY_TILE
    assert N.PK_ATTN_KEY_TILE in (32, 64)
    for s in ("crispy_pk_set_attention_precision", "crispy_pk_attention_precision", "crispy_pk_stage_attention_device"):
        assert f"pub fn {s}(" in rust and f"int {s}(" in header
    assert L.crispy_pk_attention_precision(None) == 0
    assert L.crispy_pk_set_attention_precision(None, 1) == -1
    assert b"NULL handle" in L.crispy_last_error()

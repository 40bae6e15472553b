"""CPU pins of tests/pk_f16_oracle.py, the oracle of the Parakeet encoder's precision mode 1: with its hooks off it is pk_oracle bit for
bit, the hooked modules are exactly the products the library's GEMM performs, and one Linear written out by hand gives the same
numbers.  Also the boundary of the new entry points that needs no device."""
import numpy as np
import pytest
import torch

from tests import pk_f16_oracle as FO
from tests import pk_oracle as PO

ROWS = (9, 73)


@pytest.fixture(scope="module")
def weights():
    return PO.make_weights(PO.TINY, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_hooks_off_is_pk_oracle(weights, dtype):
    clips = [PO.clip(r, 128, 100 + r) for r in ROWS]
    a = PO.Encoder(PO.TINY, weights, dtype).forward(clips)
    b = FO.Encoder(PO.TINY, weights, dtype, hooks=False).forward(clips)
    for (oa, sa, ta), (ob, sb, tb) in zip(a, b):
        assert oa.tobytes() == ob.tobytes() and sa.tobytes() == sb.tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb))


def test_hooked_modules_are_the_gemm_list(weights):
    per_layer = ["feed_forward1.linear1", "feed_forward1.linear2", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                 "self_attn.relative_k_proj", "conv.pointwise_conv1", "conv.pointwise_conv2", "feed_forward2.linear1", "feed_forward2.linear2"]
    want = ["subsampling.linear"] + [f"layers.{l}.{q}" for l in range(PO.TINY.layers) for q in per_layer]
    enc = FO.Encoder(PO.TINY, weights, torch.float64)
    assert sorted(enc.hooked) == sorted(want) and sorted(FO.gemm_names(PO.TINY)) == sorted(want)
    mods = dict(enc.net.named_modules())
    for name, m in mods.items():
        if isinstance(m, torch.nn.Conv2d):
            assert name not in enc.hooked and not m._forward_pre_hooks      # the subsampling convolutions are not touched
            assert m.weight.detach().to(torch.float32).numpy().tobytes() == weights[name + ".weight"].tobytes()
    dw = mods["layers.0.conv.depthwise_conv"]
    assert not dw._forward_pre_hooks and dw.weight.detach().to(torch.float32).numpy().tobytes() == weights["layers.0.conv.depthwise_conv.weight"].tobytes()
    for name in enc.hooked:
        w = mods[name].weight
        assert torch.equal(w, FO.round_f16(w)) and len(mods[name]._forward_pre_hooks) == 1
    assert FO.Encoder(PO.TINY, weights, torch.float64, hooks=False).hooked == []


def test_rounding_is_torch_cast():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 65504.0, 65519.0, 65520.0,
                      -70000.0], dtype=torch.float64)
    want = [1.0, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, 2.0 ** -24, 0.0, 2.0 ** -23, 65504.0, 65504.0, float("inf"), float("-inf")]
    assert FO.round_f16(x).tolist() == want      # ties to even, subnormals kept, overflow to infinity


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_single_linear_by_hand(weights, dtype):
    """subsampling.linear of the hooked network against the definition written out in numpy"""
    enc = FO.Encoder(PO.TINY, weights, dtype)
    rng = np.random.default_rng(5)
    K = PO.TINY.sub_channels * PO.TINY.mel_bins // 8
    x = (rng.standard_normal((7, K)) * 3.0).astype(np.float32)
    got = enc.net.subsampling.linear(torch.from_numpy(x).to(dtype)).detach().numpy()
    npdt = np.float64 if dtype == torch.float64 else np.float32
    want = FO.linear_f16(x, weights["subsampling.linear.weight"], weights["subsampling.linear.bias"], npdt)
    if dtype == torch.float64:      # products of f16 values are exact in double and the sums differ by order only
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    plain = PO.Encoder(PO.TINY, weights, dtype).net.subsampling.linear(torch.from_numpy(x).to(dtype)).detach().numpy()
    assert np.abs(plain - got).max() > 1e-4      # the rounding is there


def test_mode1_changes_the_oracle(weights):
    x = [PO.clip(73, 128, 173)]
    a = PO.Encoder(PO.TINY, weights, torch.float64).forward(x)[0][0]
    b = FO.Encoder(PO.TINY, weights, torch.float64).forward(x)[0][0]
    d = np.abs(a - b).max()
    assert 1e-5 < d < 0.1, d


def test_new_symbols_and_null_handles():
    from crispy_amd import _native as N
    L = N.lib()
    NEW = ("crispy_pk_set_precision", "crispy_pk_precision", "crispy_pk_stage_gemm_device")
    assert N.PK_F16_SYMBOLS == NEW and set(NEW) <= set(N.ALL_SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes, name
    assert L.crispy_pk_precision(None) == 0
    assert L.crispy_pk_set_precision(None, 1) == -1 and b"NULL handle" in L.crispy_last_error()
    assert L.crispy_pk_stage_gemm_device(None, 1, 0, None, 1, 32, None, None, 128, 1.0, None, None) == -1
    assert L.crispy_abi_version() == 6

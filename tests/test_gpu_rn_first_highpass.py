"""The first sub-chunk's high-pass of a one-wave RNNoise handle runs as ONE launch of the deep kernel (32 samples requested
ahead) instead of two launches of the 32-register one (crispy_api.cpp, process_device_impl).  Both kernels are
rn_highpass_body, so nothing may change: the five golden streams of tests/golden/rn_frame_bits.npz, tiled to 65 streams
(a second high-pass workgroup with one live lane), fed as calls of 1, 2, 3 and 8 frames -- shorter than, equal to and
longer than the first sub-chunk, filter state carried over the calls -- in both layouts give the golden PCM and VAD byte
for byte, and so does the old form, which the developer knob CRISPY_RN_HP_FIRST=0 (libcrispy_hip_dev.so) restores.

The int16 transport (crispy_rn_process_s16_device) takes integer samples, and the golden inputs are not integer-valued, so
there the new form is held against the old one over the golden inputs rounded to int16: byte-equal PCM and VAD."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

from tests.native_variant import library_variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rn_frame_bits.npz")
STREAMS = 65
CALLS = (1, 2, 3, 8)


def _tool():
    spec = importlib.util.spec_from_file_location("make_rn_bits_golden", os.path.join(ROOT, "tools", "make_rn_bits_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    x = _tool().inputs()
    assert zlib.crc32(x.tobytes()) == int(g["x_crc"]), "the seeded inputs are not the ones the golden file was made from"
    pick = np.arange(STREAMS) % x.shape[1]
    return (np.ascontiguousarray(x[:, pick]), np.ascontiguousarray(g["pcm"][:, pick]), np.ascontiguousarray(g["vad"][:, pick]))


def _run(x, per_call, layout, first, s16=False):
    """x [T, B, 480] through a fresh one-wave handle of the developer build in calls of per_call frames -> (pcm [T, B, 480],
    vad [T, B]).  first: CRISPY_RN_HP_FIRST ("1": one deep launch, the default; "0": the split form)."""
    import torch

    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState

    T, B = x.shape[0], x.shape[1]
    dev = torch.device("cuda", 0)
    pcm = np.empty_like(x)
    vad = np.empty((T, B), dtype=np.float32)
    with library_variant("dev", {"CRISPY_RN_WAVES": "1", "CRISPY_RN_HP_FIRST": first}) as L:
        ds = DenoiseState(synthetic_weights(0), B, 0, lib=L)
        try:
            for t0 in range(0, T, per_call):
                n = min(per_call, T - t0)
                part = x[t0:t0 + n] if layout == "tbf" else x[t0:t0 + n].transpose(1, 0, 2)
                d_in = torch.from_numpy(np.ascontiguousarray(part)).to(dev)
                d_out = torch.zeros_like(d_in)
                d_vad = torch.zeros(n, B, device=dev)
                if s16:
                    ds.process_s16_device(d_in.data_ptr(), d_out.data_ptr(), n, d_vad.data_ptr(), layout=layout)
                else:
                    ds.process_device(d_in.data_ptr(), d_out.data_ptr(), n, d_vad.data_ptr(), layout=layout)
                ds.synchronize()
                out = d_out.cpu().numpy()
                pcm[t0:t0 + n] = out if layout == "tbf" else out.transpose(1, 0, 2)
                vad[t0:t0 + n] = d_vad.cpu().numpy()
        finally:
            ds.close()
    return pcm, vad


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        pytest.fail(f"{what}: {len(bad)} of {got.size} values differ, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("first", ["1", "0"], ids=["deep", "split"])
@pytest.mark.parametrize("layout", ["tbf", "btf"])
@pytest.mark.parametrize("per_call", CALLS)
def test_calls_of_any_length_give_the_golden_bits(golden, per_call, layout, first):
    x, pcm_want, vad_want = golden
    pcm, vad = _run(x, per_call, layout, first)
    _same(pcm, pcm_want, f"PCM, calls of {per_call}, {layout}, CRISPY_RN_HP_FIRST={first}")
    _same(vad, vad_want, f"VAD, calls of {per_call}, {layout}, CRISPY_RN_HP_FIRST={first}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["tbf", "btf"])
@pytest.mark.parametrize("per_call", CALLS)
def test_int16_transport_is_the_split_forms(golden, per_call, layout):
    x = np.clip(np.rint(golden[0]), -32768, 32767).astype(np.int16)
    pcm, vad = _run(x, per_call, layout, "1", s16=True)
    pcm_old, vad_old = _run(x, per_call, layout, "0", s16=True)
    assert np.abs(pcm_old.astype(np.int32)).max() > 1000, "the int16 path produced no signal to compare"
    _same(pcm, pcm_old, f"int16 PCM, calls of {per_call}, {layout}")
    _same(vad, vad_old, f"int16 VAD, calls of {per_call}, {layout}")

"""Sub-chunk size and ramp are members of the RNNoise handle, read when it is created (crispy_api.cpp: read_schedule; the
developer knobs CRISPY_RN_SUB_FRAMES and CRISPY_RN_RAMP of libcrispy_hip_dev.so set them per handle).  How a call is cut
into launches must not show in what it computes: handles of grain 12 / ramp 3,4,5,7,10 (the defaults), 16 / 3,4,6,9 and
24 / 4,6,9 give the golden PCM and VAD of tests/golden/rn_frame_bits.npz byte for byte, from one 14-frame call and from
calls of 5 + 9 frames, in both frame-kernel forms.

bench.py --full divides a step's frame-kernel time by crispy_rn_n_launches(T), so a handle created with the defaults must
launch exactly that many frame kernels: counted from the timeline the developer build prints per timed sub-chunk
(CRISPY_RN_TIMELINE) for calls of 1, 3, 8, 100 and 251 frames -- 251 crosses the 250-frame segment."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

from tests.native_variant import library_variant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rn_frame_bits.npz")
SCHEDULES = [("12", "3,4,5,7,10"), ("16", "3,4,6,9"), ("24", "4,6,9")]


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
    return g, x


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 3])
@pytest.mark.parametrize("calls", [(14,), (5, 9)], ids=["one-call", "5+9"])
@pytest.mark.parametrize("grain,ramp", SCHEDULES, ids=[f"{g}:{r}" for g, r in SCHEDULES])
def test_any_grain_gives_the_golden_bits(golden, grain, ramp, calls, waves):
    import torch

    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState

    g, x = golden
    sfx = "" if waves == 1 or int(g["w3_same"]) else "_w3"
    T, B = x.shape[0], x.shape[1]
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(x).to(dev)
    d_out = torch.zeros_like(d_in)
    d_vad = torch.zeros(T, B, device=dev)
    with library_variant("dev", {"CRISPY_RN_WAVES": str(waves), "CRISPY_RN_SUB_FRAMES": grain, "CRISPY_RN_RAMP": ramp}) as L:
        ds = DenoiseState(synthetic_weights(0), B, 0, lib=L)
        try:
            t0 = 0
            for n in calls:          # TBF: a call's frames are a contiguous slice of the tensors
                ds.process_device(d_in[t0:].data_ptr(), d_out[t0:].data_ptr(), n, d_vad[t0:].data_ptr())
                t0 += n
            assert t0 == T
            ds.synchronize()
        finally:
            ds.close()
    what = f"grain {grain}, ramp {ramp}, calls {calls}, {waves} wave(s) per stream"
    _same(d_out.cpu().numpy(), g["pcm" + sfx], "PCM, " + what)
    _same(d_vad.cpu().numpy(), g["vad" + sfx], "VAD, " + what)


@pytest.mark.gpu
def test_a_default_handle_launches_what_n_launches_reports(capfd):
    import torch

    from crispy_amd import _native as N
    from crispy_amd import synth_audio, synthetic_weights
    from crispy_amd.denoise import DenoiseState

    B = 5
    dev = torch.device("cuda", 0)
    want = {T: N.lib().crispy_rn_n_launches(T) for T in (1, 3, 8, 100, 251)}
    assert want[100] == 11 and N.lib().crispy_rn_frames_per_launch() == 12      # the defaults this file's docstring names
    got = {}
    with library_variant("dev", {"CRISPY_RN_TIMELINE": "1"}) as L:
        assert not any(k in os.environ for k in ("CRISPY_RN_SUB_FRAMES", "CRISPY_RN_RAMP")), "a default handle is wanted"
        ds = DenoiseState(synthetic_weights(0), B, 0, lib=L)
        try:
            ds.set_timing(True)
            x = synth_audio.batch_torch(B, max(want), dev)
            y = torch.empty_like(x)
            for T in want:
                ds.process_device(x.data_ptr(), y.data_ptr(), T)
                ds.synchronize()
                capfd.readouterr()
                ds.last_kernel_ms()
                got[T] = sum(1 for line in capfd.readouterr().err.splitlines() if line.startswith("[rn timeline] sub-chunk"))
        finally:
            ds.close()
    print(got)
    assert got == want

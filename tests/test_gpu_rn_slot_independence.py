"""What a stream's wave computes must not depend on where the wave runs: the one-wave RNNoise frame kernel picks its issue
priority from its slot on the SIMD and the frame inside the launch (crispy_amd/csrc/rn_prio.h), which may change when a wave
issues, never what.  The five golden streams of tools/make_rn_bits_golden.py (5 streams x 14 frames) are tiled so that stream i
carries golden stream i mod 5, with 4096 streams (four waves on every SIMD of the device) and with 4160 (a second round of
workgroups whose waves inherit whichever slots fall free); every stream's PCM and VAD must equal
tests/golden/rn_frame_bits.npz byte for byte.  The default ramp cuts 14 frames into launches of 3, 4, 5 and 2 frames, so launch
boundaries and a full rotation of the priorities are inside."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rn_frame_bits.npz")


@pytest.fixture(scope="module")
def golden():
    spec = importlib.util.spec_from_file_location("make_rn_bits_golden", os.path.join(ROOT, "tools", "make_rn_bits_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = np.load(GOLDEN)
    x = tool.inputs()
    assert zlib.crc32(x.tobytes()) == int(g["x_crc"]), "the seeded inputs are not the ones the golden file was made from"
    return x, g["pcm"], g["vad"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_streams", [4096, 4160])
def test_every_stream_matches_its_golden_stream(golden, monkeypatch, n_streams):
    import torch

    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState

    x, pcm_g, vad_g = golden
    T = x.shape[0]
    src = np.arange(n_streams) % x.shape[1]
    monkeypatch.setenv("CRISPY_RN_WAVES", "1")
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(np.ascontiguousarray(x[:, src])).to(dev)
    d_out = torch.zeros_like(d_in)
    d_vad = torch.zeros(T, n_streams, device=dev)
    ds = DenoiseState(synthetic_weights(0), n_streams, 0)
    try:
        ds.process_device(d_in.data_ptr(), d_out.data_ptr(), T, d_vad.data_ptr())
        ds.synchronize()
        pcm, vad = d_out.cpu().numpy(), d_vad.cpu().numpy()
    finally:
        ds.close()
    bad = np.flatnonzero((pcm.view(np.uint32) != pcm_g[:, src].view(np.uint32)).any(axis=(0, 2)))
    assert bad.size == 0, f"PCM of {bad.size} of {n_streams} streams differs from the golden bits, first: stream {bad[0]} (golden {src[bad[0]]})"
    bad = np.flatnonzero((vad.view(np.uint32) != vad_g[:, src].view(np.uint32)).any(axis=0))
    assert bad.size == 0, f"VAD of {bad.size} of {n_streams} streams differs from the golden bits, first: stream {bad[0]} (golden {src[bad[0]]})"

"""The RNNoise frame kernel against the bits it produced before its instruction-count pass (tests/golden/rn_frame_bits.npz,
written by tools/make_rn_bits_golden.py at the parent commit): denoised PCM, VAD and the per-frame taps of 5 streams x 14
frames -- silence, tone + noise, a 600 Hz tone (remove_doubling skips every candidate chunk), a 70 Hz tone (every chunk that
can run does) and a full-scale stream -- byte for byte, in both frame-kernel forms.  The changes it guards remove
instructions and keep every floating-point operation and its order, so there is no tolerance to speak of."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rn_frame_bits.npz")


def _tool():
    spec = importlib.util.spec_from_file_location("make_rn_bits_golden", os.path.join(ROOT, "tools", "make_rn_bits_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    tool = _tool()
    x = tool.inputs()
    assert zlib.crc32(x.tobytes()) == int(g["x_crc"]), "the seeded inputs are not the ones the golden file was made from"
    return g, tool, x


def _same(got: np.ndarray, want: np.ndarray, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 3])
def test_frame_kernel_bits_match_parent(golden, waves):
    g, tool, x = golden
    sfx = "" if waves == 1 or int(g["w3_same"]) else "_w3"
    pcm, vad, taps, pcm_taps = tool.run(x, waves)
    _same(pcm, g["pcm" + sfx], f"PCM, {waves} wave(s) per stream")
    _same(vad, g["vad" + sfx], f"VAD, {waves} wave(s) per stream")
    _same(taps, g["taps" + sfx], f"taps, {waves} wave(s) per stream")
    if int(g["taps_pcm_same"]):
        _same(pcm_taps, g["pcm" + sfx], f"PCM of the call with taps, {waves} wave(s) per stream")

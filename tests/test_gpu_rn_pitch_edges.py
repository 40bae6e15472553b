"""The corners of the coarse pitch search's top-2 arg-max (wave_best and the per-lane insertion in front of it), and the gain
network on the loudest and the quietest input that reaches it, in both frame-kernel forms: 8 streams x 6 frames,
tools/make_rn_bits_golden.py: edge_inputs().

  stream  case                                                     what the CPU check below establishes first
  0       (a) no valid candidate, total_valid == 0                 every coarse correlation <= 0 on every frame
  1       (b) total_valid == 1, (e) winner in lane 0               lag 0 alone is positive from frame 1 on
  2       (c) exact ties at NON-ZERO (num, den)                    on frames 2 - 5 the winner's pair (a few units of 2^-149, 1)
                                                                   stands at other lags too, in other lanes on each of them
                                                                   and inside the winner's lane on one; the winner is the
                                                                   lowest of them and is not lag 0
  3       (c) exact ties at (0, 1)                                 at every valid lag from frame 1 on; the winner is lag 0, the
                                                                   runner-up lag 1 of the same lane
  4       (d) best and second-best lag in the same lane            on at least three of the six frames
  5       (e) winner in lane 48                                    on every frame
  6, 7    (f) noise at full scale and at 2^-13 of it               the oracle's silence flag is 0 on every frame: both streams
                                                                   run the gain network (image_i8, scale_of, dotn_i)

Three signals of the issue's list were changed after the CPU check, not the bars.  An exactly periodic integer-valued signal
does NOT tie (of five periods tried none did: the search sees the signal behind the high-pass, whose transient outlasts six
frames, so no two lags get equal operands).  Ties come from small amplitudes instead, where Syy = 1 + energy rounds to exactly 1
and num = (xcorr 1e-12)^2 is a subnormal of a few units (stream 2: equal non-zero pairs) or underflows to 0 (stream 3); both
tie streams tie (the issue allows one of them not to).  They are silent frames, so the pitch index is what shows their result.
Digital silence behind two frames of tone still has ~70 valid lags (the tail of the high-pass correlates with itself); no
valid candidate comes from an impulse train whose period no lag reaches.  Noise at 2^-20 of full scale fails the silence gate
and never runs the gain network; 2^-13 is the lowest power of two that passes it on all six frames.  And the input scale does
not steer the digit scale anyway: scale_of sees the largest feature or activation of a frame (6.8 .. 62 over these two
streams, exponent bytes 129 .. 132 of a clamp of [64, 250]).  The clamp's ends and the exponent add of scale_shift are checked
on the host over every exponent, from the header the kernel compiles: tests/test_rn_scale_host.py.

Checks on the GPU: pitch index and silence flag EQUAL to the C oracle's; PCM inside the bar of tests/test_gpu_rnnoise.py
(1e-4).  VAD: the issue says equal, this test asks |difference| < 1e-4, the bar of tests/test_gpu_rnnoise.py -- the float
oracle and the int8 digit path of the kernel do not round alike, so equality is not reachable (measured: up to 6.1e-6); the
parent's VAD is held bit for bit by the second check.  That one: every bit equal to tests/golden/rn_frame_bits_edges.npz, which
`tools/make_rn_bits_golden.py --edges` wrote at the commit before the branch-free arg-max."""
import importlib.util
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rn_frame_bits_edges.npz")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("make_rn_bits_golden", os.path.join(ROOT, "tools", "make_rn_bits_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def edge_x(tool):
    x = tool.edge_inputs()
    assert x.shape == (tool.EDGE_T, tool.EDGE_B, 480) and x.dtype == np.float32
    return x


@pytest.fixture(scope="module")
def oracle_ref(tool, edge_x, oracle, weights0):
    """Per stream: the oracle's PCM, VAD, taps, and per frame the candidate pattern of the coarse search (from the oracle's own
    whitened half-rate buffer).  Computed once, read by every test."""
    ref = []
    for b in range(tool.EDGE_B):
        st = oracle.OracleDenoiseState(weights0)
        out = np.empty((tool.EDGE_T, 480), np.float32)
        vad = np.empty(tool.EDGE_T, np.float32)
        taps = np.empty((tool.EDGE_T, oracle.TAPS), np.float32)
        pat = []
        for t in range(tool.EDGE_T):
            out[t], vad[t] = st.process_frame(edge_x[t, b])
            taps[t] = st.taps()
            pat.append(tool.coarse_pattern(st.debug()[984:984 + 864]))
        ref.append({"out": out, "vad": vad, "taps": taps, "pat": pat})
    return ref


def test_edge_inputs_reach_their_corners(tool, edge_x, oracle_ref):
    T = tool.EDGE_T
    lane = lambda lag: lag // 3
    for b, name in enumerate(tool.EDGE_CASES):
        for t, (valid, num, den, best, second, tied) in enumerate(oracle_ref[b]["pat"]):
            print(f"{name} frame {t}: {int(valid.sum())} valid, best {best} second {second}, {len(tied)} tied with the winner")
    # (a) no valid candidate at all
    assert all(int(p[0].sum()) == 0 for p in oracle_ref[0]["pat"])
    # (b) exactly one, and (e) it sits in lane 0
    for t in range(1, T):
        valid, _, _, best, second, _ = oracle_ref[1]["pat"][t]
        assert int(valid.sum()) == 1 and best == 0 and second is None, t
    # (c) exact ties at non-zero (num, den): in another lane on frames 2 - 5, inside the winner's lane on one of them; the lower
    # index wins, and it is not the {0, 1} that the search falls back to without candidates
    in_lane = 0
    for t in range(2, T):
        valid, num, den, best, second, tied = oracle_ref[2]["pat"][t]
        assert tied and num[best] > 0 and best > 1, t
        assert all(num[j] == num[best] and den[j] == den[best] for j in tied), t
        assert any(lane(j) != lane(best) for j in tied), t
        assert best < min(tied) and second == min(tied), (t, best, second)
        in_lane += any(lane(j) == lane(best) for j in tied)
    assert in_lane >= 1
    # (c) exact ties at (0, 1): in another lane and inside the winner's lane; the lower index wins both places
    for t in range(1, T):
        valid, num, den, best, second, tied = oracle_ref[3]["pat"][t]
        assert tied and num[best] == 0 and den[best] == 1, t
        assert all(num[j] == num[best] and den[j] == den[best] for j in tied), t
        assert any(lane(j) != lane(best) for j in tied) and any(lane(j) == lane(best) for j in tied), t
        assert best < min(tied) and second == min(tied) and lane(second) == lane(best), (t, best, second)
    # (d) best and second-best lag in one lane, no tie involved
    same = [t for t in range(T) if oracle_ref[4]["pat"][t][3] is not None and oracle_ref[4]["pat"][t][4] is not None
            and lane(oracle_ref[4]["pat"][t][3]) == lane(oracle_ref[4]["pat"][t][4]) and not oracle_ref[4]["pat"][t][5]]
    assert len(same) >= 3, same
    # (e) winner in the last lane that owns lags
    assert all(lane(p[3]) == 48 for p in oracle_ref[5]["pat"])
    # (f) the loudest and the quietest noise that reach the gain network: no frame is taken for silence
    assert np.abs(edge_x[:, 6]).max() == np.float32(32767.0)
    assert np.abs(edge_x[:, 7]).max() == np.float32(32767.0 * 2.0 ** -13)
    for b in (6, 7):
        assert not oracle_ref[b]["taps"][:, 67].any(), (b, oracle_ref[b]["taps"][:, 67])
        fmax = np.abs(oracle_ref[b]["taps"][:, :42]).max(axis=1)
        print(f"{tool.EDGE_CASES[b]}: largest |feature| per frame {np.round(fmax, 2).tolist()}")
        assert fmax.min() >= 4.0 and fmax.max() < 64.0          # exponent bytes 129 .. 132: the middle of the clamp, as the docstring says


_runs = {}


def _gpu_run(tool, edge_x, waves):
    if waves not in _runs:
        _runs[waves] = tool.run(edge_x, waves)
    return _runs[waves]


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 3])
def test_edges_against_the_oracle(tool, edge_x, oracle_ref, waves):
    pcm, vad, taps, _ = _gpu_run(tool, edge_x, waves)
    for b, name in enumerate(tool.EDGE_CASES):
        r = oracle_ref[b]
        err = float(np.abs(pcm[:, b] - r["out"]).max())
        bar = 1e-4 * float(np.abs(r["out"]).max()) + 1e-3
        verr = float(np.abs(vad[:, b] - r["vad"]).max())
        print(f"{name}, {waves} wave(s): pitch {taps[:, b, 64].astype(int).tolist()} oracle {r['taps'][:, 64].astype(int).tolist()}"
              f" | PCM err {err:.3e} (bar {bar:.3e}) | VAD err {verr:.2e}")
    for b, name in enumerate(tool.EDGE_CASES):
        r = oracle_ref[b]
        assert np.array_equal(taps[:, b, 64], r["taps"][:, 64]), f"pitch index, {name}"
        assert np.array_equal(taps[:, b, 67], r["taps"][:, 67]), f"silence flag, {name}"
        assert np.abs(vad[:, b] - r["vad"]).max() < 1e-4, f"VAD, {name}"
        assert np.abs(pcm[:, b] - r["out"]).max() <= 1e-4 * np.abs(r["out"]).max() + 1e-3, f"PCM, {name}"


def _same(got: np.ndarray, want: np.ndarray, what: str):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        pytest.fail(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[0].tolist()}: "
                    f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 3])
def test_edges_bits_match_parent(tool, edge_x, waves):
    g = np.load(GOLDEN)
    assert zlib.crc32(edge_x.tobytes()) == int(g["x_crc"]), "the seeded inputs are not the ones the golden file was made from"
    sfx = "" if waves == 1 or int(g["w3_same"]) else "_w3"
    pcm, vad, taps, pcm_taps = _gpu_run(tool, edge_x, waves)
    _same(pcm, g["pcm" + sfx], f"PCM, {waves} wave(s) per stream")
    _same(vad, g["vad" + sfx], f"VAD, {waves} wave(s) per stream")
    _same(taps, g["taps" + sfx], f"taps, {waves} wave(s) per stream")
    if int(g["taps_pcm_same"]):
        _same(pcm_taps, g["pcm" + sfx], f"PCM of the call with taps, {waves} wave(s) per stream")

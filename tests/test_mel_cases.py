"""tests/mel_cases.py -- the references and the statistic of tests/test_gpu_logmel_precision.py -- checked on the CPU: the
float64 form against the two log-mel oracles the suite already has, the conditions on the inputs (how many elements may
lie in the band around the floor's switch), the teeth of the statistic, and the exactness of (x + 4) / 4 that lets the
public output give back the frame kernel's floats."""
import numpy as np
import pytest

from tests import mel_cases as MC


def _normalised(r64, n_frames=3000):
    """[n_mel, 3000] as the 30 s path gives it: the frames past the audio are the floor."""
    full = np.full((r64.shape[0], n_frames), MC.FLOOR)
    full[:, :min(n_frames, r64.shape[1])] = r64[:, :n_frames]
    return (np.maximum(full, full.max() - 8.0) + 4.0) / 4.0


@pytest.mark.parametrize("n", [201, 399, 401, 9881, 40123])
def test_float64_form_equals_the_long_oracle(n):
    from tests import long_logmel_oracle as LO
    for b in ("80", "128"):
        x = MC.edge_clip(n)
        r64 = MC.power(x, MC.bank(b))[2]
        ref = LO.raw(x, int(b), MC.bank(b))
        T = MC.live_frames(n)
        assert r64.shape == (int(b), T) and np.all(ref[:, T:] == MC.FLOOR)
        d = np.abs(r64 - ref[:, :T]).max()
        print(f"n {n}, {b} mels: max difference {d:.1e}")
        assert d <= 1e-12                       # the same float64 formula; the filter sums may be added in another order


@pytest.mark.parametrize("n", [1, 100, 399, 401, 16000])
def test_float64_form_equals_the_c_oracle(oracle, n):
    F = MC.bank("80")
    x = MC.edge_clip(n)
    d = np.abs(_normalised(MC.power(x, F)[2]) - oracle.oracle_logmel(x, F)).max()
    print(f"n {n}: max difference {d:.2e}")
    assert d < 2e-5                             # tests/test_long_logmel_oracle.py: BAR


def test_band_caps_and_teeth_on_every_numeric_case():
    """The conditions on the inputs, from the float64 reference alone: the band between 0.5e-10 and 2e-10 holds at most
    1 % (clips of >= 64 frames) or 4 % of a clip's elements at the scale the quiet rule gives.  And the statistic sees a
    poor table: the float32 reference with every bin's gain off by 1e-5 rms exceeds FACTOR x the clean one."""
    gains = MC.bin_gains(1e-5)
    worst_band, least = {}, {}
    banks = {b: MC.bank(b) for b in ("80", "128", "id0", "id73", "limits")}
    for name, b, x in MC.numeric_cases():
        F = banks[b]
        xq, k = MC.quiet(x, F)
        ref = MC.Ref(xq, F)
        assert ref.r64.max() < MC.QUIET_MAX and ref.r64.max() - 8.0 < MC.FLOOR
        share = MC.band_share(ref.M)
        assert share <= MC.band_cap(xq.size), (name, share)
        assert MC.floor_ok(ref.r32, ref.M), name
        assert ref.D32 > 0.0, name
        ratio = ref.D(MC.power_f32(xq, F, gains)[1]) / ref.D32
        assert ratio > MC.FACTOR, (name, ratio)
        group = name.rsplit("/", 1)[0] if name.startswith("c/") else name
        worst_band[b] = max(worst_band.get(b, 0.0), share)
        least[group] = min(least.get(group, np.inf), ratio)
    print("largest share of a clip's elements in the band, per bank:", {k: f"{100 * v:.3f} %" for k, v in worst_band.items()})
    print("1e-5 rms gain fault / clean float32 reference, least per case:", {k: round(v, 1) for k, v in least.items()})


def test_burst_clips_hold_their_maximum_where_they_say():
    """(d): the maximum of the float64 reference lies in the frame the case names, in a row below 64 (200 Hz) or from 64
    on (7 kHz), at least two decades above every frame the tone does not reach, and the band cap holds."""
    for b in ("80", "128"):
        F = MC.bank(b)
        for hz in (200.0, 7000.0):
            for where in MC.BURST_FRAMES:
                x, t = MC.burst_clip(where, hz)
                M, Tp, r64 = MC.power(x, F)
                m, tt = np.unravel_index(r64.argmax(), r64.shape)
                assert tt == t and (m >= 64) == (hz > 1000.0), (b, hz, where, m, tt)
                far = np.abs(np.arange(r64.shape[1]) - t) > 2
                assert r64[:, far].max() <= r64.max() - 2.0, (b, hz, where)
                assert r64[:, np.arange(r64.shape[1]) != t].max() < r64.max() - 0.01      # another frame is 10^5 tolerances away
                assert MC.band_share(M) <= MC.band_cap(x.size)
    assert MC.live_frames(MC.BURST_N) == 70


def test_output_gives_back_every_raw_float_between_minus_10_and_minus_2():
    """Every f32 in [-10, -2): (raw + 4) / 4 as the finish kernel computes it (float64, rounded once) is exact, so
    4 out - 4 is the float again."""
    lo, hi = np.float32(-2.0).view(np.uint32), np.float32(-10.0).view(np.uint32)      # negative floats: bits grow with |x|
    n = 0
    for a in range(int(lo) + 1, int(hi) + 1, 1 << 22):
        raw = np.arange(a, min(a + (1 << 22), int(hi) + 1), dtype=np.uint32).view(np.float32)
        out = ((raw.astype(np.float64) + 4.0) / 4.0).astype(np.float32)
        assert np.array_equal(out.astype(np.float64) * 4.0 - 4.0, raw.astype(np.float64))
        assert np.array_equal(MC.out_to_raw(out).view(np.uint32), raw.view(np.uint32))
        n += raw.size
    assert n == (1 << 21) + (1 << 23) + (1 << 23)          # a quarter of [-16, -8), [-8, -4), [-4, -2)


def test_limits_bank_and_inputs_are_what_they_claim():
    F = MC.limits_bank()
    assert MC.bank_taps(F) == (MC.MEL_FW_MAX, 64)
    assert not F[1].any() and F[0, 0] != 0 and F[0, 63] != 0 and not F[0, 64:].any()
    nz = np.flatnonzero(F[2])
    assert (F[2, nz[0]:nz[-1] + 1] == 0).sum() == 3
    assert F[:, 0].any() and F[:, 200].any()
    s, near1 = MC.log10_inputs()
    assert 5.9e6 < s.size < 6.3e6 and np.all(np.diff(s) >= 0) and np.abs(near1 - 1.0).max() <= 2.0 ** -10
    assert MC.ulp32(1.0) == 2.0 ** -23 and MC.ulp32(0.99) == 2.0 ** -24 and MC.ulp32(-9.5) == 2.0 ** -20

"""Developer tool, needs the GPU: records what the RNNoise frame kernel computes, bit for bit, so that a change that is
meant to keep every floating-point operation and its order can be held against the commit before it.
    python tools/make_rn_bits_golden.py [out.npz]        (default tests/golden/rn_frame_bits.npz)
    python tools/make_rn_bits_golden.py --edges [out.npz] (default tests/golden/rn_frame_bits_edges.npz: edge_inputs(), below)
Run it at the PARENT of the change; tests/test_gpu_rn_frame_bits.py and tests/test_gpu_rn_pitch_edges.py compare the working
tree with the files.

5 streams x 14 frames in one call (long enough to cross the 3-, 4- and 5-frame sub-chunk boundaries of a call), both
frame-kernel forms (CRISPY_RN_WAVES=1 and =3):
  0  digital silence                      the `silence` branch
  1  synth_audio stream 1                 tone + noise
  2  600 Hz tone                          T0 = 40: remove_doubling skips every candidate chunk ((2 T0 + k0) / (2 k0) < 30)
  3  70 Hz tone                           T0 ~ 342: every candidate chunk that can run does
  4  tone + noise at full scale           the digit scale of the gain network's fixed-point images
PCM and VAD come from the plain kernel (what bench.py runs), the taps from a second call with taps on (the capture
instantiation of the same code; `taps_pcm_same` = 1: that call's PCM equals the first one's).  The three-wave form's arrays are stored only
where they differ from the one-wave form's (`w3_same` = 1: they do not).  The inputs are not stored: the test makes them
again with inputs() and checks their CRC against `x_crc`."""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T = 5, 14


def inputs() -> np.ndarray:
    """[T, B, 480] f32 in int16 range, seeded."""
    from crispy_amd import synth_audio

    n = T * 480
    t = np.arange(n, dtype=np.float64) / 48000.0
    rng = np.random.default_rng(20240611)

    def tone(f0, noise):
        s = np.zeros(n)
        for h in range(1, 5):
            s += np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi)) / h
        s *= 0.2 / np.sqrt(np.mean(s ** 2))
        return s + noise * rng.standard_normal(n)

    full = synth_audio.stream_np(3, T, silent=False).astype(np.float64)
    full *= 32767.0 / np.abs(full).max()
    streams = [np.zeros(n), synth_audio.stream_np(1, T, silent=False) * 32768.0, tone(600.0, 0.002) * 32768.0,
               tone(70.0, 0.002) * 32768.0, full]
    x = np.stack([s.astype(np.float32) for s in streams], axis=0)
    return np.ascontiguousarray(x.reshape(B, T, 480).transpose(1, 0, 2))


EDGE_B, EDGE_T = 8, 6
EDGE_CASES = ("a_none_valid", "b_one_valid", "c_tie_nonzero", "c_tie_zero", "d_same_lane", "e_lane48", "f_full_scale", "f_low_scale")


def edge_inputs() -> np.ndarray:
    """[EDGE_T, EDGE_B, 480] f32: the corners of the coarse pitch search's top-2 arg-max and of the digit scales
    (tests/test_gpu_rn_pitch_edges.py checks on the CPU that each stream reaches its corner).  Lag i of the coarse search is
    a delay of 192 - i samples at 12 kHz; lane l owns lags 3 l .. 3 l + 2.
      0  impulses every 800 samples    delay 200 is out of reach, every other product is tail x impulse < 0: no valid lag
      1  impulses every 768 samples    delay 192 = lag 0 alone lines up: one valid lag, the winner sits in lane 0
      2  263.7 Hz tone, amplitude 1e-5 Syy = 1 + 1e-8 rounds to 1 and num = (xcorr 1e-12)^2 is a subnormal of a few units of
                                       2^-149: the lags around each correlation peak hold EQUAL NON-ZERO (num, den), in one
                                       lane and across lanes, and the peaks (182 samples = 4 periods) sit off lag 0
      3  62.5 Hz tone, amplitude 1e-7  num underflows to 0: every valid lag holds the pair (0, 1) exactly -- ties across the
                                       lanes and inside lane 0 (lags 0, 1, 2 are at the peak of the correlation, 192 being a
                                       whole number of periods)
      4  100 Hz + 200 Hz               best and second-best lag in one lane
      5  255 Hz square wave, decaying  winner in lane 48
      6  noise at full scale           the gain network on loud input
      7  noise at 2^-13 of full scale  and on the quietest input that still passes the silence gate on every frame (2^-14
                                       fails it on the first).  Both run image_i8 / scale_of / dotn_i; the digit scale
                                       follows the largest feature or activation, not the PCM, so it stays near the middle
                                       of its range (exponent bytes 129 .. 132 for the features): the ends of the clamp are
                                       tests/test_rn_scale_host.py's.
    (A periodic integer-valued signal does not tie: what the search sees has been through the high-pass, whose transient
    outlasts six frames, so no two lags see equal operands.  Digital silence behind a tone is not free of candidates
    either: the high-pass tail correlates with itself at every lag.)"""
    n = EDGE_T * 480
    k = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(20240917)
    imp800, imp768 = np.zeros(n), np.zeros(n)
    imp800[::800] = 20000.0
    imp768[::768] = 20000.0
    noise = rng.standard_normal(n)
    noise *= 32767.0 / np.abs(noise).max()
    streams = [imp800, imp768,
               1e-5 * np.sin(2 * np.pi * (4 * 12000.0 / 182.0) * k / 48000.0), 1e-7 * np.sin(2 * np.pi * 62.5 * k / 48000.0),
               8000.0 * np.sin(2 * np.pi * 100.0 * k / 48000.0) + 3000.0 * np.sin(2 * np.pi * 200.0 * k / 48000.0 + 1.0),
               8000.0 * np.sign(np.sin(2 * np.pi * 255.0 * k / 48000.0)) * 0.999 ** (k / 48.0),
               noise, noise * 2.0 ** -13]
    x = np.stack([s.astype(np.float32) for s in streams], axis=0)
    return np.ascontiguousarray(x.reshape(EDGE_B, EDGE_T, 480).transpose(1, 0, 2))


def coarse_pattern(lp: np.ndarray):
    """The candidates of the coarse search (find_best_pitch over 147 lags at quarter rate) from one frame's whitened
    half-rate buffer lp[864], in numpy: -> (valid [147] bool, num [147] f32, den [147] f32, best, second, tied) with best /
    second the lags the top-2 rule picks (None where there is none) and tied the valid lags whose (num, den) compare equal
    to the winner's in both rounded products.
    The sums are formed in float64 and rounded once: neither the kernel's nor the oracle's fmaf order, a third arithmetic.
    Signs, the underflow of num and the rounding of Syy to 1 do not depend on that; which lags hold equal subnormal num and
    which lag wins cases (d) and (e) could, at a rounding boundary -- what the GPU does is held against the oracle itself."""
    f32 = np.float32
    lp = np.asarray(lp, dtype=f32)
    x4 = lp[384 + 2 * np.arange(240)].astype(np.float64)
    y4 = lp[2 * np.arange(387)].astype(np.float64)
    xc = np.array([np.dot(x4, y4[i:i + 240]) for i in range(147)]).astype(f32)
    pre = np.concatenate([[0.0], np.cumsum(y4 * y4)])
    den = np.maximum(f32(1), (1.0 + (pre[240:387] - pre[:147])).astype(f32))
    x16 = xc * f32(1e-12)
    num = x16 * x16
    valid = xc > 0

    def better(a, b):
        lhs, rhs = num[a] * den[b], num[b] * den[a]
        return bool(lhs > rhs) or (not bool(rhs > lhs) and a < b)

    best = second = None
    for i in np.flatnonzero(valid):
        if best is None or better(i, best):
            best, second = int(i), best
        elif second is None or better(i, second):
            second = int(i)
    tied = [] if best is None else [int(j) for j in np.flatnonzero(valid)
                                    if j != best and num[best] * den[j] == num[j] * den[best]]
    return valid, num, den, best, second, tied


def run(x: np.ndarray, waves: int, lib=None):
    """-> (pcm [T,B,480], vad [T,B], taps [T,B,72], pcm of the call with taps) of a fresh handle in the given form."""
    T, B = x.shape[0], x.shape[1]
    import torch

    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState

    old = os.environ.get("CRISPY_RN_WAVES")
    os.environ["CRISPY_RN_WAVES"] = str(waves)
    try:
        dev = torch.device("cuda", 0)
        d_in = torch.from_numpy(x).to(dev)
        res = []
        for with_taps in (False, True):
            ds = DenoiseState(synthetic_weights(0), B, 0, lib=lib)
            d_out = torch.zeros_like(d_in)
            d_vad = torch.zeros(T, B, device=dev)
            d_taps = torch.zeros(T, B, 72, device=dev)
            ds.process_device(d_in.data_ptr(), d_out.data_ptr(), T, d_vad.data_ptr(), d_taps.data_ptr() if with_taps else 0)
            ds.synchronize()
            res.append((d_out.cpu().numpy(), d_vad.cpu().numpy(), d_taps.cpu().numpy()))
            ds.close()
    finally:
        if old is None:
            del os.environ["CRISPY_RN_WAVES"]
        else:
            os.environ["CRISPY_RN_WAVES"] = old
    return res[0][0], res[0][1], res[1][2], res[1][0]


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    args = [a for a in sys.argv[1:] if a != "--edges"]
    edges = len(args) != len(sys.argv) - 1
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "rn_frame_bits_edges.npz" if edges else "rn_frame_bits.npz")
    x = edge_inputs() if edges else inputs()
    pcm1, vad1, taps1, pcm1t = run(x, 1)
    pcm3, vad3, taps3, pcm3t = run(x, 3)
    taps_pcm_same = same_bits(pcm1, pcm1t) and same_bits(pcm3, pcm3t)      # the capture instantiation against the plain one
    assert np.isfinite(pcm1).all() and np.isfinite(taps1).all()
    arrays = {"x_crc": np.array(zlib.crc32(x.tobytes()), dtype=np.uint32), "pcm": pcm1, "vad": vad1, "taps": taps1}
    w3_same = same_bits(pcm1, pcm3) and same_bits(vad1, vad3) and same_bits(taps1, taps3)
    if not w3_same:
        arrays.update({"pcm_w3": pcm3, "vad_w3": vad3, "taps_w3": taps3})
    arrays["w3_same"] = np.array(int(w3_same))
    arrays["taps_pcm_same"] = np.array(int(taps_pcm_same))
    np.savez_compressed(out, **arrays)
    tp = taps1
    print(f"wrote {out}: {os.path.getsize(out)} bytes, w3_same {w3_same}, taps_pcm_same {taps_pcm_same}")
    for b in range(x.shape[1]):
        print(f"stream {b}: silence flags {tp[:, b, 67].astype(int).tolist()} pitch {tp[:, b, 64].astype(int).tolist()} "
              f"vad {np.round(vad1[:, b], 3).tolist()} peak out {np.abs(pcm1[:, b]).max():.1f}")


if __name__ == "__main__":
    main()

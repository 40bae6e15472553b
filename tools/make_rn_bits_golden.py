"""Developer tool, needs the GPU: records what the RNNoise frame kernel computes, bit for bit, so that a change that is
meant to keep every floating-point operation and its order can be held against the commit before it.
    python tools/make_rn_bits_golden.py [out.npz]        (default tests/golden/rn_frame_bits.npz)
Run it at the PARENT of the change; tests/test_gpu_rn_frame_bits.py compares the working tree with the file.

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


def run(x: np.ndarray, waves: int, lib=None):
    """-> (pcm [T,B,480], vad [T,B], taps [T,B,72], pcm of the call with taps) of a fresh handle in the given form."""
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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "rn_frame_bits.npz")
    x = inputs()
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
    for b in range(B):
        print(f"stream {b}: silence flags {tp[:, b, 67].astype(int).tolist()} pitch {tp[:, b, 64].astype(int).tolist()} "
              f"vad {np.round(vad1[:, b], 3).tolist()} peak out {np.abs(pcm1[:, b]).max():.1f}")


if __name__ == "__main__":
    main()

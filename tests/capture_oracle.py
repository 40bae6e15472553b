"""The capture callbacks of the reference's live path restated in Python / numpy for B lock-stepped streams: the per-sample
conversion and downmix of build_input_stream_f32 / _i16 / _u16 (src-tauri/src/audio.rs:732-921), the `shared == None` arm of
push_mono_to_buffers (audio.rs:697-726: the callback's own LinearResampler into the recording ring), and the macOS app-audio
handler's `resample_audio` (src-tauri/src/recording.rs:13-39).

Every f32 operation of the reference is a numpy f32 operation of its own, so each rounds separately, as Rust's do; the f64
position arithmetic is Python float arithmetic.  The bypass arm is built from `crispy_amd.denoise.LinearResampler`, whose
recurrence it runs once for all streams (the positions do not depend on the samples), and `record_oracle.RecordOracle`."""
import math

import numpy as np

from crispy_amd.denoise import LinearResampler
from tests import record_oracle as RO

F32 = np.float32
FORMATS = {"f32": np.float32, "i16": np.int16, "u16": np.uint16}
# Buffer lengths for the end of resample_audio's loop (tests/test_capture_host.py searches for them and checks them):
BRANCH_44K = 441       # at 44.1 kHz: like every buffer of an upsampled stream it ends with `samples[src_index]`, src_index + 1 == n
BRANCH_N = 1025        # at 96 kHz: the last output takes that branch ...
NO_BRANCH_N = 1024     # ... and here it still has a sample behind it


def convert(x: np.ndarray) -> np.ndarray:
    """What the callbacks map over a frame: f32 `s`; i16 `s as f32 / 32768.0` (audio.rs:817); u16
    `(s as f32 - 32768.0) / 32768.0` (audio.rs:882)."""
    if x.dtype == np.float32:
        return x
    if x.dtype == np.int16:
        return x.astype(F32) / F32(32768)
    if x.dtype == np.uint16:
        return (x.astype(F32) - F32(32768)) / F32(32768)
    raise ValueError(f"no capture format {x.dtype}")


def mic_downmix(f: np.ndarray, channels: int) -> np.ndarray:
    """f [B, n * channels] f32 interleaved -> [B, n]: `frame.iter().sum::<f32>() / input_channels as f32` for EVERY channel
    count -- the mic path has no special case for one or two channels.  [UPSTREAM-RECALL] the identity of `Sum for f32` is
    +0.0, as in record_oracle.downmix: the sum starts there and adds in channel order, every add rounded."""
    f = np.asarray(f, dtype=F32).reshape(f.shape[0], -1, channels)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros(f.shape[:2], dtype=F32)
        for c in range(channels):
            acc = acc + f[:, :, c]
        return acc / F32(channels)


def capture_mono(x: np.ndarray, channels: int) -> np.ndarray:
    """x [B, n * channels] of a capture format -> the callback's mono [B, n]."""
    return mic_downmix(convert(x), channels)


def resample_audio(s: np.ndarray, from_rate: int, to_rate: int = 48000) -> np.ndarray:
    """recording.rs:13-39 over the rows of s [B, n]: stateless per buffer, positions in f64."""
    s = np.asarray(s, dtype=F32)
    if from_rate == to_rate:
        return s.copy()
    n = s.shape[1]
    ratio = float(from_rate) / float(to_rate)
    output_len = int(math.ceil(float(n) / ratio))
    cols = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(output_len):
            src_pos = float(i) * ratio
            idx = int(math.floor(src_pos))
            frac = F32(src_pos - float(idx))
            if idx + 1 < n:
                s1, s2 = s[:, idx], s[:, idx + 1]
                cols.append(s1 + (s2 - s1) * frac)
            elif idx < n:
                cols.append(s[:, idx].copy())
    return np.stack(cols, axis=1).astype(F32) if cols else np.zeros((s.shape[0], 0), F32)


def last_output_takes_the_copy_branch(n: int, from_rate: int, to_rate: int = 48000) -> bool:
    """Whether the last output of a buffer of n samples is `samples[src_index]` with src_index + 1 == n."""
    ratio = float(from_rate) / float(to_rate)
    i = int(math.ceil(float(n) / ratio)) - 1
    return int(math.floor(float(i) * ratio)) + 1 == n


def app_at(x: np.ndarray, channels: int, from_rate: int) -> np.ndarray:
    """The macOS app handler: the handlers' downmix (1: the sample, 2: (f0 + f1) / 2.0), then resample_audio to 48 kHz."""
    return resample_audio(RO.downmix(x, channels), from_rate)


def push_app_at(orc: RO.RecordOracle, x: np.ndarray, channels: int, from_rate: int) -> int:
    """One app buffer at from_rate into the oracle's app deque; returns the 48 kHz samples it made."""
    rows = app_at(x, channels, from_rate)
    orc.app_evictions += orc._append(orc.app, rows)
    return rows.shape[1]


class BypassOracle:
    """push_mono_to_buffers with `shared == None` for B streams: every mono sample through the callback's
    LinearResampler(raw_input_rate, 48000), what it emitted appended to the recording deque.  The resampler object is
    denoise.LinearResampler itself, driven with the sample's index so that each emission tells which two samples it
    interpolates; the interpolation is then three numpy f32 operations over the streams."""

    def __init__(self, n_streams: int, raw_input_rate: float, rec: "RO.RecordOracle | None" = None):
        self.n_streams = n_streams
        self.rs = LinearResampler(float(raw_input_rate), 48000.0)
        self.last = np.zeros(n_streams, dtype=F32)       # last_sample of every stream
        self.rec = rec

    def capture(self, mono: np.ndarray) -> np.ndarray:
        """mono [B, n] -> the `out` vectors of audio.rs:711-714 over the n samples, [B, n_out]."""
        mono = np.asarray(mono, dtype=F32)
        cols = []
        passthrough = abs(self.rs.input_rate - self.rs.output_rate) < 1.0
        with np.errstate(invalid="ignore", over="ignore"):
            for m in range(mono.shape[1]):
                sample = mono[:, m]
                if passthrough:
                    cols.append(sample.copy())
                    continue
                ts = []
                # the position recurrence, on a stand-in stream whose last_sample is 0 and whose sample is 1: it emits t itself
                self.rs.last_sample = F32(0.0)
                self.rs.process_sample(1.0, ts.append)
                for t in ts:
                    cols.append(self.last + (sample - self.last) * F32(t))
                self.last = sample.copy()
        out = np.stack(cols, axis=1).astype(F32) if cols else np.zeros((self.n_streams, 0), F32)
        if self.rec is not None and out.shape[1]:
            self.rec.push_mic(np.ascontiguousarray(out))
        return out

"""The playback half of the reference's RnnNoiseProcessor restated in Python / numpy for B lock-stepped streams: the
`output_buf` deque that push_sample fills (src-tauri/src/audio.rs:280-285) and `next_sample` (audio.rs:297-314), plus the
output callback's three sample conversions (audio.rs:613-650).

It is fed with the arrays the pushes returned and never runs the frame kernels.  Every f32 operation is a numpy f32 operation
of its own, so each rounds separately, as Rust's do; `resample_pos` and the step are Python floats (f64)."""
from collections import deque

import numpy as np

F32 = np.float32


class PlaybackOracle:
    def __init__(self, n_streams: int, capture_rate: float, output_rate: float):
        capture_rate, output_rate = F32(capture_rate), F32(output_rate)
        # RnnNoiseProcessor::new (audio.rs:216-240): a rate a whole hertz off 48 kHz is resampled to it
        self.input_rate = F32(48000.0) if abs(float(capture_rate) - 48000.0) >= 1.0 else capture_rate
        self.output_rate = output_rate
        self.max_output_len = int(self.input_rate)          # `as usize`
        self.n_streams = n_streams
        self.buf = deque()                                   # rows [B] f32
        self.pos = 0.0
        self.evictions = self.pops = self.zeros = 0

    def __len__(self):
        return len(self.buf)

    def push(self, out: np.ndarray) -> None:
        """out [B, n]: what one push returned."""
        assert out.dtype == np.float32 and out.shape[0] == self.n_streams
        for i in range(out.shape[1]):
            if len(self.buf) >= self.max_output_len:
                self.buf.popleft()
                self.evictions += 1
            self.buf.append(out[:, i].copy())

    def next_sample(self):
        """-> ([B] f32, live)"""
        zero = np.zeros(self.n_streams, dtype=np.float32)
        if len(self.buf) < 2:
            self.zeros += 1
            return zero, False
        step = float(self.input_rate) / float(self.output_rate)
        while self.pos >= 1.0:
            self.buf.popleft()
            self.pops += 1
            self.pos -= 1.0
            if len(self.buf) < 2:
                self.zeros += 1
                return zero, False
        s0, s1 = self.buf[0], self.buf[1]
        frac = F32(self.pos)
        d = s1 - s0
        p = d * frac
        self.pos += step
        return s0 + p, True

    def pull(self, n_frames: int):
        """-> (samples [B, n_frames] f32, n_live)"""
        out = np.zeros((self.n_streams, n_frames), dtype=np.float32)
        live = 0
        for f in range(n_frames):
            s, ok = self.next_sample()
            out[:, f] = s
            live += ok
        return out, live


def to_i16(s: np.ndarray) -> np.ndarray:
    return np.trunc(np.clip(s, F32(-1), F32(1)) * F32(32767)).astype(np.int16)


def to_u16(s: np.ndarray) -> np.ndarray:
    h = np.clip(s, F32(-1), F32(1)) * F32(0.5)
    u = h + F32(0.5)
    return np.trunc(u * F32(65535)).astype(np.uint16)


def convert(s: np.ndarray, fmt: str, channels: int) -> np.ndarray:
    """[B, n] f32 -> [B, n * channels] of the format, every channel of a frame the same value."""
    v = {"f32": lambda x: x, "i16": to_i16, "u16": to_u16}[fmt](s)
    return np.repeat(v, channels, axis=1)

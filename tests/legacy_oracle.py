"""The Legacy arm of the reference's NsState restated in Python / numpy for B lock-stepped streams: `SharedAudio`
(src-tauri/src/audio.rs:63-72, 136-200) -- push_sample, next_sample, the LCG both share -- and push_mono_to_buffers around any
processor (audio.rs:682-730): the callback's LinearResampler, re-configured and so reset when the rate the processor produces
moved by 1 Hz or more, into the recording deque.

Vectorised across the streams and looped over the samples.  Every f32 operation of the reference is a numpy f32 operation of
its own, so each rounds separately, as Rust's do; positions and steps are Python floats (f64); the LCG is Python integers.
Written on its own, not from crispy_amd.denoise.SharedAudio: tests/test_legacy_host.py compares the two.  The mic side is
tests/record_oracle.py's ring."""
from collections import deque

import numpy as np

from tests import record_oracle as RO

F32 = np.float32
LCG_A, LCG_C, LCG_SEED = 1664525, 1013904223, 0x1234ABCD


def lcg_naive(state: int, n: int) -> int:
    """n steps, one at a time."""
    for _ in range(n):
        state = (state * LCG_A + LCG_C) & 0xFFFFFFFF
    return state


def lcg_after(state: int, n: int) -> int:
    """n steps by squaring the affine map (a, c): for the step counts a loop cannot reach in a test."""
    a, c = LCG_A, LCG_C
    while n:
        if n & 1:
            state = (state * a + c) & 0xFFFFFFFF
        c = ((a + 1) * c) & 0xFFFFFFFF
        a = (a * a) & 0xFFFFFFFF
        n >>= 1
    return state


def noise_of(state: int) -> np.float32:
    """`(rng_state as f32 / u32::MAX as f32) * 2.0 - 1.0`: `as f32` rounds to nearest even, u32::MAX as f32 is 2^32."""
    r = F32(np.uint32(state))
    q = F32(r / F32(4294967296.0))
    d = F32(q * F32(2.0))
    return F32(d - F32(1.0))


class SharedAudioOracle:
    def __init__(self, n_streams: int, input_rate: float, output_rate: float, noisy: bool, volume: float):
        self.n_streams = n_streams
        self.input_rate, self.output_rate = F32(input_rate), F32(output_rate)
        self.max_len = int(self.input_rate)              # `input_rate as usize`
        self.buf = deque()                               # rows [B] f32, RAW samples
        self.pos = 0.0
        self.noisy = noisy
        self.volume = F32(volume)
        self.rng = LCG_SEED
        self.evictions = self.pops = self.zeros = 0

    def __len__(self):
        return len(self.buf)

    def set_volume(self, volume: float) -> None:
        self.volume = F32(min(max(F32(volume), F32(0.0)), F32(1.0)))

    def produced_rate_hz(self) -> float:
        return float(self.input_rate)

    def _noise_term(self) -> np.float32:
        self.rng = (self.rng * LCG_A + LCG_C) & 0xFFFFFFFF
        return F32(noise_of(self.rng) * F32(0.05))

    def push(self, x: np.ndarray) -> np.ndarray:
        """x [B, n] -> what the n push_sample calls returned, [B, n]."""
        x = np.asarray(x, dtype=F32)
        assert x.shape[0] == self.n_streams
        out = np.empty_like(x)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(x.shape[1]):
                if len(self.buf) >= self.max_len:
                    self.buf.popleft()
                    self.evictions += 1
                self.buf.append(x[:, k].copy())
                processed = x[:, k] * self.volume
                if self.noisy:
                    processed = processed + self._noise_term()
                out[:, k] = processed
        return out

    def next_sample(self):
        """-> ([B] f32, live)"""
        zero = np.zeros(self.n_streams, dtype=F32)
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
        with np.errstate(invalid="ignore", over="ignore"):
            d = s1 - s0
            p = d * frac
            sample = s0 + p
            if self.noisy:
                sample = sample + self._noise_term()
            self.pos += step
            return sample * self.volume, True

    def pull(self, n_frames: int):
        """-> (samples [B, n_frames] f32, n_live)"""
        out = np.zeros((self.n_streams, n_frames), dtype=F32)
        live = 0
        for f in range(n_frames):
            s, ok = self.next_sample()
            out[:, f] = s
            live += ok
        return out, live


class CallbackOracle:
    """push_mono_to_buffers behind the processor: the capture stream's `LinearResampler::new(input_rate, 48000)` and the
    recording deque.  `feed` takes what a block of push_sample calls returned and the rate the processor produces; the rates
    are compared only when samples were returned (audio.rs:701-709).  `resets` counts the set_rates calls."""

    def __init__(self, n_streams: int, input_rate: float, rec: "RO.RecordOracle | None" = None):
        self.n_streams = n_streams
        self.rec = rec
        self.rates = (F32(input_rate), F32(48000.0))
        self.resets = 0
        self._fresh()

    def _fresh(self):
        self.last = np.zeros(self.n_streams, dtype=F32)
        self.has_last = False
        self.input_pos = 0.0
        self.next_pos = 0.0

    def feed(self, produced_rate: float, samples: np.ndarray) -> np.ndarray:
        """samples [B, n] -> what the resampler emitted, [B, n_out] (appended to the recording deque if there is one)."""
        samples = np.asarray(samples, dtype=F32)
        if samples.shape[1] == 0:
            return np.zeros((self.n_streams, 0), F32)
        produced = F32(produced_rate)
        if abs(float(self.rates[0]) - float(produced)) >= 1.0 or abs(float(self.rates[1]) - 48000.0) >= 1.0:
            self.rates = (produced, F32(48000.0))
            self.resets += 1
            self._fresh()
        cols = []
        passthrough = abs(float(self.rates[0]) - float(self.rates[1])) < 1.0
        step = float(F32(self.rates[0] / self.rates[1]))
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(samples.shape[1]):
                sample = samples[:, k]
                if passthrough:
                    cols.append(sample.copy())
                    continue
                if not self.has_last:
                    self.last = sample.copy()
                    self.has_last = True
                    self.input_pos = 0.0
                    self.next_pos = 0.0
                    continue
                self.input_pos += 1.0
                while self.next_pos <= self.input_pos:
                    t = F32(self.next_pos - (self.input_pos - 1.0))
                    t = F32(min(max(t, F32(0.0)), F32(1.0)))
                    d = sample - self.last
                    p = d * t
                    cols.append(self.last + p)
                    self.next_pos += step
                self.last = sample.copy()
        out = np.stack(cols, axis=1).astype(F32) if cols else np.zeros((self.n_streams, 0), F32)
        if self.rec is not None and out.shape[1]:
            self.rec.push_mic(np.ascontiguousarray(out))
        return out


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Bit for bit; where the oracle's value is a NaN, any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))

"""The recording leg of the reference's live path restated in Python / numpy for B lock-stepped streams: the recording deque
that push_mono_to_buffers fills (src-tauri/src/audio.rs:701-726) and the app-audio deque of the capture handlers, both with a
cap; the handlers' downmix; the recording worker's loop (src-tauri/src/commands/recording.rs:196-264); the WAV writer's
quantiser (src-tauri/src/recording.rs:101-118); the capture callback's level meter (audio.rs:728-729, 779-781).

It is fed with the arrays the pushes returned and never runs the denoiser.  Every f32 operation of the reference is a numpy f32
operation of its own, so each rounds separately, as Rust's do.  The counters say which branches a schedule went through."""
from collections import deque

import numpy as np

F32 = np.float32
FRAME = 1152                 # frame_size
MAX_DESYNC = 2400            # (recording::SAMPLE_RATE / 20).max(frame_size)
DEFAULT_CAP = 48000 * 10     # recording::SAMPLE_RATE * 10


def quantise(mixed: np.ndarray) -> np.ndarray:
    """`(s.clamp(-1.0, 1.0) * 32767.0) as i16`: the clamp keeps a NaN, `as` truncates toward zero and makes a NaN 0."""
    mixed = np.asarray(mixed, dtype=F32)
    with np.errstate(invalid="ignore"):
        x = np.clip(mixed, F32(-1), F32(1)) * F32(32767)
        nan = np.isnan(x)
        return np.where(nan, 0, np.trunc(np.where(nan, F32(0), x))).astype(np.int16)


def as_transcriber(q: np.ndarray) -> np.ndarray:
    """run_transcription's read-back of channel 0 (commands/transcription.rs:306-313): `s as f32 / 32768.0`."""
    return q.astype(F32) / F32(32768)


def downmix(x: np.ndarray, channels: int) -> np.ndarray:
    """x [B, n * channels] interleaved -> [B, n].  1: the sample; 2: (f0 + f1) / 2.0; more: iter().sum::<f32>() -- from 0.0,
    in order -- / channels as f32."""
    x = np.asarray(x, dtype=F32)
    f = x.reshape(x.shape[0], -1, channels)
    if channels == 1:
        return f[:, :, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if channels == 2:
            return (f[:, :, 0] + f[:, :, 1]) / F32(2)
        acc = np.zeros(f.shape[:2], dtype=F32)
        for c in range(channels):
            acc = acc + f[:, :, c]
        return acc / F32(channels)


def level(x: np.ndarray) -> np.ndarray:
    """x [B, n], n > 0 -> rms [B]: sum = 0.0; per sample sum += mono * mono, frames += 1.0; (sum / frames).sqrt()."""
    x = np.asarray(x, dtype=F32)
    s = np.zeros(x.shape[0], dtype=F32)
    frames = F32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x.shape[1]):
            mono = x[:, k]
            sq = mono * mono
            s = s + sq
            frames = F32(frames + F32(1))
        return np.sqrt(s / frames).astype(F32)


def worker_plan(mic_len: int, app_len: int, max_frames: int):
    """The worker loop on lengths alone -> (n_frames, mic_off[], app_off[] (-1: zeros), mic_left, app_left, counts)."""
    mic_off, app_off = [], []
    mic_pop = app_pop = 0
    counts = dict(mic_trim=0, app_trim=0, zero_app=0, mixed=0, app_left_alone=0)
    while mic_len >= FRAME and len(mic_off) < max_frames:
        if mic_len > app_len + MAX_DESYNC:
            trim = mic_len - app_len - MAX_DESYNC
            mic_pop += trim
            mic_len -= trim
            counts["mic_trim"] += trim
        elif app_len > mic_len + MAX_DESYNC:
            trim = app_len - mic_len - MAX_DESYNC
            app_pop += trim
            app_len -= trim
            counts["app_trim"] += trim
        mic_off.append(mic_pop)
        mic_pop += FRAME
        mic_len -= FRAME
        if app_len >= FRAME:
            app_off.append(app_pop)
            app_pop += FRAME
            app_len -= FRAME
            counts["mixed"] += 1
        else:
            app_off.append(-1)
            counts["zero_app"] += 1
            counts["app_left_alone"] += app_len > 0
    return len(mic_off), mic_off, app_off, mic_len, app_len, counts


class RecordOracle:
    def __init__(self, n_streams: int, cap: int = DEFAULT_CAP):
        self.n_streams = n_streams
        self.cap = cap
        self.mic = deque()          # rows [B] f32
        self.app = deque()
        self.mic_evictions = self.app_evictions = 0
        self.mic_trim = self.app_trim = 0
        self.zero_app_frames = self.mixed_frames = self.app_left_alone = 0

    def buffered(self):
        return len(self.mic), len(self.app)

    def _append(self, buf: deque, rows: np.ndarray) -> int:
        evicted = 0
        for i in range(rows.shape[1]):
            if len(buf) >= self.cap:
                buf.popleft()
                evicted += 1
            buf.append(rows[:, i].copy())
        return evicted

    def push_mic(self, out: np.ndarray) -> None:
        """out [B, n]: what one push returned (the recording resampler passes it through)."""
        assert out.dtype == np.float32 and out.shape[0] == self.n_streams
        self.mic_evictions += self._append(self.mic, out)

    def push_app(self, x: np.ndarray, channels: int) -> None:
        """x [B, n_frames * channels] interleaved app audio at 48 kHz."""
        assert x.dtype == np.float32 and x.shape[0] == self.n_streams
        self.app_evictions += self._append(self.app, downmix(x, channels))

    def frames_ready(self) -> int:
        return worker_plan(len(self.mic), len(self.app), 1 << 62)[0]

    def drain(self, max_frames=None) -> np.ndarray:
        """The worker loop, deque operation by deque operation -> the WAV payload int16 [B, n_frames * 1152 * 2]."""
        frames = []
        zeros = np.zeros(self.n_streams, dtype=F32)
        while len(self.mic) >= FRAME and (max_frames is None or len(frames) < max_frames):
            mic_len, app_len = len(self.mic), len(self.app)
            if mic_len > app_len + MAX_DESYNC:
                for _ in range(mic_len - app_len - MAX_DESYNC):
                    self.mic.popleft()
                    self.mic_trim += 1
            elif app_len > mic_len + MAX_DESYNC:
                for _ in range(app_len - mic_len - MAX_DESYNC):
                    self.app.popleft()
                    self.app_trim += 1
            left = np.stack([self.mic.popleft() if self.mic else zeros for _ in range(FRAME)], axis=1)      # [B, 1152]
            if len(self.app) >= FRAME:
                right = np.stack([self.app.popleft() for _ in range(FRAME)], axis=1)
                self.mixed_frames += 1
            else:
                right = np.zeros_like(left)
                self.zero_app_frames += 1
                self.app_left_alone += len(self.app) > 0
            with np.errstate(invalid="ignore", over="ignore"):
                mixed = left + right
            q = quantise(mixed)
            frames.append(np.repeat(q, 2, axis=1))          # write_samples: L, R interleaved, both the mixed sample
        if not frames:
            return np.zeros((self.n_streams, 0), dtype=np.int16)
        return np.concatenate(frames, axis=1)

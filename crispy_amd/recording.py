"""Host-side mirror of the reference's recording file writer (src-tauri/src/recording.rs:78-130): a 48 kHz, two-channel,
16-bit WAV that takes the frames `DenoiseState.record_drain` (crispy_rn_record_drain, format i16) produced.  The
quantisation `(s.clamp(-1, 1) * 32767.0) as i16` already happened on the device; this only lays the bytes down."""
from __future__ import annotations

import wave

import numpy as np

SAMPLE_RATE = 48000      # recording::SAMPLE_RATE (recording.rs:8)
CHANNELS = 2             # recording::CHANNELS
FRAME_SIZE = 1152        # the worker's frame (commands/recording.rs:196)


class WavWriter:
    """`WavWriter::new` sets up the spec of recording.rs:85-90; `write_frames` is `write_samples` for frames that are already
    interleaved s16; `finalize` closes the file and returns its path."""

    def __init__(self, output_path):
        self.output_path = output_path
        self._w = wave.open(str(output_path), "wb")
        self._w.setnchannels(CHANNELS)
        self._w.setsampwidth(2)
        self._w.setframerate(SAMPLE_RATE)
        self.frames_written = 0

    def write_frames(self, pcm: np.ndarray) -> None:
        """pcm: one stream's drained payload, int16 [n * 2] (L, R interleaved) or [n, 2]."""
        pcm = np.asarray(pcm)
        if pcm.dtype != np.int16 or pcm.size % CHANNELS:
            raise ValueError("write_frames: interleaved int16 stereo frames are required")
        self._w.writeframes(np.ascontiguousarray(pcm).astype("<i2", copy=False).tobytes())
        self.frames_written += pcm.size // CHANNELS

    def finalize(self):
        self._w.close()
        return self.output_path

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._w.close()
        return False

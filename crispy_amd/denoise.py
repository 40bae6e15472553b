"""Host-side mirror of the reference's RNNoise surface, backed by the HIP library.

* `DenoiseState`        -- nnnoiseless::DenoiseState for B streams at once
                           (`new`: src-tauri/src/audio.rs:229, `process_frame`: audio.rs:268).
* `RnnNoiseProcessor`   -- the adapter of audio.rs:202-315 (`push_sample`, x32768, clamp, volume,
                           first-frame drop, optional input LinearResampler), batched: one
                           processor object drives B streams that are pushed in lock step.
                           `push_block` is the same on the device (crispy_rn_push), a block per call.
* `LinearResampler`     -- audio.rs:73-134.

All arithmetic of `process_frame` runs in libcrispy_hip.so on the GPU; nothing here falls back
to a CPU implementation."""
from __future__ import annotations

import ctypes as C
from collections import deque
from typing import Optional

import numpy as np

from . import _native as N

FRAME_SIZE = N.RN_FRAME  # nnnoiseless::FRAME_SIZE


class DenoiseState:
    """B independent `DenoiseState`s living in HBM.

    `process_frame(out, inp)` keeps the reference's argument order and returns the VAD
    probabilities; arrays are [B, 480] (or [480] when B == 1), f32 in int16 range."""

    def __init__(self, weights, n_streams: int = 1, device: int = 0, lib=None):
        """weights: the 87 503-byte int8 blob, or the path of an rnnoise-nu text model file
        (`crispy_rn_create_from_file`).  lib: another build of the library (`_native.load_variant`), tests only."""
        self._L = lib if lib is not None else N.lib()
        self._h = C.c_void_p()
        self.n_streams = int(n_streams)
        self.device = int(device)
        if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
            import os
            N.check(self._L.crispy_rn_create_from_file(os.fsencode(weights), self.n_streams, self.device,
                                                       C.byref(self._h)), self._L)
            return
        w = np.ascontiguousarray(weights, dtype=np.int8)
        N.check(self._L.crispy_rn_create(w.ctypes.data_as(C.c_void_p), w.size, self.n_streams,
                                         self.device, C.byref(self._h)), self._L)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.crispy_rn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference-shaped single tick ------------------------------------------------------
    def process_frame(self, output: np.ndarray, input: np.ndarray):
        x = np.ascontiguousarray(input, dtype=np.float32)
        if x.size != self.n_streams * FRAME_SIZE:
            raise ValueError(f"process_frame: expected {self.n_streams}x{FRAME_SIZE} samples, got {x.size}")
        if output.dtype != np.float32 or not output.flags["C_CONTIGUOUS"] or output.size != x.size:
            raise ValueError("process_frame: output must be a contiguous float32 array of the input's size")
        vad = np.empty(self.n_streams, dtype=np.float32)
        N.check(self._L.crispy_rn_process(self._h, x.ctypes.data, output.ctypes.data, vad.ctypes.data,
                                          1, N.LAYOUT_TBF), self._L)
        return float(vad[0]) if self.n_streams == 1 else vad

    # -- batched host arrays ---------------------------------------------------------------
    def process(self, x: np.ndarray, layout: str = "tbf"):
        """x: [T, B, 480] ('tbf') or [B, T, 480] ('btf') -> (out like x, vad [T, B])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        lay = N.LAYOUT_TBF if layout == "tbf" else N.LAYOUT_BTF
        if x.ndim != 3 or x.shape[2] != FRAME_SIZE:
            raise ValueError("process: x must be [T,B,480] or [B,T,480]")
        T = x.shape[0] if layout == "tbf" else x.shape[1]
        Bn = x.shape[1] if layout == "tbf" else x.shape[0]
        if Bn != self.n_streams:
            raise ValueError(f"process: {Bn} streams given, handle has {self.n_streams}")
        out = np.empty_like(x)
        vad = np.empty((T, Bn), dtype=np.float32)
        N.check(self._L.crispy_rn_process(self._h, x.ctypes.data, out.ctypes.data, vad.ctypes.data, T, lay), self._L)
        return out, vad

    def process_s16(self, x: np.ndarray, layout: str = "tbf", out: np.ndarray | None = None, vad: np.ndarray | None = None):
        """`crispy_rn_process_s16`: int16 PCM [T, B, 480] / [B, T, 480] in -> (int16 out like x, vad [T, B]).  A sample s
        enters process_frame as float(s); the output is trunc(clamp(y / 32768, -1, 1) * 32767) -- the adapter's scaling and
        clamp (audio.rs:270-273) and the WAV writer's quantisation (recording.rs:109-110).  Half the PCIe bytes of `process`."""
        if x.dtype != np.int16 or not x.flags.c_contiguous:
            raise ValueError("process_s16: a C-contiguous int16 array is required")
        lay = N.LAYOUT_TBF if layout == "tbf" else N.LAYOUT_BTF
        if x.ndim != 3 or x.shape[2] != FRAME_SIZE:
            raise ValueError("process_s16: x must be [T,B,480] or [B,T,480]")
        T = x.shape[0] if layout == "tbf" else x.shape[1]
        Bn = x.shape[1] if layout == "tbf" else x.shape[0]
        if Bn != self.n_streams:
            raise ValueError(f"process_s16: {Bn} streams given, handle has {self.n_streams}")
        out = np.empty_like(x) if out is None else out
        vad = np.empty((T, Bn), dtype=np.float32) if vad is None else vad
        if out.dtype != np.int16 or out.shape != x.shape or not out.flags.c_contiguous or vad.shape != (T, Bn):
            raise ValueError("process_s16: out / vad shape or type mismatch")
        N.check(self._L.crispy_rn_process_s16(self._h, x.ctypes.data, out.ctypes.data, vad.ctypes.data, T, lay), self._L)
        return out, vad

    def process_s16_device(self, d_in: int, d_out: int, n_frames: int, d_vad: int = 0, layout: str = "tbf", stream: int = 0):
        lay = N.LAYOUT_TBF if layout == "tbf" else N.LAYOUT_BTF
        N.check(self._L.crispy_rn_process_s16_device(self._h, d_in, d_out, d_vad or None, int(n_frames), lay, stream or None), self._L)

    @staticmethod
    def register_host(arr: np.ndarray):
        """Page-lock a host array the caller reuses across `process` calls (crispy_host_register): copies become DMA."""
        N.check(N.lib().crispy_host_register(arr.ctypes.data, arr.nbytes))

    @staticmethod
    def unregister_host(arr: np.ndarray):
        N.check(N.lib().crispy_host_unregister(arr.ctypes.data))

    def process_into(self, x: np.ndarray, out: np.ndarray, vad: np.ndarray, layout: str = "tbf"):
        """`process` into caller-owned (e.g. registered) arrays: x, out [T,B,480] / [B,T,480] float32 contiguous,
        vad [T,B]."""
        lay = N.LAYOUT_TBF if layout == "tbf" else N.LAYOUT_BTF
        T = x.shape[0] if layout == "tbf" else x.shape[1]
        Bn = x.shape[1] if layout == "tbf" else x.shape[0]
        if x.dtype != np.float32 or out.dtype != np.float32 or not x.flags.c_contiguous or not out.flags.c_contiguous:
            raise ValueError("process_into: float32 C-contiguous arrays required")
        if Bn != self.n_streams or out.shape != x.shape or vad.shape != (T, Bn):
            raise ValueError("process_into: shape mismatch")
        N.check(self._L.crispy_rn_process(self._h, x.ctypes.data, out.ctypes.data, vad.ctypes.data, T, lay), self._L)

    # -- device-resident tensors (torch is only the allocator here) --------------------------
    def process_device(self, d_in: int, d_out: int, n_frames: int, d_vad: int = 0, d_taps: int = 0,
                       layout: str = "tbf", stream: int = 0):
        lay = N.LAYOUT_TBF if layout == "tbf" else N.LAYOUT_BTF
        N.check(self._L.crispy_rn_process_device(self._h, d_in, d_out, d_vad or None, d_taps or None,
                                                 int(n_frames), lay, stream or None), self._L)

    # -- the capture-rate adapter (RnnNoiseProcessor on the device: crispy_rn_adapter_* / crispy_rn_push*) -----
    def adapter_configure(self, input_rate: float, volume: float = 1.0):
        """`RnnNoiseProcessor::new(input_rate, _, volume)` for every stream: fresh adapter and denoiser state."""
        N.check(self._L.crispy_rn_adapter_configure(self._h, float(input_rate), float(volume)), self._L)

    def adapter_set_volume(self, volume: float):
        N.check(self._L.crispy_rn_adapter_set_volume(self._h, float(volume)), self._L)

    def adapter_produced_rate_hz(self) -> float:
        r = C.c_float()
        N.check(self._L.crispy_rn_adapter_produced_rate_hz(self._h, C.byref(r)), self._L)
        return r.value

    def push_out_len(self, n_in: int) -> int:
        """Samples per stream the NEXT push of n_in samples returns."""
        n = self._L.crispy_rn_push_out_len(self._h, int(n_in))
        if n < 0:
            N.check(int(n), self._L)
        return int(n)

    def push(self, x: np.ndarray, want_vad: bool = False):
        """`crispy_rn_push`: x [B, n] raw capture samples in +-1 at the configured rate -> out [B, n_out] (and, with
        want_vad, the VAD probabilities [frames, B] of the frames this push completed)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.n_streams:
            raise ValueError(f"push: x must be [{self.n_streams}, n]")
        n_in = x.shape[1]
        n_out = self.push_out_len(n_in)
        out = np.empty((self.n_streams, n_out), dtype=np.float32)
        # frames completed: those returned, and the dropped first one if this push completes it
        vad = np.full((n_out // FRAME_SIZE + 1, self.n_streams), np.nan, dtype=np.float32) if want_vad else None
        got = C.c_long()
        N.check(self._L.crispy_rn_push(self._h, x.ctypes.data, n_in, n_in, out.ctypes.data, max(n_out, 1),
                                       vad.ctypes.data if want_vad else None, C.byref(got)), self._L)
        assert got.value == n_out
        if want_vad:
            return out, vad[~np.isnan(vad[:, 0])]
        return out

    def push_device(self, d_in: int, in_stride: int, n_in: int, d_out: int, out_stride: int, d_frames48: int = 0,
                    frames_stride: int = 0, d_vad: int = 0, stream: int = 0) -> int:
        """`crispy_rn_push_device` on device pointers; returns n_out (known on return, the work is only enqueued)."""
        got = C.c_long()
        N.check(self._L.crispy_rn_push_device(self._h, d_in, int(in_stride), int(n_in), d_out, int(out_stride),
                                              d_frames48 or None, int(frames_stride), d_vad or None, C.byref(got),
                                              stream or None), self._L)
        return int(got.value)

    def last_push_ms(self):
        """With `set_timing(True)`: device time of (rn_adapt_in_kernel, rn_adapt_out_kernel) of the last push."""
        a, b = C.c_float(), C.c_float()
        N.check(self._L.crispy_rn_last_push_ms(self._h, C.byref(a), C.byref(b)), self._L)
        return a.value, b.value

    # -- the playback half (output_buf / next_sample on the device: crispy_rn_playback_* / crispy_rn_pull*) -----
    PCM = {"f32": (N.PCM_F32, np.float32), "i16": (N.PCM_I16, np.int16), "u16": (N.PCM_U16, np.uint16)}

    def playback_configure(self, output_rate: float):
        """A fresh `output_buf` (one second at the effective input rate) and `resample_pos = 0`; from here on every push
        feeds the ring.  Leaves the denoiser and the capture side of the adapter alone."""
        N.check(self._L.crispy_rn_playback_configure(self._h, float(output_rate)), self._L)

    def playback_buffered(self) -> int:
        """`output_buf.len()`, the same for every stream."""
        n = self._L.crispy_rn_playback_buffered(self._h)
        if n < 0:
            N.check(int(n), self._L)
        return int(n)

    def pull(self, n_frames: int, channels: int = 1, fmt: str = "f32", want_live: bool = False):
        """`crispy_rn_pull`: n_frames calls of `next_sample` per stream, converted as the output callback does and written
        to `channels` interleaved channels -> [B, n_frames * channels] of float32 / int16 / uint16 (and, with want_live,
        how many of the frames were real samples, not underrun zeros)."""
        code, dtype = self.PCM[fmt]
        n = int(n_frames) * int(channels)
        out = np.empty((self.n_streams, max(n, 0)), dtype=dtype)
        live = C.c_long()
        N.check(self._L.crispy_rn_pull(self._h, int(n_frames), int(channels), code, out.ctypes.data, max(n, 1),
                                       C.byref(live)), self._L)
        return (out, int(live.value)) if want_live else out

    def pull_device(self, n_frames: int, d_out: int, out_stride: int, channels: int = 1, fmt: str = "f32", stream: int = 0) -> int:
        """`crispy_rn_pull_device` on a device pointer; returns n_live (known on return, the work is only enqueued)."""
        live = C.c_long()
        N.check(self._L.crispy_rn_pull_device(self._h, int(n_frames), int(channels), self.PCM[fmt][0], d_out, int(out_stride),
                                              C.byref(live), stream or None), self._L)
        return int(live.value)

    # -- the recording leg (rec ring, app ring, worker, s16 frames, level meter: crispy_rn_record_* / crispy_rn_level*) -----
    REC_FRAME = N.REC_FRAME

    def record_configure(self, ring_samples: int = 0):
        """`start_recording`: empty mic and app rings of `ring_samples` per stream (0 = the reference's ten seconds); from
        here on every push that returns samples feeds the mic ring.  Leaves denoiser, adapter and playback ring alone."""
        N.check(self._L.crispy_rn_record_configure(self._h, int(ring_samples)), self._L)

    def record_app_push(self, x: np.ndarray, channels: int = 1, from_rate: Optional[int] = None):
        """`crispy_rn_record_app_push`: x [B, n_frames * channels] interleaved app audio at 48 kHz, downmixed on the device
        and appended to the app ring.  With from_rate (`crispy_rn_record_app_push_at`): audio at that rate, resampled to
        48 kHz as the handler's `resample_audio` does (recording.rs:13-39), buffer by buffer, in the same kernel."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.n_streams or x.shape[1] % int(channels):
            raise ValueError(f"record_app_push: x must be [{self.n_streams}, n_frames * channels]")
        if from_rate is None:
            N.check(self._L.crispy_rn_record_app_push(self._h, x.ctypes.data, max(x.shape[1], 1), x.shape[1] // int(channels),
                                                      int(channels)), self._L)
        else:
            N.check(self._L.crispy_rn_record_app_push_at(self._h, x.ctypes.data, max(x.shape[1], 1), x.shape[1] // int(channels),
                                                         int(channels), int(from_rate)), self._L)

    def record_app_push_device(self, d_in: int, in_stride: int, n_frames: int, channels: int = 1, stream: int = 0,
                               from_rate: Optional[int] = None):
        if from_rate is None:
            N.check(self._L.crispy_rn_record_app_push_device(self._h, d_in, int(in_stride), int(n_frames), int(channels),
                                                             stream or None), self._L)
        else:
            N.check(self._L.crispy_rn_record_app_push_at_device(self._h, d_in, int(in_stride), int(n_frames), int(channels),
                                                                int(from_rate), stream or None), self._L)

    # -- the capture callback itself (format, downmix, level, arm: crispy_rn_capture* / crispy_rn_bypass_configure) -----
    def bypass_configure(self, raw_input_rate: float):
        """Noise suppression off, recording on -- the `shared == None` arm of push_mono_to_buffers (audio.rs:697-714) with a
        fresh `LinearResampler(raw_input_rate, 48000)`: from here on `capture` resamples the raw mono instead of denoising it.
        0 returns to the RNNoise arm.  Pushes, pulls, the denoiser and the playback ring are not affected."""
        N.check(self._L.crispy_rn_bypass_configure(self._h, float(raw_input_rate)), self._L)

    def capture_out_len(self, n_frames: int) -> int:
        """Samples per stream the NEXT capture of n_frames frames returns."""
        n = self._L.crispy_rn_capture_out_len(self._h, int(n_frames))
        if n < 0:
            N.check(int(n), self._L)
        return int(n)

    def capture(self, x: np.ndarray, channels: int = 1):
        """`crispy_rn_capture`, one capture callback: x [B, n_frames * channels] interleaved frames as the device hands them
        out -- float32, int16 or uint16, uploaded as they are -- -> (out [B, n_out], rms [B]): conversion, the mic downmix
        (`iter().sum::<f32>() / channels`), the level meter and the handle's arm, all on the device."""
        fmt = {np.dtype(np.float32): N.PCM_F32, np.dtype(np.int16): N.PCM_I16, np.dtype(np.uint16): N.PCM_U16}.get(x.dtype)
        if fmt is None:
            raise ValueError("capture: x must be float32, int16 or uint16")
        x = np.ascontiguousarray(x)
        if x.ndim != 2 or x.shape[0] != self.n_streams or x.shape[1] % int(channels):
            raise ValueError(f"capture: x must be [{self.n_streams}, n_frames * channels]")
        n_frames = x.shape[1] // int(channels)
        n_out = self.capture_out_len(n_frames)
        out = np.empty((self.n_streams, n_out), dtype=np.float32)
        rms = np.zeros(self.n_streams, dtype=np.float32)
        got = C.c_long()
        N.check(self._L.crispy_rn_capture(self._h, x.ctypes.data, max(x.shape[1], 1), n_frames, int(channels), fmt,
                                          out.ctypes.data, max(n_out, 1), rms.ctypes.data, C.byref(got)), self._L)
        assert got.value == n_out
        return out, rms

    def capture_device(self, d_in: int, in_stride: int, n_frames: int, channels: int, fmt: str, d_out: int, out_stride: int,
                       d_mono: int = 0, mono_stride: int = 0, d_rms: int = 0, stream: int = 0) -> int:
        """`crispy_rn_capture_device` on device pointers; returns n_out (known on return, the work is only enqueued)."""
        got = C.c_long()
        N.check(self._L.crispy_rn_capture_device(self._h, d_in, int(in_stride), int(n_frames), int(channels), self.PCM[fmt][0],
                                                 d_out, int(out_stride), d_mono or None, int(mono_stride), d_rms or None,
                                                 C.byref(got), stream or None), self._L)
        return int(got.value)

    # -- the model switch and NsState's Legacy arm (crispy_rn_model_configure / crispy_rn_model) -----
    MODELS = {"rnnnoise": N.NS_RNNOISE, "dummy": N.NS_DUMMY, "noisy": N.NS_NOISY}

    def model_configure(self, model):
        """`set_monitoring_model` (audio.rs:942-967): a fresh processor of that model -- "rnnnoise", "dummy", "noisy" or a
        CRISPY_NS_* code -- at the configured capture rate, the current volume and the configured output rate.  From here on
        push, pull and capture are that processor's: for a Legacy model `SharedAudio` (audio.rs:136-200)."""
        code = self.MODELS[model] if isinstance(model, str) else int(model)
        N.check(self._L.crispy_rn_model_configure(self._h, code), self._L)

    def model(self) -> int:
        """The handle's model, a CRISPY_NS_* code (`_native.NS_*`)."""
        m = C.c_int()
        N.check(self._L.crispy_rn_model(self._h, C.byref(m)), self._L)
        return int(m.value)

    def level(self, x: np.ndarray) -> np.ndarray:
        """`crispy_rn_level`: the callback's level meter over x [B, n], `(sum(mono * mono) / n).sqrt()` per stream with the
        reference's f32 rounding; n == 0 gives zeros (the callback emits nothing then)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] != self.n_streams:
            raise ValueError(f"level: x must be [{self.n_streams}, n]")
        rms = np.zeros(self.n_streams, dtype=np.float32)
        N.check(self._L.crispy_rn_level(self._h, x.ctypes.data, max(x.shape[1], 1), x.shape[1], rms.ctypes.data), self._L)
        return rms

    def level_device(self, d_in: int, in_stride: int, n_in: int, d_rms: int, stream: int = 0):
        N.check(self._L.crispy_rn_level_device(self._h, d_in, int(in_stride), int(n_in), d_rms, stream or None), self._L)

    def record_buffered(self):
        """(mic, app): samples per stream in the two rings."""
        mic, app = C.c_long(), C.c_long()
        N.check(self._L.crispy_rn_record_buffered(self._h, C.byref(mic), C.byref(app)), self._L)
        return int(mic.value), int(app.value)

    def record_frames_ready(self) -> int:
        """1152-sample frames a drain without a limit would write now."""
        n = self._L.crispy_rn_record_frames_ready(self._h)
        if n < 0:
            N.check(int(n), self._L)
        return int(n)

    def record_drain(self, max_frames: Optional[int] = None, fmt: str = "i16") -> np.ndarray:
        """`crispy_rn_record_drain`: the worker loop for at most max_frames frames (None: all that are ready).  'i16': the
        WAV payload [B, n_frames * 1152 * 2] int16, L == R; 'f32': channel 0 as the transcriber reads it, [B, n_frames * 1152]."""
        if fmt not in ("i16", "f32"):
            raise ValueError("record_drain: fmt is 'i16' or 'f32'")
        code, dtype = self.PCM[fmt]
        ready = self.record_frames_ready()
        n = ready if max_frames is None else min(ready, int(max_frames))
        per = N.REC_FRAME * (2 if fmt == "i16" else 1)
        out = np.empty((self.n_streams, max(n, 0) * per), dtype=dtype)
        if n <= 0:
            return out
        got = C.c_long()
        N.check(self._L.crispy_rn_record_drain(self._h, n, code, out.ctypes.data, n * per, C.byref(got)), self._L)
        assert got.value == n
        return out

    def record_drain_device(self, max_frames: int, d_out: int, out_stride: int, fmt: str = "i16", stream: int = 0) -> int:
        """`crispy_rn_record_drain_device` on a device pointer; returns the frames written (known on return)."""
        got = C.c_long()
        N.check(self._L.crispy_rn_record_drain_device(self._h, int(max_frames), self.PCM[fmt][0], d_out, int(out_stride),
                                                      C.byref(got), stream or None), self._L)
        return int(got.value)

    def stage_tansig_device(self, d_x: int, d_y: int, n: int, sigmoid: bool = False):
        """tansig_approx / sigmoid_approx as the frame kernel evaluates them (stage entry point for parity tests)."""
        N.check(self._L.crispy_rn_stage_tansig_device(self._h, d_x, d_y, int(n), int(sigmoid), None), self._L)

    def synchronize(self):
        N.check(self._L.crispy_rn_synchronize(self._h), self._L)

    def reset(self, stream: int = -1):
        N.check(self._L.crispy_rn_reset(self._h, int(stream)), self._L)

    def set_timing(self, enable: bool):
        N.check(self._L.crispy_rn_set_timing(self._h, int(enable)), self._L)

    def last_kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        N.check(self._L.crispy_rn_last_kernel_ms(self._h, C.byref(a), C.byref(b)), self._L)
        return a.value, b.value

    def debug_capture(self, enable: bool):
        N.check(self._L.crispy_rn_debug_capture(self._h, int(enable)), self._L)

    def debug_read(self, stream: int) -> np.ndarray:
        d = np.empty(N.RN_DBG_FLOATS, dtype=np.float32)
        N.check(self._L.crispy_rn_debug_read(self._h, int(stream), d.ctypes.data_as(C.POINTER(C.c_float)), d.size), self._L)
        return d


class LinearResampler:
    """Streaming 2-tap linear interpolation resampler (audio.rs:73-134)."""

    def __init__(self, input_rate: float, output_rate: float):
        self.input_rate = np.float32(input_rate)
        self.output_rate = np.float32(output_rate)
        self.last_sample = np.float32(0.0)
        self.has_last = False
        self.input_pos = 0.0
        self.next_output_pos = 0.0

    def rates(self):
        return float(self.input_rate), float(self.output_rate)

    def set_rates(self, input_rate: float, output_rate: float):
        self.__init__(input_rate, output_rate)

    def process_sample(self, sample, emit):
        sample = np.float32(sample)
        if abs(self.input_rate - self.output_rate) < 1.0:
            emit(sample)
            return
        if not self.has_last:
            self.last_sample = sample
            self.has_last = True
            self.input_pos = 0.0
            self.next_output_pos = 0.0
            return
        self.input_pos += 1.0
        step = float(np.float32(self.input_rate / self.output_rate))
        while self.next_output_pos <= self.input_pos:
            t = np.float32(self.next_output_pos - (self.input_pos - 1.0))
            t = np.float32(min(max(t, np.float32(0.0)), np.float32(1.0)))
            emit(np.float32(self.last_sample + (sample - self.last_sample) * t))
            self.next_output_pos += step
        self.last_sample = sample


class RnnNoiseProcessor:
    """audio.rs:202-315 for B lock-stepped streams: `push_sample(samples[B])` returns None or an
    array [n, B] of denoised samples (n = 480 per completed frame), scaled and clamped exactly
    as the reference does (x32768 in, /32768 + clamp(-1, 1) * volume out, first frame dropped)."""

    def __init__(self, weights: np.ndarray, input_rate: float, output_rate: float, volume: float,
                 n_streams: int = 1, device: int = 0):
        if abs(input_rate - 48000.0) >= 1.0:
            self.input_rate = 48000.0
            self.input_resamplers: Optional[list] = [LinearResampler(input_rate, 48000.0) for _ in range(n_streams)]
        else:
            self.input_rate = float(input_rate)
            self.input_resamplers = None
        self.output_rate = float(output_rate)
        self.volume = float(min(max(volume, 0.0), 1.0))
        self.n_streams = n_streams
        self.first_frame = True
        self.max_output_len = int(self.input_rate)
        self.denoise = DenoiseState(weights, n_streams, device)
        self.denoise.adapter_configure(input_rate, self.volume)     # the device form of all of the above: push_block
        self.denoise.playback_configure(output_rate)                # ... and of output_buf / resample_pos: pull_block
        self.input_buf: deque = deque()
        self.output_buf: deque = deque()
        self.resample_pos = 0.0

    def set_volume(self, volume: float):
        self.volume = float(min(max(volume, 0.0), 1.0))
        self.denoise.adapter_set_volume(self.volume)

    def produced_rate_hz(self) -> float:
        return self.input_rate

    def push_block(self, x: np.ndarray) -> np.ndarray:
        """A loop of `push_sample` over the columns of x [B, n], as one `crispy_rn_push`: resampler, framing, scaling,
        process_frame, clamp, volume and the first-frame drop all run on the device.  Returns [B, n_out] (n_out = 480 per
        completed frame; possibly 0).  The carried samples and the resampler state live in the handle, those of
        `push_sample` in this object: drive a processor through one of the two.  The samples returned also go to the
        handle's playback ring, which `pull_block` reads; `next_sample` reads the ring `push_sample` fills."""
        return self.denoise.push(x)

    def pull_block(self, n: int) -> np.ndarray:
        """n calls of `next_sample` as one `crispy_rn_pull`, reading what `push_block` buffered: [B, n] float32."""
        return self.denoise.pull(n)

    def push_sample(self, samples) -> Optional[np.ndarray]:
        samples = np.atleast_1d(np.asarray(samples, dtype=np.float32))
        if samples.size != self.n_streams:
            raise ValueError("push_sample: one sample per stream")
        rows = []
        if self.input_resamplers is not None:
            per_stream = [[] for _ in range(self.n_streams)]
            for b, rs in enumerate(self.input_resamplers):
                rs.process_sample(samples[b], per_stream[b].append)
            for k in range(len(per_stream[0])):  # lock-stepped streams emit equal counts
                rows.append(np.array([per_stream[b][k] for b in range(self.n_streams)], dtype=np.float32))
        else:
            rows.append(samples)
        acc = []
        for row in rows:
            if len(self.input_buf) >= self.max_output_len:
                self.input_buf.popleft()
            self.input_buf.append(row)
            if len(self.input_buf) >= FRAME_SIZE:
                frame = np.stack([self.input_buf.popleft() for _ in range(FRAME_SIZE)], axis=1)  # [B,480]
                frame = np.ascontiguousarray(frame * np.float32(32768.0))
                out = np.empty_like(frame)
                self.denoise.process_frame(out, frame)
                out = np.clip(out / np.float32(32768.0), -1.0, 1.0).astype(np.float32) * np.float32(self.volume)
                if self.first_frame:
                    self.first_frame = False
                    continue
                for i in range(FRAME_SIZE):
                    if len(self.output_buf) >= self.max_output_len:
                        self.output_buf.popleft()
                    self.output_buf.append(out[:, i])
                acc.append(out.T)
        if not acc:
            return None
        return np.concatenate(acc, axis=0)

    def next_sample(self) -> np.ndarray:
        zero = np.zeros(self.n_streams, dtype=np.float32)
        if len(self.output_buf) < 2:
            return zero
        step = self.input_rate / self.output_rate
        while self.resample_pos >= 1.0:
            self.output_buf.popleft()
            self.resample_pos -= 1.0
            if len(self.output_buf) < 2:
                return zero
        s0, s1 = self.output_buf[0], self.output_buf[1]
        frac = np.float32(self.resample_pos)
        self.resample_pos += step
        return (s0 + (s1 - s0) * frac).astype(np.float32)


class SharedAudio:
    """`SharedAudio` (audio.rs:63-72, 136-200), the processor of NsState's Legacy arm, sample by sample for B lock-stepped
    streams: every f32 operation of the reference is a numpy f32 operation of its own, in the reference's order.  `model` is
    "dummy" or "noisy" (`ModelKind::from_name`: anything but "noisy" is Dummy).  One LCG serves `push_sample` and
    `next_sample` and is the same for every stream.  The device form is `NsState` below."""

    def __init__(self, input_rate: float, output_rate: float, model: str, volume: float, n_streams: int = 1):
        self.input_rate = np.float32(input_rate)
        self.output_rate = np.float32(output_rate)
        self.max_len = int(self.input_rate)          # `input_rate as usize`: the raw capture rate
        self.buffer: deque = deque()
        self.resample_pos = 0.0
        self.noisy = model == "noisy"
        self.volume = np.float32(volume)
        self.rng_state = 0x1234ABCD
        self.n_streams = n_streams

    def _noise(self) -> np.float32:
        self.rng_state = (self.rng_state * 1664525 + 1013904223) & 0xFFFFFFFF
        r = np.float32(np.uint32(self.rng_state))            # `as f32`: to nearest even
        return np.float32(np.float32(r / np.float32(4294967296.0)) * np.float32(2.0) - np.float32(1.0))

    def push_sample(self, samples) -> np.ndarray:
        """One sample per stream -> `Some(vec![processed])` as an array [1, B]."""
        samples = np.atleast_1d(np.asarray(samples, dtype=np.float32))
        if samples.size != self.n_streams:
            raise ValueError("push_sample: one sample per stream")
        if len(self.buffer) >= self.max_len:
            self.buffer.popleft()
        self.buffer.append(samples.copy())
        with np.errstate(invalid="ignore", over="ignore"):
            processed = samples * self.volume
            if self.noisy:
                processed = processed + np.float32(self._noise() * np.float32(0.05))
        return processed.astype(np.float32)[None, :]

    def next_sample(self) -> np.ndarray:
        zero = np.zeros(self.n_streams, dtype=np.float32)
        if len(self.buffer) < 2:
            return zero
        step = float(self.input_rate) / float(self.output_rate)
        while self.resample_pos >= 1.0:
            self.buffer.popleft()
            self.resample_pos -= 1.0
            if len(self.buffer) < 2:
                return zero
        s0, s1 = self.buffer[0], self.buffer[1]
        frac = np.float32(self.resample_pos)
        with np.errstate(invalid="ignore", over="ignore"):
            sample = s0 + (s1 - s0) * frac
            if self.noisy:
                sample = sample + np.float32(self._noise() * np.float32(0.05))
            self.resample_pos += step
            return (sample * self.volume).astype(np.float32)


class NsState:
    """`NsState` (audio.rs:317-358) over one handle for B lock-stepped streams: the processor behind the capture and the
    output callbacks, whichever model it is, with `set_monitoring_model` (audio.rs:942-967) as `set_model`.  Everything runs on
    the device; `push_sample` / `next_sample` are blocks of one, so `CaptureBuffers.push_mono` takes it as it takes a
    per-sample processor."""

    def __init__(self, weights: np.ndarray, input_rate: float, output_rate: float, volume: float, n_streams: int = 1,
                 device: int = 0, model: str = "rnnnoise"):
        self.n_streams = n_streams
        self.denoise = DenoiseState(weights, n_streams, device)
        self.denoise.adapter_configure(input_rate, float(min(max(volume, 0.0), 1.0)))
        self.denoise.playback_configure(output_rate)
        if model != "rnnnoise":
            self.set_model(model)

    def set_model(self, name: str) -> None:
        """A fresh processor of the named model at the remembered rates and the current volume, also when it is unchanged:
        "rnnnoise", "noisy", anything else is the dummy (`ModelKind::from_name`)."""
        self.denoise.model_configure(name if name in ("rnnnoise", "noisy") else "dummy")

    def model(self) -> int:
        return self.denoise.model()

    def set_volume(self, volume: float) -> None:
        self.denoise.adapter_set_volume(float(min(max(volume, 0.0), 1.0)))

    def produced_rate_hz(self) -> float:
        """RNNoise: the effective rate (48000 when it resamples); Legacy: the raw capture rate."""
        return self.denoise.adapter_produced_rate_hz()

    def push_block(self, x: np.ndarray) -> np.ndarray:
        """A loop of `push_sample` over the columns of x [B, n] as one `crispy_rn_push` -> [B, n_out]."""
        return self.denoise.push(x)

    def pull_block(self, n: int, channels: int = 1, fmt: str = "f32") -> np.ndarray:
        """n calls of `next_sample` and the output callback's conversion as one `crispy_rn_pull`."""
        return self.denoise.pull(n, channels, fmt)

    def push_sample(self, samples) -> Optional[np.ndarray]:
        samples = np.atleast_1d(np.asarray(samples, dtype=np.float32))
        out = self.denoise.push(samples.reshape(self.n_streams, 1))
        return out.T if out.shape[1] else None

    def next_sample(self) -> np.ndarray:
        return self.denoise.pull(1)[:, 0]


REC_SAMPLE_RATE = 48000          # recording::SAMPLE_RATE (recording.rs:8)


class CaptureBuffers:
    """`push_mono_to_buffers` (audio.rs:682-730), the per-sample glue of the capture callback: feed the mono sample
    to the noise suppressor (or pass it through when none is active), resample whatever it produced to the 48 kHz
    recording rate with the caller's `LinearResampler` -- re-configured only when a rate changed by >= 1 Hz --,
    append to the recording ring (10 s cap, oldest dropped), and accumulate the level meter's sum / count
    (`rms()` is the `(sum / frames).sqrt()` of audio.rs:780)."""

    def __init__(self):
        self.rec_resampler = LinearResampler(float(REC_SAMPLE_RATE), float(REC_SAMPLE_RATE))
        self.rec_buffer = deque()
        self.max_len = REC_SAMPLE_RATE * 10
        self.sum = np.float32(0.0)
        self.frames = np.float32(0.0)

    def push_mono(self, mono: float, ns: "RnnNoiseProcessor | NsState | SharedAudio | None", raw_input_rate_hz: float) -> None:
        """ns: any processor with `produced_rate_hz` and `push_sample` -- with an `NsState` the rate follows the model, so a
        switch from RNNoise at 44.1 kHz (produces 48000) to a Legacy model (produces 44100) resets the recording resampler at
        the first Legacy sample, and dummy <-> noisy at one rate does not."""
        mono = np.float32(mono)
        if ns is not None:
            produced_rate = float(ns.produced_rate_hz())
            out = ns.push_sample([mono])
            samples = None if out is None else out[:, 0]
        else:
            produced_rate = float(raw_input_rate_hz)
            samples = np.array([mono], dtype=np.float32)
        if samples is not None:
            cur_in, cur_out = self.rec_resampler.rates()
            if abs(cur_in - produced_rate) >= 1.0 or abs(cur_out - REC_SAMPLE_RATE) >= 1.0:
                self.rec_resampler.set_rates(produced_rate, float(REC_SAMPLE_RATE))
            emitted = []
            for s in samples:
                self.rec_resampler.process_sample(s, emitted.append)
            for o in emitted:
                if len(self.rec_buffer) >= self.max_len:
                    self.rec_buffer.popleft()
                self.rec_buffer.append(np.float32(o))
        self.sum = np.float32(self.sum + mono * mono)
        self.frames = np.float32(self.frames + np.float32(1.0))

    # -- block form: one capture callback as one call, rings and level meter on the device ------------------------------
    @staticmethod
    def start_block(ns: "RnnNoiseProcessor", ring_samples: int = 0) -> None:
        """`start_recording` for the block form: empty mic and app rings in the processor's handle (0 = ten seconds)."""
        ns.denoise.record_configure(ring_samples)

    @staticmethod
    def push_mono_block(x: np.ndarray, ns: "RnnNoiseProcessor"):
        """A capture callback over the columns of x [B, n] as `crispy_rn_push` + `crispy_rn_level`: the samples the
        suppressor returned ([B, n_out], appended to the handle's recording ring on the device, which `drain_block` reads)
        and the callback's rms per stream.  The RNNoise arm only: its recording resampler always passes through."""
        return ns.push_block(x), ns.denoise.level(x)

    @staticmethod
    def capture_block(x: np.ndarray, ns: "RnnNoiseProcessor", channels: int = 1):
        """The whole capture callback as one `crispy_rn_capture`: x [B, n_frames * channels] in the device's own format
        (float32 / int16 / uint16) -> what `push_mono_block` returns for the mono of these frames.  After
        `ns.denoise.bypass_configure(rate)` it is the `ns=None` arm of `push_mono` instead: the raw mono resampled to 48 kHz."""
        return ns.denoise.capture(x, channels)

    @staticmethod
    def drain_block(ns: "RnnNoiseProcessor", max_frames: Optional[int] = None, fmt: str = "i16") -> np.ndarray:
        """The recording worker's loop body for the frames that are ready: see `DenoiseState.record_drain`."""
        return ns.denoise.record_drain(max_frames, fmt)

    def rms(self) -> float:
        return float(np.sqrt(self.sum / self.frames)) if self.frames > 0 else 0.0

    def reset_level(self) -> None:
        self.sum = np.float32(0.0)
        self.frames = np.float32(0.0)

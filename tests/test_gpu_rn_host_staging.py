"""GPU test of the one host-pointer staging set of the RNNoise handle (crispy_amd/csrc/rn_handle.h: stage_in, stage_out,
stage_aux).  Every entry point that takes host arrays -- crispy_rn_process, crispy_rn_process_s16, crispy_rn_push,
crispy_rn_pull, crispy_rn_record_app_push, crispy_rn_level, crispy_rn_record_drain -- copies through the same three device
buffers and synchronises before it returns.  What must hold: no call sees another call's data, whatever the buffers held
before and whether a call found them too small (freed and allocated again) or larger than it needs.

The device forms take the caller's buffers and never touch the staging set, so they are the reference here: the same calls on
a second handle through torch tensors must give the same bits."""
import numpy as np
import pytest

from tests.playback_oracle import PlaybackOracle

pytestmark = pytest.mark.gpu

FRAME = 480
REC_FRAME = 1152
CAPTURE, PLAYBACK, REC_RING = 44100.0, 32000.0, 2304


def _mk(B):
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState
    ds = DenoiseState(synthetic_weights(0), B, 0)
    ds.adapter_configure(CAPTURE, 0.8)
    ds.playback_configure(PLAYBACK)
    ds.record_configure(REC_RING)
    return ds


def _audio(B, n_frames, first_stream=0):
    """Seeded synth_audio, [B, n_frames * 480] in +-1."""
    from crispy_amd import synth_audio
    x = synth_audio.batch_np(B, n_frames, first_stream)             # [T, B, 480]
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(B, n_frames * FRAME))


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class _Device:
    """The same calls as DenoiseState's host forms, through the *_device entry points on torch tensors."""

    def __init__(self, ds):
        import torch
        self.t, self.ds, self.B = torch, ds, ds.n_streams

    def _up(self, x):
        d = self.t.from_numpy(np.ascontiguousarray(x)).cuda()
        self.t.cuda.synchronize()
        return d

    def _new(self, shape, dtype):
        d = self.t.zeros(shape, dtype=dtype, device="cuda")
        self.t.cuda.synchronize()
        return d

    def _down(self, *tensors):
        self.ds.synchronize()
        return [d.cpu().numpy() for d in tensors]

    def process(self, x, s16=False):
        T = x.shape[0]
        d_x, d_out, d_vad = self._up(x), self._new(x.shape, self.t.int16 if s16 else self.t.float32), self._new((T, self.B), self.t.float32)
        (self.ds.process_s16_device if s16 else self.ds.process_device)(d_x.data_ptr(), d_out.data_ptr(), T, d_vad.data_ptr())
        return self._down(d_out, d_vad)

    def push(self, x):
        n_in, n_out = x.shape[1], self.ds.push_out_len(x.shape[1])
        frames = n_out // FRAME + 1
        d_x, d_out = self._up(x), self._new((self.B, max(n_out, 1)), self.t.float32)
        d_vad = self.t.full((frames, self.B), float("nan"), device="cuda")
        self.t.cuda.synchronize()
        got = self.ds.push_device(d_x.data_ptr(), n_in, n_in, d_out.data_ptr(), max(n_out, 1), d_vad=d_vad.data_ptr())
        assert got == n_out
        out, vad = self._down(d_out, d_vad)
        return out[:, :n_out], vad[~np.isnan(vad[:, 0])]

    def level(self, x):
        d_x, d_rms = self._up(x), self._new((self.B,), self.t.float32)
        self.ds.level_device(d_x.data_ptr(), x.shape[1], x.shape[1], d_rms.data_ptr())
        return self._down(d_rms)[0]

    def pull(self, n, channels, fmt):
        d_out = self._new((self.B, n * channels), {"f32": self.t.float32, "i16": self.t.int16}[fmt])
        live = self.ds.pull_device(n, d_out.data_ptr(), n * channels, channels, fmt)
        return self._down(d_out)[0], live

    def app_push(self, x, channels):
        d_x = self._up(x)
        self.ds.record_app_push_device(d_x.data_ptr(), x.shape[1], x.shape[1] // channels, channels)
        self.ds.synchronize()

    def drain(self, fmt):
        n = self.ds.record_frames_ready()
        d_out = self._new((self.B, max(n, 1) * REC_FRAME * 2), self.t.int16)
        got = self.ds.record_drain_device(n, d_out.data_ptr(), max(n, 1) * REC_FRAME * 2, fmt) if n else 0
        return self._down(d_out)[0][:, :got * REC_FRAME * 2], got


def test_host_forms_in_any_order_equal_the_device_forms():
    """Handle A through the host-pointer forms only, in an order in which every staging buffer is used by calls of different
    sizes and kinds in turn (bytes per buffer for 3 streams, in / out / aux):
      process 1 frame 5760 / 5760 / 12; push 1500 18000 / 11520 / 36; level 480 5760 / - / 12; pull 64 x 2 i16 - / 768 / -;
      app_push 1200 x 2 28800 / - / -; process 3 frames 17280 / 17280 / 36; push 500 6000 / 5760 / 12; pull 700 f32 - / 8400 / -;
      drain i16 - / 13824 / -; process_s16 2 frames 11520 (5760 used) / the same / 24.
    Handle B gets the same calls through the device forms.  Every returned array, count and VAD value is the same, bit for bit."""
    B = 3
    a, ds_b = _mk(B), _mk(B)
    b = _Device(ds_b)
    x = _audio(B, 8)
    frames = lambda t0, T: np.ascontiguousarray((x[:, t0 * FRAME:(t0 + T) * FRAME] * np.float32(32768.0)).reshape(B, T, FRAME).transpose(1, 0, 2))
    app = _audio(B, 5, first_stream=20)[:, :2400]
    seen = []

    def check(what, got, want):
        for i, (g, w) in enumerate(zip(got, want)):
            if isinstance(w, np.ndarray):
                assert _same(g, w), (what, i, g.shape, w.shape)
            else:
                assert g == w, (what, i, g, w)
        seen.append(what)

    check("process 1", a.process(frames(0, 1)), b.process(frames(0, 1)))
    check("push 1500", a.push(x[:, 480:1980], want_vad=True), b.push(x[:, 480:1980]))
    check("level 480", [a.level(x[:, 2000:2480])], [b.level(x[:, 2000:2480])])
    check("pull 64 x 2 i16", a.pull(64, 2, "i16", want_live=True), b.pull(64, 2, "i16"))
    a.record_app_push(app, 2)
    b.app_push(app, 2)
    check("app_push 1200 x 2", a.record_buffered(), ds_b.record_buffered())
    check("process 3", a.process(frames(5, 3)), b.process(frames(5, 3)))
    check("push 500", a.push(x[:, 2500:3000], want_vad=True), b.push(x[:, 2500:3000]))
    check("pull 700 f32", a.pull(700, 1, "f32", want_live=True), b.pull(700, 1, "f32"))
    ready = a.record_frames_ready()
    got_b, n_b = b.drain("i16")
    check("drain i16", [a.record_drain(fmt="i16"), ready], [got_b, n_b])
    s16 = np.ascontiguousarray(np.clip(frames(3, 2), -32768.0, 32767.0).astype(np.int16))
    check("process_s16 2", a.process_s16(s16), b.process(s16, s16=True))
    check("lengths", [a.playback_buffered(), *a.record_buffered(), a.push_out_len(1000)],
          [ds_b.playback_buffered(), *ds_b.record_buffered(), ds_b.push_out_len(1000)])
    # the calls did something: every step compared, and a frame was drained
    assert ready >= 1 and n_b == ready and len(seen) == 11
    a.close()
    ds_b.close()


def test_a_pipelined_process_between_a_push_and_a_pull():
    """crispy_rn_process cuts a call of 8 MB or more into pieces that flow through three streams and a copy-out thread; 64
    streams x 72 frames (8.4 MiB of f32; 69 frames is where the path begins) takes that path and makes all three staging buffers
    larger than the push before it and the pull after it need.  It equals process_device on a handle with the same history bit
    for bit, and the pull after it equals the playback oracle's on what the push returned."""
    B, T = 64, 72
    a, ds_b = _mk(B), _mk(B)
    x = _audio(B, T + 4)
    orc = PlaybackOracle(B, CAPTURE, PLAYBACK)
    out = a.push(x[:, :1500])
    assert _same(out, ds_b.push(x[:, :1500])) and out.shape[1] == 2 * FRAME
    orc.push(out)
    big = np.ascontiguousarray((x[:, 4 * FRAME:] * np.float32(32768.0)).reshape(B, T, FRAME).transpose(1, 0, 2))
    assert big.nbytes >= 8 << 20
    got, vad = a.process(big)
    want, want_vad = _Device(ds_b).process(big)
    assert _same(got, want) and _same(vad, want_vad)
    assert np.abs(got).max() > 100.0                               # the frames went through the denoiser, not around it
    pulled, live = a.pull(600, 1, "f32", want_live=True)           # 900 of the 960 samples the push left in the ring
    ref, ref_live = orc.pull(600)
    assert live == ref_live == 600 and a.playback_buffered() == len(orc)
    for s in range(B):
        assert _same(pulled[s], ref[s]), ("stream", s, np.nonzero(pulled[s] != ref[s])[0][:8])
    a.close()
    ds_b.close()

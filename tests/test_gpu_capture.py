"""GPU tests of the capture callbacks, crispy_rn_capture* / crispy_rn_bypass_configure / crispy_rn_record_app_push_at*
(include/crispy_hip.h): the device's frames to mono (src-tauri/src/audio.rs:732-921), the level meter, the RNNoise arm (a push
on the mono) and the `shared == None` arm (audio.rs:697-726), and the app-audio handler at the stream's own rate
(src-tauri/src/recording.rs:13-39), for every stream of a handle at once.

Everything is compared on the bytes: against tests/capture_oracle.py, against the per-sample `CaptureBuffers.push_mono`, and
against a second handle that is driven through the calls a capture replaces."""
import ctypes as C

import numpy as np
import pytest

from tests import capture_oracle as CO
from tests import record_oracle as RO

pytestmark = pytest.mark.gpu

FRAME = RO.FRAME       # 1152
INVALID = -1           # CRISPY_ERR_INVALID_ARG


def _mk(B, capture_rate=None, ring_samples=None, output_rate=None, bypass=None):
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState
    ds = DenoiseState(synthetic_weights(0), B, 0)
    if capture_rate is not None:
        ds.adapter_configure(capture_rate, 0.9)
    if output_rate is not None:
        ds.playback_configure(output_rate)
    if ring_samples is not None:
        ds.record_configure(ring_samples)
    if bypass is not None:
        ds.bypass_configure(bypass)
    return ds


def _raw(fmt, B, n_elems, seed):
    """Frames as a device of that format hands them out: the whole integer range with both ends in it; floats in +-1 with
    both zeros in them, the last stream at amplitude 3."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        x = rng.uniform(-1.0, 1.0, size=(B, n_elems)).astype(np.float32)
        x[-1] *= np.float32(3.0)
        x[:, ::7] = np.float32(-0.0)
        x[:, 3::11] = np.float32(0.0)
        return x
    lo, hi = (-32768, 32768) if fmt == "i16" else (0, 65536)
    x = rng.integers(lo, hi, size=(B, n_elems)).astype(CO.FORMATS[fmt])
    x[:, ::13] = lo
    x[:, 5::17] = hi - 1
    return x


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    for b in range(want.shape[0]):
        assert _same(got[b], want[b]), (what, "stream", b, np.nonzero(got[b] != want[b])[0][:8])


def _to_device(x, stride):
    """x [B, n] of any capture format -> a byte tensor holding rows of `stride` elements, the rest of a row poisoned."""
    import torch
    item = x.dtype.itemsize
    rows = np.full((x.shape[0], stride * item), 0x7f, dtype=np.uint8)
    rows[:, :x.shape[1] * item] = np.ascontiguousarray(x).view(np.uint8)
    return torch.from_numpy(rows).cuda()


def _capture_device(ds, x, channels, fmt, stride, n_out_room, want_mono=True, want_rms=True):
    """One crispy_rn_capture_device over device copies -> (out [B, n_out], mono [B, n] or None, rms [B] or None)."""
    import torch
    B, n = x.shape[0], x.shape[1] // channels
    d_in = _to_device(x, stride)
    assert d_in.data_ptr() % 16 == 0
    d_out = torch.full((B, max(n_out_room, 1)), float("nan"), dtype=torch.float32, device="cuda")
    d_mono = torch.full((B, n + 3), float("nan"), dtype=torch.float32, device="cuda") if want_mono else None
    d_rms = torch.full((B,), float("nan"), dtype=torch.float32, device="cuda") if want_rms else None
    n_out = ds.capture_device(d_in.data_ptr(), stride, n, channels, fmt, d_out.data_ptr(), d_out.shape[1],
                              d_mono.data_ptr() if want_mono else 0, n + 3, d_rms.data_ptr() if want_rms else 0)
    ds.synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(out[:, n_out:]).all()                      # nothing behind the samples of this capture is written
    mono = None
    if want_mono:
        mono = d_mono.cpu().numpy()
        assert np.isnan(mono[:, n:]).all()
        mono = np.ascontiguousarray(mono[:, :n])
    return np.ascontiguousarray(out[:, :n_out]), mono, (d_rms.cpu().numpy() if want_rms else None)


def _strides(n_elems, itemsize):
    """(a stride whose rows stay 16-byte aligned, an odd one: the 16-byte loads and the fallback)."""
    per16 = 16 // itemsize
    aligned = (n_elems + per16 - 1) // per16 * per16
    odd = n_elems + 1 if n_elems % 2 == 0 else n_elems + 2
    return aligned, odd


# ---- 1: a capture equals the three calls it replaces -----------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("fmt", ["f32", "i16", "u16"])
def test_capture_equals_conversion_level_and_push(fmt, B):
    """Channels 1, 2, 3, 8 x frames 1, 441, 1023, 1025 (the kernel's tile is 1024) x (aligned rows, odd stride) on one pair of
    handles: `cap` gets crispy_rn_capture_device, `ref` the oracle's mono through crispy_rn_level and crispy_rn_push.  70 streams
    cross the level kernel's 64-stream tile."""
    import torch
    cap, ref = _mk(B, 44100.0), _mk(B, 44100.0)
    side = _mk(B, bypass=48000.0)          # noise suppression off at 48 kHz: d_out is the mono
    seed, returned = 0, 0
    for channels in (1, 2, 3, 8):
        for n in (1, 441, 1023, 1025):
            x = _raw(fmt, B, n * channels, seed)
            seed += 1
            want_mono = CO.capture_mono(x, channels)
            want_rms = ref.level(want_mono)
            want_out = ref.push(want_mono)
            aligned, odd = _strides(n * channels, x.dtype.itemsize)
            assert cap.capture_out_len(n) == want_out.shape[1]
            out, mono, rms = _capture_device(cap, x, channels, fmt, aligned, want_out.shape[1] + 5)
            what = (fmt, B, channels, n)
            _check_rows(mono, want_mono, what + ("mono",))
            assert _same(rms, want_rms), what
            _check_rows(out, want_out, what + ("out",))
            returned += out.shape[1]
            # the same frames through the fallback loads: the same mono bits (a handle of its own, so that `cap` stays in step)
            d_in = _to_device(x, odd)
            d_mono = torch.full((B, n), float("nan"), dtype=torch.float32, device="cuda")
            d_out = torch.empty((B, 4096), dtype=torch.float32, device="cuda")
            assert side.capture_device(d_in.data_ptr(), odd, n, channels, fmt, d_out.data_ptr(), 4096, d_mono.data_ptr(), n) == n
            side.synchronize()
            _check_rows(d_mono.cpu().numpy(), want_mono, what + ("mono, odd stride",))
            _check_rows(d_out.cpu().numpy()[:, :n], want_mono, what + ("bypass at 48 kHz passes the mono through",))
    assert returned >= 20 * 480
    # a mono f32 -0.0 becomes +0.0 (on the bytes above, where the data has them); the hand-checked vector once more
    z = np.full((B, 4), -0.0, np.float32)
    _, mono, _ = _capture_device(side, z, 1, "f32", 4, 5)
    assert not np.signbit(mono).any() and np.signbit(z).all()
    cap.close(), ref.close(), side.close()


@pytest.mark.parametrize("rate", [44100.0, 48000.0])
def test_state_behind_captures_is_the_pushs(rate):
    """Five captures of mixed sizes and formats with playback and recording configured, then a pull and a drain: the two
    handles agree, so what a capture left behind (carry, resampler, rings) is what the pushes left."""
    B = 3
    cap, ref = _mk(B, rate, 2304, 32000.0), _mk(B, rate, 2304, 32000.0)
    plan = [("i16", 2, 441), ("f32", 1, 1025), ("u16", 3, 1), ("i16", 1, 2000), ("f32", 8, 1500)]
    for k, (fmt, channels, n) in enumerate(plan):
        x = _raw(fmt, B, n * channels, 100 + k)
        mono = CO.capture_mono(x, channels)
        want_rms, want = ref.level(mono), ref.push(mono)
        if k % 2:
            got, rms = cap.capture(x, channels)                # the host-pointer form
        else:
            aligned, odd = _strides(n * channels, x.dtype.itemsize)
            got, _, rms = _capture_device(cap, x, channels, fmt, odd if k == 2 else aligned, want.shape[1] + 1, want_mono=False)
        _check_rows(got, want, ("capture", k))
        assert _same(rms, want_rms), k
        assert cap.playback_buffered() == ref.playback_buffered() and cap.record_buffered() == ref.record_buffered(), k
    assert cap.playback_buffered() > 2000 and cap.record_buffered()[0] == 2304         # the mic ring evicted
    assert cap.push_out_len(480) == ref.push_out_len(480)
    got, live = cap.pull(700, 2, "i16", want_live=True)
    want, want_live = ref.pull(700, 2, "i16", want_live=True)
    assert live == want_live > 0
    _check_rows(got, want, "pull")
    _check_rows(cap.record_drain(None, "f32"), ref.record_drain(None, "f32"), "drain")
    assert cap.record_buffered() == ref.record_buffered()
    cap.close(), ref.close()


def test_host_form_equals_device_form():
    B = 3
    for fmt, channels, n in (("i16", 1, 1030), ("i16", 2, 441), ("u16", 4, 257), ("f32", 3, 1024), ("f32", 2, 5)):
        dev, host = _mk(B, 44100.0), _mk(B, 44100.0)
        for rnd in range(2):
            x = _raw(fmt, B, n * channels, 200 + rnd)
            aligned, _ = _strides(n * channels, x.dtype.itemsize)
            out_d, _, rms_d = _capture_device(dev, x, channels, fmt, aligned, dev.capture_out_len(n) + 2)
            out_h, rms_h = host.capture(x, channels)
            _check_rows(out_h, out_d, (fmt, channels, n, rnd))
            assert _same(rms_h, rms_d)
        assert out_d.shape[1] > 0 or n < 480          # (five frames complete no frame: there the level is what is compared)
        dev.close(), host.close()


# ---- 2: the bypass arm -----------------------------------------------------------------------------------------------------
BYPASS_CAPTURES = (1, 2, 441, 1024, 7, 441)


@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("rate", [44100.0, 16000.0, 47999.5, 48000.0])
def test_bypass_equals_the_per_sample_arm(rate, B):
    """Six captures, so that has_last and the position carry cross calls, into a ring of 2304 samples, so that it evicts.
    d_out / n_out against the oracle for every stream and against `CaptureBuffers.push_mono(ns=None)`, sample by sample, for the
    first and the last one; then the f32 drain."""
    from crispy_amd.denoise import CaptureBuffers
    cap_ring = 2304
    ds = _mk(B, 44100.0, cap_ring, bypass=rate)
    orc = CO.BypassOracle(B, rate, RO.RecordOracle(B, cap_ring))
    per_sample = {b: CaptureBuffers() for b in (0, B - 1)}
    for cb in per_sample.values():
        cb.max_len = 1 << 40           # keeps everything it emitted: the ring's eviction is the record oracle's business
    total = 0
    for k, n in enumerate(BYPASS_CAPTURES):
        fmt, channels = (("f32", 1), ("i16", 2), ("u16", 1))[k % 3]
        x = _raw(fmt, B, n * channels, 300 + k)
        mono = CO.capture_mono(x, channels)
        want = orc.capture(mono)
        assert ds.capture_out_len(n) == want.shape[1], (k, n)
        if k % 2:
            got, rms = ds.capture(x, channels)
        else:
            aligned, odd = _strides(n * channels, x.dtype.itemsize)
            got, got_mono, rms = _capture_device(ds, x, channels, fmt, odd if k == 4 else aligned, want.shape[1] + 3)
            _check_rows(got_mono, mono, ("mono", k))
        _check_rows(got, want, ("bypass", rate, k))
        assert _same(rms, RO.level(mono)), k
        for b, cb in per_sample.items():
            for v in mono[b]:
                cb.push_mono(v, None, rate)
            emitted = np.array(cb.rec_buffer, np.float32)
            assert _same(emitted[total:], got[b]), (rate, k, b)
        total += got.shape[1]
        assert ds.record_buffered() == orc.rec.buffered() == (min(total, cap_ring), 0)
    if abs(rate - 48000.0) < 1.0:
        assert total == sum(BYPASS_CAPTURES)
    assert (orc.rec.mic_evictions > 0) == (rate == 16000.0)         # three samples out per sample in: 5745 into 2304
    want = RO.as_transcriber(orc.rec.drain()[:, 0::2])
    got = ds.record_drain(None, "f32")
    assert want.shape[1] >= FRAME
    _check_rows(got, want, ("drain", rate))
    assert ds.record_buffered() == orc.rec.buffered()
    ds.close()


def test_bypass_evicts_from_the_ring():
    """16 kHz in, three 48 kHz samples out per capture sample: 1024 captured samples overfill a ring of 2304."""
    B, cap_ring = 3, 2304
    ds = _mk(B, None, cap_ring, bypass=16000.0)
    orc = CO.BypassOracle(B, 16000.0, RO.RecordOracle(B, cap_ring))
    for k, n in enumerate((1024, 300)):
        x = _raw("i16", B, n, 400 + k)
        got, _ = ds.capture(x, 1)
        _check_rows(got, orc.capture(CO.capture_mono(x, 1)), k)
    assert orc.rec.mic_evictions > 1000 and ds.record_buffered() == orc.rec.buffered() == (cap_ring, 0)
    _check_rows(ds.record_drain(None, "f32"), RO.as_transcriber(orc.rec.drain()[:, 0::2]), "drain")
    ds.close()


def test_bypass_leaves_the_denoiser_alone():
    """A bypassed capture between two pushes: the second push returns what it returns on a handle that never bypassed, the
    playback ring has not moved, and crispy_rn_bypass_configure(0) is the RNNoise arm again."""
    B = 3
    x = _raw("f32", B, 3000, 500)
    a, b = _mk(B, 44100.0, 4608, 48000.0), _mk(B, 44100.0, 4608, 48000.0)
    _check_rows(a.push(x[:, :1000]), b.push(x[:, :1000]), "first push")
    a.bypass_configure(44100.0)
    before = a.playback_buffered()
    raw = _raw("i16", B, 2 * 700, 501)
    got, _ = a.capture(raw, 2)
    _check_rows(got, CO.BypassOracle(B, 44100.0).capture(CO.capture_mono(raw, 2)), "bypassed capture")
    assert a.playback_buffered() == before and a.push_out_len(1000) == b.push_out_len(1000)
    assert a.record_buffered()[0] == b.record_buffered()[0] + got.shape[1]
    _check_rows(a.push(x[:, 1000:2000]), b.push(x[:, 1000:2000]), "second push")
    a.bypass_configure(0.0)
    got, rms = a.capture(np.ascontiguousarray(x[:, 2000:]), 1)
    mono = CO.capture_mono(x[:, 2000:], 1)
    _check_rows(got, b.push(mono), "capture after leaving the arm")
    assert _same(rms, b.level(mono)) and got.shape[1] > 0
    _check_rows(a.pull(500), b.pull(500), "pull")
    a.close(), b.close()


# ---- 3: app audio at the stream's own rate ---------------------------------------------------------------------------------
def _fill_mic(ds, orc, B, n):
    """n zeros into the mic ring through a bypassed capture at 48 kHz (it passes through), so that a drain shows the app ring."""
    z = np.zeros((B, n), np.float32)
    got, _ = ds.capture(z, 1)
    assert got.shape == (B, n)
    orc.push_mic(got)


@pytest.mark.parametrize("B", [3, 70])
@pytest.mark.parametrize("from_rate", [44100, 32000, 96000])
def test_app_push_at_a_rate_equals_resample_audio(from_rate, B):
    """Buffers of 1, 2, 441, 1024, 1025 frames and the lengths whose last output does / does not copy the last sample, in 1,
    2 and 5 channels; the ring through f32 drains against the oracle.  The ring of 2304 evicts at 44.1 and 32 kHz."""
    assert CO.BRANCH_44K == 441
    cap_ring = 2304
    ds = _mk(B, None, cap_ring, bypass=48000.0)
    orc = RO.RecordOracle(B, cap_ring)
    made = 0
    for k, n in enumerate((1, 2, CO.BRANCH_44K, CO.NO_BRANCH_N, CO.BRANCH_N, 600)):
        channels = (1, 2, 5)[k % 3]
        x = _raw("f32", B, n * channels, 600 + k) * np.float32(0.5)
        if k % 2:
            ds.record_app_push(x, channels, from_rate=from_rate)
        else:
            import torch
            d = torch.from_numpy(x).cuda()
            ds.record_app_push_device(d.data_ptr(), x.shape[1], n, channels, from_rate=from_rate)
            ds.synchronize()
        made += CO.push_app_at(orc, x, channels, from_rate)
        assert ds.record_buffered() == orc.buffered(), (k, n)
    assert made > 1000 and (orc.app_evictions > 0) == (from_rate != 96000), (made, orc.app_evictions)
    _fill_mic(ds, orc, B, len(orc.app))
    want = RO.as_transcriber(orc.drain()[:, 0::2])
    assert want.shape[1] >= FRAME and np.abs(want).max() > 0.2
    _check_rows(ds.record_drain(None, "f32"), want, ("drain", from_rate))
    assert ds.record_buffered() == orc.buffered()
    ds.close()


def test_app_push_at_48000_is_the_existing_entry_point():
    B = 3
    a, b = _mk(B, None, 2304, bypass=48000.0), _mk(B, None, 2304, bypass=48000.0)
    for k, (n, channels) in enumerate(((1025, 2), (700, 1), (900, 5))):
        x = _raw("f32", B, n * channels, 700 + k)
        a.record_app_push(x, channels, from_rate=48000)
        b.record_app_push(x, channels)
        assert a.record_buffered() == b.record_buffered()
    z = np.zeros((B, 2304), np.float32)
    a.capture(z, 1), b.capture(z, 1)
    got, want = a.record_drain(None, "f32"), b.record_drain(None, "f32")
    assert want.shape[1] == 2 * FRAME and np.abs(want).max() > 0.2
    _check_rows(got, want, "drain")
    a.close(), b.close()


# ---- 4: rejections ---------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_handle_as_it_was():
    import torch
    from crispy_amd import _native as N
    B, n = 3, 600
    bad, good = _mk(B, 44100.0, 2304, 48000.0), _mk(B, 44100.0, 2304, 48000.0)
    L = bad._L
    x = _raw("i16", B, 2 * n, 800)
    d_in = _to_device(x, 2 * n)
    d_out = torch.zeros((B, 4096), dtype=torch.float32, device="cuda")
    d_mono = torch.zeros((B, 4096), dtype=torch.float32, device="cuda")       # (room for d_out too: the overlap case)
    app = torch.zeros((B, 2 * n), dtype=torch.float32, device="cuda")
    got = C.c_long(-5)

    def capture(in_stride=2 * n, n_frames=n, channels=2, fmt=N.PCM_I16, out_stride=4096, mono=d_mono.data_ptr(), mono_stride=4096, out=d_out.data_ptr()):
        return L.crispy_rn_capture_device(bad._h, d_in.data_ptr(), in_stride, n_frames, channels, fmt, out, out_stride, mono, mono_stride,
                                          None, C.byref(got), None)

    def rejected(rc, what):
        assert rc == INVALID, (what, rc)
        msg = L.crispy_last_error().decode()
        assert msg.startswith("crispy_rn_"), (what, msg)
        return msg

    first = _raw("i16", B, 2 * 1000, 801)          # behind the dropped first frame: the captures below return samples
    _check_rows(bad.capture(first, 2)[0], good.capture(first, 2)[0], "first capture")
    for arm in ("rnnoise", "bypass"):
        if arm == "bypass":
            bad.bypass_configure(44100.0), good.bypass_configure(44100.0)
        assert "format" in rejected(capture(fmt=3), "unknown format") and "format" in rejected(capture(fmt=-1), "format -1")
        assert "channels" in rejected(capture(channels=0), "0 channels") and "channels" in rejected(capture(channels=9), "9 channels")
        assert "in_stride" in rejected(capture(in_stride=2 * n - 1), "short in_stride")
        assert "mono_stride" in rejected(capture(mono_stride=n - 1), "short mono_stride")
        need = good.capture_out_len(n)
        assert need > 0 and "out_stride" in rejected(capture(out_stride=need - 1), "short out_stride")
        assert "n_frames" in rejected(capture(n_frames=-1), "negative count")
        assert "n_frames" in rejected(capture(n_frames=(1 << 24) + 1, in_stride=1 << 26, mono_stride=1 << 25), "too many frames")
        rejected(capture(out=None), "NULL d_out")
        assert "overlaps" in rejected(capture(out=d_mono.data_ptr()), "d_out on d_mono")
        rejected(L.crispy_rn_capture(bad._h, None, 2 * n, n, 2, N.PCM_I16, x.ctypes.data, 4096, None, C.byref(got)), "NULL in")
        assert got.value == 0
        assert capture(n_frames=0) == 0 and got.value == 0                     # a no-op
        for rate in (0, -44100, 7999, 384001):
            assert "from_rate" in rejected(L.crispy_rn_record_app_push_at_device(bad._h, app.data_ptr(), 2 * n, n, 2, rate, None), rate)
        assert "channels" in rejected(L.crispy_rn_record_app_push_at_device(bad._h, app.data_ptr(), 2 * n, n, 9, 44100, None), "app channels")
        assert "in_stride" in rejected(L.crispy_rn_record_app_push_at_device(bad._h, app.data_ptr(), 2 * n - 1, n, 2, 44100, None), "app stride")
        assert "n_frames" in rejected(L.crispy_rn_record_app_push_at_device(bad._h, app.data_ptr(), 2 * n, -1, 2, 44100, None), "app count")
        for rate in (-1.0, float("nan"), float("inf")):
            rejected(L.crispy_rn_bypass_configure(bad._h, rate), ("bypass rate", rate))
        assert bad.capture_out_len(n) == need and bad.record_buffered() == good.record_buffered()
        assert bad.playback_buffered() == good.playback_buffered()
        # a valid call on both: as if the rejected ones had never happened
        for rnd in range(2):
            y = _raw("i16", B, 2 * n, 810 + rnd)
            out_b, rms_b = bad.capture(y, 2)
            out_g, rms_g = good.capture(y, 2)
            _check_rows(out_b, out_g, (arm, rnd))
            assert _same(rms_b, rms_g) and out_b.shape[1] > 0
        a = _raw("f32", B, 2 * n, 820)
        bad.record_app_push(a, 2, from_rate=44100), good.record_app_push(a, 2, from_rate=44100)
        assert bad.record_buffered() == good.record_buffered()
    plain = _mk(B)
    assert "not configured" in rejected(L.crispy_rn_record_app_push_at_device(plain._h, app.data_ptr(), 2 * n, n, 2, 44100, None), "no recording")
    _check_rows(bad.record_drain(None, "f32"), good.record_drain(None, "f32"), "drain")
    bad.close(), good.close(), plain.close()

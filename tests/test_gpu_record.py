"""GPU tests of the recording leg, crispy_rn_record_* / crispy_rn_level* (include/crispy_hip.h): the recording ring that
push_mono_to_buffers fills (src-tauri/src/audio.rs:701-726), the app-audio ring and the handlers' downmix, the recording
worker's loop (src-tauri/src/commands/recording.rs:196-264), WavWriter's quantisation (src-tauri/src/recording.rs:101-118) and
the callback's level meter (audio.rs:728-729, 779-781), for every stream of a handle at once.

Everything is compared on the bytes against tests/record_oracle.py, which is fed the arrays the pushes returned."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import record_oracle as RO

pytestmark = pytest.mark.gpu

FRAME = RO.FRAME       # 1152
PUSH = 1000            # capture samples per round
ROUNDS = 16
APP = {4: 4000, 5: 4000, 6: 4000, 14: 1000, 15: 1000, 16: 1000}     # app samples per round, 0 elsewhere
NO_DRAIN = (9, 10, 11, 12)
ONE_FRAME = 13         # the round whose drain has max_frames = 1


def _mk(B, capture_rate=None, ring_samples=None, output_rate=None):
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState
    ds = DenoiseState(synthetic_weights(0), B, 0)
    if capture_rate is not None:
        ds.adapter_configure(capture_rate, 1.0)
    if ring_samples is not None:
        ds.record_configure(ring_samples)
    if output_rate is not None:
        ds.playback_configure(output_rate)
    return ds


def _data(B, n, seed=0):
    """Every stream its own random samples in +-0.5; the last stream at amplitude 1.5, so that the clamp has work."""
    x = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(B, n)).astype(np.float32)
    x[-1] *= np.float32(3.0)
    return x


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    for b in range(want.shape[0]):
        assert _same(got[b], want[b]), (what, "stream", b, np.nonzero(got[b] != want[b])[0][:8])


# ---- 1 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _schedule(capture_rate):
    B = 3
    x = _data(B, ROUNDS * PUSH)
    app = _data(B, sum(APP.values()), seed=1)
    ds = _mk(B, capture_rate, 0 if capture_rate == 48000.0 else 20000)
    orc = RO.RecordOracle(B, RO.DEFAULT_CAP if capture_rate == 48000.0 else 20000)
    log, a0 = [], 0
    for r in range(1, ROUNDS + 1):
        out = ds.push(np.ascontiguousarray(x[:, (r - 1) * PUSH:r * PUSH]))
        orc.push_mic(out)
        na = APP.get(r, 0)
        if na:
            blk = np.ascontiguousarray(app[:, a0:a0 + na])
            a0 += na
            ds.record_app_push(blk, 1)
            orc.push_app(blk, 1)
        rec = dict(round=r, ready=ds.record_frames_ready(), want_ready=orc.frames_ready(), before=ds.record_buffered(),
                   want_before=orc.buffered(), got=None, want=None)
        if r not in NO_DRAIN:
            limit = 1 if r == ONE_FRAME else None
            rec["got"] = ds.record_drain(limit)
            rec["want"] = orc.drain(limit)
        rec["after"], rec["want_after"] = ds.record_buffered(), orc.buffered()
        log.append(rec)
    ds.close()
    counts = dict(mic_trim=orc.mic_trim, app_trim=orc.app_trim, zero_app=orc.zero_app_frames, mixed=orc.mixed_frames,
                  app_left_alone=orc.app_left_alone)
    return tuple(log), counts


@pytest.mark.parametrize("capture_rate", [48000.0, 44100.0])
def test_schedule_equals_the_oracle(capture_rate):
    """16 rounds of (push 1000 capture samples, app push, drain): the app source runs ahead in rounds 4-6 (app trims), is
    silent before and after (frames of zeros), nothing is drained in rounds 9-12 (the mic runs ahead: a mic trim) and round 13
    takes one frame only, with fewer than 1152 app samples in the ring, which stay there.  At 44100 the input resampler is in
    and the rings are 20000 samples."""
    log, counts = _schedule(capture_rate)
    for p in log:
        n = -1 if p["want"] is None else p["want"].shape[1] // (2 * FRAME)
        print(f"[rn record] {capture_rate:.0f} round {p['round']}: ready {p['ready']} ({p['want_ready']}), buffered {p['before']} "
              f"({p['want_before']}), drained {n} frames, left {p['after']} ({p['want_after']})")
    print(f"[rn record] {capture_rate:.0f} oracle counts: {counts}")
    total = 0
    for p in log:
        assert p["ready"] == p["want_ready"] and p["before"] == p["want_before"] and p["after"] == p["want_after"], p["round"]
        if p["want"] is not None:
            _check_rows(p["got"], p["want"], ("round", p["round"]))
            total += p["want"].shape[1] // (2 * FRAME)
    # what the schedule is for, on the oracle's own counts, so that a changed schedule cannot silently lose a branch
    assert all(v > 0 for v in counts.values()), counts
    by = {p["round"]: p for p in log}
    assert by[ONE_FRAME]["want"].shape[1] == 2 * FRAME and by[ONE_FRAME]["want_ready"] > 1
    assert 0 < by[ONE_FRAME]["want_after"][1] < FRAME and by[ONE_FRAME]["want_after"][1] == by[ONE_FRAME]["want_before"][1]
    assert total == counts["zero_app"] + counts["mixed"] and any(p["want"].any() for p in log if p["want"] is not None)


# ---- 2 -------------------------------------------------------------------------------------------------------------
def test_eviction_and_wrap():
    B, cap = 3, 3000
    x = _data(B, 5 * PUSH, seed=2)
    app = _data(B, 5000 + 700, seed=3)
    ds = _mk(B, 48000.0, cap)
    orc = RO.RecordOracle(B, cap)
    for r in range(4):                                   # 480 + 3 x 960 = 3360 samples into a ring of 3000
        orc.push_mic(ds.push(np.ascontiguousarray(x[:, r * PUSH:(r + 1) * PUSH])))
    assert orc.mic_evictions == 360 and ds.record_buffered() == orc.buffered() == (cap, 0)
    blk = np.ascontiguousarray(app[:, :5000])            # more than the ring holds: only the last 3000 survive
    ds.record_app_push(blk, 1)
    orc.push_app(blk, 1)
    assert orc.app_evictions == 2000 and ds.record_buffered() == orc.buffered() == (cap, cap)
    got, want = ds.record_drain(1), orc.drain(1)         # the heads move: the next appends wrap
    _check_rows(got, want, "first frame")
    orc.push_mic(ds.push(np.ascontiguousarray(x[:, 4 * PUSH:])))       # 960 into 1848: 2808
    blk = np.ascontiguousarray(app[:, 5000:])            # 700 into 1848
    ds.record_app_push(blk, 1)
    orc.push_app(blk, 1)
    assert ds.record_buffered() == orc.buffered() == (cap - FRAME + 960, cap - FRAME + 700)
    orc.push_mic(ds.push(_data(B, PUSH, seed=4)))        # 960 more: evicts from a partly consumed ring, the tail has wrapped
    assert orc.mic_evictions == 360 + 768 and ds.record_buffered() == orc.buffered()
    assert ds.record_frames_ready() == orc.frames_ready() == 2
    got, want = ds.record_drain(), orc.drain()
    print(f"[rn record] eviction: mic {orc.mic_evictions}, app {orc.app_evictions} evicted, left {orc.buffered()}")
    _check_rows(got, want, "rest")
    assert want.shape[1] == 2 * 2 * FRAME and ds.record_buffered() == orc.buffered()
    ds.close()


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_the_reference_ring_of_ten_seconds():
    B, sec = 2, 48000
    x = _data(B, 10 * sec + sec // 2, seed=5)
    app = _data(B, 10 * sec + sec // 2, seed=6)
    ds = _mk(B, 48000.0, 0)
    orc = RO.RecordOracle(B)
    for p in range(0, x.shape[1], sec):
        orc.push_mic(ds.push(np.ascontiguousarray(x[:, p:p + sec])))
        blk = np.ascontiguousarray(app[:, p:p + sec])
        ds.record_app_push(blk, 1)
        orc.push_app(blk, 1)
        assert ds.record_buffered() == orc.buffered()
    assert orc.mic_evictions == sec // 2 - 480 and orc.app_evictions == sec // 2
    assert ds.record_buffered() == (10 * sec, 10 * sec) and ds.record_frames_ready() == orc.frames_ready() == 416
    got, want = ds.record_drain(), orc.drain()
    _check_rows(got, want, "ten seconds")
    assert want.shape == (B, 416 * 2 * FRAME) and ds.record_buffered() == orc.buffered() == (768, 768)
    ds.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_formats_strides_and_splitting():
    """Four handles fed the same: s16 and f32, each once as one drain into 16-byte aligned rows and once cut into 1 frame +
    the rest into rows one element past alignment with an odd stride (the fallback stores).  Buffers hold a sentinel first."""
    import torch
    B = 3
    x = _data(B, 4 * PUSH, seed=7)
    app = _data(B, 2 * FRAME + 100, seed=8)
    d_app = torch.from_numpy(app).cuda()
    torch.cuda.synchronize()
    orc = RO.RecordOracle(B, 6000)
    hs = [_mk(B, 48000.0, 6000) for _ in range(4)]
    outs = [h.push(x) for h in hs]                        # 8 frames completed, 7 returned: 3360 samples
    for o in outs[1:]:
        assert _same(o, outs[0])
    orc.push_mic(outs[0])
    orc.push_app(app, 1)
    for h in hs:
        h.record_app_push_device(d_app.data_ptr(), app.shape[1], app.shape[1], 1)
        h.synchronize()
        assert h.record_buffered() == orc.buffered() == (3360, 2 * FRAME + 100)
    want = orc.drain()
    n = want.shape[1] // (2 * FRAME)
    assert n == 2 and orc.mixed_frames == 2
    res = {}
    for h, (fmt, aligned) in zip(hs, (("i16", True), ("i16", False), ("f32", True), ("f32", False))):
        tdt, ndt, sentinel, eps = (torch.int16, np.int16, 0x5A5A, 2) if fmt == "i16" else (torch.float32, np.float32, 12345.0, 1)
        ne = n * FRAME * eps
        per16 = 16 // np.dtype(ndt).itemsize
        stride, shift = (ne + per16, 0) if aligned else ((ne + 3) | 1, 1)
        buf = torch.full((B * stride + 8,), sentinel, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        ptr = buf.data_ptr() + shift * buf.element_size()
        assert (ptr % 16 == 0 and stride * buf.element_size() % 16 == 0) == aligned
        if aligned:
            assert h.record_drain_device(1 << 40, ptr, stride, fmt=fmt) == n
        else:
            assert h.record_drain_device(1, ptr, stride, fmt=fmt) == 1
            assert h.record_drain_device(99, ptr + FRAME * eps * buf.element_size(), stride, fmt=fmt) == n - 1
        h.synchronize()
        assert h.record_buffered() == orc.buffered()
        flat = buf.cpu().numpy()
        rows = flat[shift:shift + B * stride].reshape(B, stride)
        assert (rows[:, ne:] == sentinel).all() and (flat[:shift] == sentinel).all() and (flat[shift + B * stride:] == sentinel).all(), (fmt, aligned)
        res[(fmt, aligned)] = rows[:, :ne].copy()
        h.close()
    _check_rows(res[("i16", True)], want, "s16, aligned")
    _check_rows(res[("i16", False)], want, "s16, odd stride, 1 + rest")
    fr = want.reshape(B, -1, 2)
    assert (fr[:, :, 0] == fr[:, :, 1]).all()                                   # L == R
    f32 = RO.as_transcriber(fr[:, :, 0])                                        # channel 0, / 32768
    _check_rows(res[("f32", True)], f32, "f32, aligned")
    _check_rows(res[("f32", False)], f32, "f32, odd stride, 1 + rest")
    assert (want[-1] == 32767).any() and (want[-1] == -32767).any()             # the clamped stream


# ---- 5 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 3, 8])
def test_downmix_and_clamp(channels):
    """Stream 0: small samples; stream 1: mic at 0.8 in, app 0.8 on every channel; stream 2: mic at amplitude 1.5 (+-1 after the
    push's clamp).  One inf, one -inf and one NaN in the app data, and from two channels on a frame of (inf, -inf)."""
    B, n_app = 3, 2 * FRAME + 77
    x = _data(B, 4 * PUSH, seed=9)
    x[1] = np.where(x[1] >= 0, np.float32(0.8), np.float32(-0.8))
    app = np.random.default_rng(10 + channels).uniform(-0.5, 0.5, size=(B, n_app, channels)).astype(np.float32)
    app[1] = np.float32(0.8)
    app[0, 5, 0] = np.inf
    app[0, 9, channels - 1] = -np.inf
    app[2, 11, 0] = np.nan
    if channels >= 2:
        app[0, 20, 0], app[0, 20, 1] = np.inf, -np.inf
    app[2, 30, :] = np.float32(-0.0)
    app = np.ascontiguousarray(app.reshape(B, n_app * channels))
    ds = _mk(B, 48000.0, 5000)
    orc = RO.RecordOracle(B, 5000)
    out = ds.push(x)
    orc.push_mic(out)
    ds.record_app_push(app, channels)
    orc.push_app(app, channels)
    assert ds.record_buffered() == orc.buffered() == (3360, n_app)
    got, want = ds.record_drain(), orc.drain()
    _check_rows(got, want, f"{channels} channels")
    assert want.shape[1] == 2 * 2 * FRAME and orc.mixed_frames == 2
    q = want[:, 0::2]
    mono = RO.downmix(app, channels)
    assert np.isposinf(mono[0, 5]) and np.isneginf(mono[0, 9]) and np.isnan(mono[2, 11])
    assert q[0, 5] == 32767 and q[0, 9] == -32767 and q[2, 11] == 0
    if channels >= 2:
        assert np.isnan(mono[0, 20]) and q[0, 20] == 0                          # inf + (-inf)
    loud = np.abs(out[1, :2 * FRAME] + mono[1, :2 * FRAME]) > 1
    print(f"[rn record] {channels} channels: {int(loud.sum())} mixed samples of stream 1 beyond +-1, "
          f"{int((np.abs(q[2]) == 32767).sum())} full-scale samples on stream 2")
    assert loud.any() and (np.abs(q[1][loud]) == 32767).all() and (np.abs(q[2]) == 32767).any()
    ds.close()


# ---- 6 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64, 65, 130])
def test_level_equals_the_sequential_loop(B):
    import torch
    ds = _mk(B)
    for n in (1, 63, 64, 65, 1000, 4097):
        stride = n + 3
        x = np.random.default_rng(100 * B + n).uniform(-1, 1, size=(B, stride)).astype(np.float32)
        x[-1] *= np.float32(1e-3)                      # a quiet stream: small squares added to a small sum
        want = RO.level(x[:, :n])
        d_x = torch.from_numpy(x).cuda()
        d_rms = torch.full((B + 2,), -7.0, device="cuda")
        torch.cuda.synchronize()
        ds.level_device(d_x.data_ptr(), stride, 0, d_rms.data_ptr())           # n_in == 0: a no-op
        ds.level_device(d_x.data_ptr(), stride, n, d_rms.data_ptr() + 4)
        ds.synchronize()
        got = d_rms.cpu().numpy()
        assert got[0] == -7.0 and got[-1] == -7.0, (B, n)
        assert _same(got[1:-1], want), (B, n, np.nonzero(got[1:-1] != want)[0][:8])
        if n in (65, 4097):
            assert _same(ds.level(np.ascontiguousarray(x[:, :n])), want), (B, n, "host")
    assert want.all() and want[-1] < 1e-3
    ds.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_lifecycle():
    import torch
    B = 3
    x = _data(B, 6 * PUSH, seed=11)
    app = _data(B, 3000, seed=12)
    # the order of the two configures does not matter, and a handle that does not record pushes and pulls the same bytes
    plain = _mk(B, 44100.0, None, 22050.0)
    rec_first = _mk(B, 44100.0, 4000, 22050.0)
    rec_last = _mk(B, 44100.0, None, 22050.0)
    rec_last.record_configure(4000)
    orc = RO.RecordOracle(B, 4000)
    L = plain._L
    for r in range(3):
        blk = np.ascontiguousarray(x[:, r * PUSH:(r + 1) * PUSH])
        outs = [h.push(blk, want_vad=True) for h in (plain, rec_first, rec_last)]
        pulls = [h.pull(300, channels=2, fmt="i16") for h in (plain, rec_first, rec_last)]
        for o, p in zip(outs[1:], pulls[1:]):
            assert _same(o[0], outs[0][0]) and _same(o[1], outs[0][1]) and _same(p, pulls[0])
        orc.push_mic(outs[0][0])
        a = np.ascontiguousarray(app[:, r * 1000:(r + 1) * 1000])
        orc.push_app(a, 1)
        for h in (rec_first, rec_last):
            h.record_app_push(a, 1)
            assert h.record_buffered() == orc.buffered()
    assert plain.record_buffered() == (0, 0) and plain.record_frames_ready() == 0
    n, buf = C.c_long(5), np.zeros((B, 4 * FRAME), np.int16)
    assert L.crispy_rn_record_drain(plain._h, 1, 1, buf.ctypes.data, buf.shape[1], C.byref(n)) == -1
    assert "crispy_rn_record_drain:" in L.crispy_last_error().decode() and "not configured" in L.crispy_last_error().decode()
    assert L.crispy_rn_record_app_push(plain._h, app.ctypes.data, app.shape[1], 10, 1) == -1
    assert "crispy_rn_record_app_push:" in L.crispy_last_error().decode() and "not configured" in L.crispy_last_error().decode()
    # invalid calls leave the state as it was
    h = rec_first
    d = torch.zeros((B, 4 * FRAME), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    before = h.record_buffered()
    assert before[0] >= FRAME and h.record_frames_ready() >= 1
    bad = [("max_frames < 0", (h._h, -1, 1, d.data_ptr(), 4 * FRAME, C.byref(n))),
           ("format", (h._h, 1, 2, d.data_ptr(), 4 * FRAME, C.byref(n))),
           ("format", (h._h, 1, -1, d.data_ptr(), 4 * FRAME, C.byref(n))),
           ("NULL", (h._h, 1, 1, None, 4 * FRAME, C.byref(n))),
           ("NULL", (h._h, 1, 1, d.data_ptr(), 4 * FRAME, None)),
           ("out_stride", (h._h, 1, 1, d.data_ptr(), 2 * FRAME - 1, C.byref(n))),
           ("out_stride", (h._h, 1, 0, d.data_ptr(), FRAME - 1, C.byref(n)))]
    for what, args in bad:
        assert L.crispy_rn_record_drain_device(*args, None) == -1, what
        msg = L.crispy_last_error().decode()
        assert msg.startswith("crispy_rn_record_drain_device:") and what in msg, (what, msg)
        hargs = args[:3] + (buf.ctypes.data if args[3] else None,) + args[4:]
        assert L.crispy_rn_record_drain(*hargs) == -1, what
        assert L.crispy_last_error().decode().startswith("crispy_rn_record_drain:"), what
    for what, args in (("n_frames < 0", (h._h, d.data_ptr(), 64, -1, 1)), ("channels", (h._h, d.data_ptr(), 64, 8, 0)),
                       ("channels", (h._h, d.data_ptr(), 64, 4, 9)), ("in_stride", (h._h, d.data_ptr(), 15, 8, 2)),
                       ("NULL", (h._h, None, 64, 8, 1))):
        assert L.crispy_rn_record_app_push_device(*args, None) == -1, what
        assert what in L.crispy_last_error().decode(), what
    assert L.crispy_rn_record_configure(h._h, 2 * FRAME - 1) == -1 and L.crispy_rn_record_configure(h._h, -1) == -1
    assert L.crispy_rn_level_device(h._h, d.data_ptr(), 3, 4, d.data_ptr(), None) == -1
    assert L.crispy_rn_level_device(h._h, d.data_ptr(), 1 << 25, (1 << 24) + 1, d.data_ptr(), None) == -1
    assert n.value == 5 and not buf.any() and h.record_buffered() == before == rec_last.record_buffered()
    assert L.crispy_rn_record_drain_device(h._h, 0, 1, d.data_ptr(), 0, C.byref(n), None) == 0 and n.value == 0       # max_frames == 0
    assert h.record_buffered() == before
    # a model switch and a state reset leave the recording rings alone
    for hh in (rec_first, rec_last):
        hh.reset()
        hh.adapter_configure(44100.0, 1.0)
        assert hh.record_buffered() == before and hh.playback_buffered() == 0
    want = orc.drain()
    assert want.shape[1] >= 2 * FRAME
    _check_rows(rec_first.record_drain(), want, "configure first")
    _check_rows(rec_last.record_drain(), want, "configure last")
    assert rec_first.record_buffered() == rec_last.record_buffered() == orc.buffered()
    # start_recording empties both rings (and may resize them); pushes go on
    assert orc.buffered()[0] > 0
    rec_first.record_configure(4000)
    rec_last.record_configure(2 * FRAME)
    for hh in (rec_first, rec_last):
        assert hh.record_buffered() == (0, 0) and hh.record_frames_ready() == 0
    out = rec_last.push(np.ascontiguousarray(x[:, 3 * PUSH:]))
    fresh = RO.RecordOracle(B, 2 * FRAME)
    fresh.push_mic(out)
    assert rec_last.record_buffered() == fresh.buffered() and fresh.mic_evictions > 0
    _check_rows(rec_last.record_drain(), fresh.drain(), "after start_recording")
    for hh in (plain, rec_first, rec_last):
        hh.close()

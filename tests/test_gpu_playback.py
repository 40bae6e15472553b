"""GPU tests of the playback half of the capture-rate adapter, crispy_rn_playback_* / crispy_rn_pull* (include/crispy_hip.h):
RnnNoiseProcessor's `output_buf` and `next_sample` (src-tauri/src/audio.rs:280-285, 297-314) and the output callback's
conversions (audio.rs:610-657) for every stream of a handle at once.

Everything is compared on the bytes against tests/playback_oracle.py, which is fed the arrays the pushes returned."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests.playback_oracle import PlaybackOracle, convert

pytestmark = pytest.mark.gpu

FRAME = 480
RATES = (44100.0, 48000.0, 96000.0, 16000.0, 22050.0)
PUSH = 1000            # capture samples per round
ROUNDS = 12
LONG = (4, 8)          # rounds whose pull is 1.9 x the push's worth, the others 0.8 x


def _mk(B, capture_rate=None, output_rate=None):
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState
    ds = DenoiseState(synthetic_weights(0), B, 0)
    if capture_rate is not None:
        ds.adapter_configure(capture_rate, 1.0)
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


def _pull_frames(out_rate, r):
    return int(PUSH * out_rate / 48000.0 * (1.9 if r in LONG else 0.8))


@functools.lru_cache(maxsize=None)
def _run(B, capture_rate, out_rate, rounds=ROUNDS, split=False):
    """37 frames pulled before any push, then `rounds` rounds of (push 1000 samples, pull).  split: every pull cut in three
    (1, n / 2, rest).  Returns one record per pull, with what the oracle gives beside it; shared and never changed."""
    x = _data(B, rounds * PUSH)
    ds = _mk(B, capture_rate, out_rate)
    orc = PlaybackOracle(B, capture_rate, out_rate)
    log = []

    def pull(r, n):
        parts = [1, n // 2, n - 1 - n // 2] if split else [n]
        got, live = [], 0
        for m in parts:
            g, l = ds.pull(m, want_live=True)
            got.append(g)
            live += l
        want, want_live = orc.pull(n)
        log.append(dict(round=r, n=n, got=np.concatenate(got, axis=1), live=live, want=want, want_live=want_live,
                        buffered=ds.playback_buffered(), want_buffered=len(orc)))

    pull(0, 37)
    for r in range(1, rounds + 1):
        out = ds.push(np.ascontiguousarray(x[:, (r - 1) * PUSH:r * PUSH]))
        orc.push(out)
        assert ds.playback_buffered() == len(orc), (r, ds.playback_buffered(), len(orc))
        pull(r, _pull_frames(out_rate, r))
    ds.close()
    return tuple(log), (orc.evictions, orc.pops, orc.zeros)


def _check_log(log, what):
    for p in log:
        print(f"[rn pull] {what} round {p['round']}: {p['n']} frames, {p['live']} live (oracle {p['want_live']}), buffered {p['buffered']} ({p['want_buffered']})")
    for p in log:
        assert p["live"] == p["want_live"] and p["buffered"] == p["want_buffered"], (what, p["round"])
        for b in range(p["want"].shape[0]):
            assert _same(p["got"][b], p["want"][b]), (what, "round", p["round"], "stream", b, np.nonzero(p["got"][b] != p["want"][b])[0][:8])


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_rate", RATES)
def test_interleaved_schedule_equals_the_oracle(out_rate):
    """The 37 'pulls' before the first push are 37 calls of next_sample: one pull of 37 frames."""
    log, _ = _run(3, 48000.0, out_rate)
    _check_log(log, f"48000 -> {out_rate}")
    # what the schedule is for, on the oracle's own counts, so that a changed schedule cannot silently lose it
    by = {p["round"]: p for p in log}
    assert by[0]["want_live"] == 0 and not by[0]["want"].any()                 # nothing but zeros before the first push
    assert 0 < by[1]["want_live"] < by[1]["n"]                                 # the first round runs dry part way
    for r in (2, 3, 5, 6, 7, 9, 10, 11, 12):
        assert by[r]["want_live"] == by[r]["n"], r                             # fully live pulls, also after a dry one
    for r in LONG:
        assert 0 < by[r]["want_live"] < by[r]["n"] and by[r]["want_buffered"] == 1, r     # a pull that runs dry
    if out_rate == 44100.0:
        assert (by[1]["n"], by[1]["n"] - by[1]["want_live"]) == (735, 294)
        assert (by[8]["n"], by[8]["n"] - by[8]["want_live"]) == (1745, 422)


def test_interleaved_schedule_with_the_input_resampler():
    """Capture rate 44100: the input resampler is in, the ring holds 48000 samples and the step is 48000 / 44100."""
    log, _ = _run(3, 44100.0, 44100.0)
    _check_log(log, "44100 -> 44100")
    by = {p["round"]: p for p in log}
    assert by[0]["want_live"] == 0
    assert (by[1]["n"], by[1]["n"] - by[1]["want_live"]) == (735, 294)         # 480 samples returned by the first push
    assert 0 < by[4]["want_live"] < by[4]["n"]
    assert by[12]["want_live"] == by[12]["n"]


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capture_rate,figures", [
    (48000.0, (480, 48000, 47703, 1623, 101, 1)),
    (48000.5, (480, 48000, 47703, 1623, 101, 1)),       # no resampler, cap stays 48000
    (47999.5, (481, 47999, 47703, 1625, 101, 1)),       # cap 47999; the step is a hair under 3: 296 pops in the first pull
])
def test_eviction_and_wrap(capture_rate, figures):
    B, out_rate = 2, 16000.0
    n1 = 101 * FRAME + FRAME + 7
    x = _data(B, n1 + 3 * FRAME, seed=2)
    ds = _mk(B, capture_rate, out_rate)
    orc = PlaybackOracle(B, capture_rate, out_rate)
    out = ds.push(np.ascontiguousarray(x[:, :n1]))
    assert out.shape == (B, 101 * FRAME)                     # more than the ring holds
    orc.push(out)
    seen = [orc.evictions, len(orc)]
    assert ds.playback_buffered() == len(orc)
    got, live = ds.pull(100, want_live=True)
    want, want_live = orc.pull(100)
    assert _same(got, want) and live == want_live == 100
    seen.append(len(orc))
    assert ds.playback_buffered() == len(orc)
    out = ds.push(np.ascontiguousarray(x[:, n1:]))
    assert out.shape == (B, 3 * FRAME)
    orc.push(out)                                            # evicts from a partly consumed ring; the tail wraps
    seen.append(orc.evictions)
    assert ds.playback_buffered() == len(orc) == orc.max_output_len
    got, live = ds.pull(16100, want_live=True)
    want, want_live = orc.pull(16100)
    seen += [16100 - want_live, len(orc)]
    print(f"[rn pull] eviction, capture {capture_rate}: {seen}")
    assert tuple(seen) == figures
    assert live == want_live and ds.playback_buffered() == len(orc)
    for b in range(B):
        assert _same(got[b], want[b]), (b, np.nonzero(got[b] != want[b])[0][:8])
    ds.close()


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_splitting_does_not_matter():
    whole, _ = _run(3, 48000.0, 44100.0)
    split, _ = _run(3, 48000.0, 44100.0, split=True)
    assert len(whole) == len(split) == ROUNDS + 1
    a = np.concatenate([p["got"] for p in whole], axis=1)
    b = np.concatenate([p["got"] for p in split], axis=1)
    assert _same(a, b)
    assert [p["live"] for p in whole] == [p["live"] for p in split]
    assert whole[-1]["buffered"] == split[-1]["buffered"] == whole[-1]["want_buffered"]


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_formats_and_channels():
    """f32 x 1, i16 x 2 and u16 x 3 on three handles with the same pushes, 48000 -> 96000 (every other frame is a ring
    sample itself, so the clamped stream's +-1 arrive unchanged).  The first pull (1201 frames, partly dry) goes to 16-byte
    aligned rows whose last 16 bytes are partial, the second (1001 frames) to rows one element past alignment with an odd
    stride: the fallback store path.  Buffers are filled with a sentinel first."""
    import torch
    B, out_rate = 3, 96000.0
    x = _data(B, 2 * PUSH, seed=4)
    specs = (("f32", 1, torch.float32, np.float32, 12345.0), ("i16", 2, torch.int16, np.int16, 0x5A5A), ("u16", 3, torch.int16, np.uint16, 0x5A5A))
    hs = [_mk(B, 48000.0, out_rate) for _ in specs]
    orc = PlaybackOracle(B, 48000.0, out_rate)
    pulls = {s[0]: [] for s in specs}
    wants = []
    for k, n in enumerate((1201, 1001)):
        outs = [h.push(np.ascontiguousarray(x[:, k * PUSH:(k + 1) * PUSH])) for h in hs]
        assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])
        orc.push(outs[0])
        want, want_live = orc.pull(n)
        wants.append(want)
        for h, (fmt, ch, tdt, ndt, sentinel) in zip(hs, specs):
            ne = n * ch
            per16 = 16 // np.dtype(ndt).itemsize
            if k == 0:
                stride, shift = (ne + per16 - 1) // per16 * per16 + per16, 0
            else:
                stride, shift = (ne + 3) | 1, 1
            buf = torch.full((B * stride + 8,), sentinel, dtype=tdt, device="cuda")
            torch.cuda.synchronize()
            ptr = buf.data_ptr() + shift * buf.element_size()
            assert (ptr % 16 == 0 and stride * buf.element_size() % 16 == 0) == (k == 0)
            live = h.pull_device(n, ptr, stride, channels=ch, fmt=fmt)
            h.synchronize()
            assert live == want_live
            flat = buf.cpu().numpy().view(ndt)
            rows = flat[shift:shift + B * stride].reshape(B, stride)
            sv = np.array([sentinel]).astype(np.int16 if ndt != np.float32 else np.float32).view(ndt)[0]
            assert (rows[:, ne:] == sv).all() and (flat[:shift] == sv).all() and (flat[shift + B * stride:] == sv).all(), (fmt, k)
            pulls[fmt].append(rows[:, :ne].copy())
    assert not wants[0][:, -1].any() and wants[0][:, :100].any()                 # the first pull is partly dry
    for k, want in enumerate(wants):
        f32 = pulls["f32"][k]
        assert _same(f32, want), k
        for fmt, ch in (("i16", 2), ("u16", 3)):
            got = pulls[fmt][k]
            assert _same(got, convert(f32, fmt, ch)), (fmt, k, np.nonzero(got != convert(f32, fmt, ch)))
            fr = got.reshape(B, -1, ch)
            assert (fr == fr[:, :, :1]).all()                                    # every channel of a frame the same value
    assert (pulls["u16"][0][:, -3:] == 32767).all() and (pulls["i16"][0][:, -2:] == 0).all()     # silence
    i16 = np.concatenate(pulls["i16"], axis=1)[-1]
    u16 = np.concatenate(pulls["u16"], axis=1)[-1]
    print(f"[rn pull] clamped stream: i16 {int((i16 == 32767).sum())} x +32767, {int((i16 == -32767).sum())} x -32767; "
          f"u16 {int((u16 == 65535).sum())} x 65535, {int((u16 == 0).sum())} x 0")
    assert (i16 == 32767).any() and (i16 == -32767).any() and (u16 == 65535).any() and (u16 == 0).any()
    for h in hs:
        h.close()


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_width_seventy_streams():
    """B is not a multiple of the wave; every stream has its own data and is checked on its own."""
    log, _ = _run(70, 48000.0, 44100.0, rounds=1)
    assert len(log) == 2 and 0 < log[1]["want_live"] < log[1]["n"]
    _check_log(log, "B = 70")


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_host_entry_points_equal_the_device_ones():
    import torch
    B, rounds, out_rate = 3, 5, 44100.0
    x = _data(B, rounds * PUSH, seed=6)
    host, dev = _mk(B, 44100.0, out_rate), _mk(B, 44100.0, out_rate)
    d_x = torch.from_numpy(x).cuda()
    n_live = 0
    for r in range(1, rounds + 1):
        a = host.push(np.ascontiguousarray(x[:, (r - 1) * PUSH:r * PUSH]))
        d_out = torch.zeros((B, 3 * FRAME), device="cuda")
        torch.cuda.synchronize()
        n_out = dev.push_device(d_x.data_ptr() + 4 * (r - 1) * PUSH, rounds * PUSH, PUSH, d_out.data_ptr(), 3 * FRAME)
        assert n_out == a.shape[1] and host.playback_buffered() == dev.playback_buffered()
        n = _pull_frames(out_rate, r)
        got, live = host.pull(n, channels=2, fmt="i16", want_live=True)
        d_pcm = torch.full((B, 2 * n + 6), 77, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        live_d = dev.pull_device(n, d_pcm.data_ptr(), 2 * n + 6, channels=2, fmt="i16")
        dev.synchronize()
        pcm = d_pcm.cpu().numpy()
        assert _same(d_out.cpu().numpy()[:, :n_out], a)
        assert live == live_d and _same(pcm[:, :2 * n], got) and (pcm[:, 2 * n:] == 77).all(), r
        assert host.playback_buffered() == dev.playback_buffered()
        n_live += live
    assert n_live > 0 and got.any()
    host.close()
    dev.close()


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_a_push_is_unchanged_by_playback():
    import torch
    B, n = 3, 2 * PUSH
    x = _data(B, n, seed=7)
    d_x = torch.from_numpy(x).cuda()
    res = []
    for out_rate in (None, 22050.0):
        h = _mk(B, 44100.0, out_rate)
        got = []
        for pos, nb in ((0, 7), (7, 1200), (1207, n - 1207)):
            d_out = torch.full((B, 4 * FRAME), float("nan"), device="cuda")
            d_fr = torch.full((B, 4 * FRAME), float("nan"), device="cuda")
            d_vad = torch.full((4, B), float("nan"), device="cuda")
            torch.cuda.synchronize()
            n_out = h.push_device(d_x.data_ptr() + 4 * pos, n, nb, d_out.data_ptr(), 4 * FRAME, d_fr.data_ptr(), 4 * FRAME, d_vad.data_ptr())
            h.synchronize()
            got.append((n_out, d_out.cpu().numpy(), d_fr.cpu().numpy(), d_vad.cpu().numpy()))
        res.append((got, h.playback_buffered()))
        h.close()
    (plain, nb0), (play, nb1) = res
    assert nb0 == 0 and nb1 == sum(g[0] for g in play) > 0
    for a, b in zip(plain, play):
        assert a[0] == b[0]
        for u, v in zip(a[1:], b[1:]):
            assert _same(u, v)


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_configure_empties_the_ring():
    B = 2
    x = _data(B, 3 * PUSH, seed=8)
    # adapter_configure: the new processor
    h = _mk(B, 48000.0, 44100.0)
    h.push(np.ascontiguousarray(x[:, :2 * PUSH]))
    got, live = h.pull(100, want_live=True)
    assert live == 100 and h.playback_buffered() > 0             # resample_pos is now 0.84...
    h.adapter_configure(48000.0, 1.0)
    assert h.playback_buffered() == 0
    got, live = h.pull(10, want_live=True)
    assert live == 0 and not got.any()
    out = h.push(np.ascontiguousarray(x[:, 2 * PUSH:]))
    assert out.shape == (B, FRAME)                               # the first frame is dropped again
    orc = PlaybackOracle(B, 48000.0, 44100.0)                    # the output rate stayed
    orc.push(out)
    got = h.pull(50)
    assert _same(got, orc.pull(50)[0]) and _same(got[:, 0], out[:, 0])       # pos started at 0: the first output is buf[0]
    h.close()
    # playback_configure: the same, and the capture side keeps what it carried
    h = _mk(B, 44100.0, 44100.0)
    h.push(np.ascontiguousarray(x[:, :700]))                      # 761 samples at 48 kHz: a frame and 281 carried
    out = h.push(np.ascontiguousarray(x[:, 700:1400]))
    assert out.shape[1] > 0 and h.playback_buffered() == out.shape[1]
    h.pull(33)
    want_n = h.push_out_len(500)
    h.playback_configure(22050.0)
    assert h.playback_buffered() == 0 and h.push_out_len(500) == want_n
    got, live = h.pull(10, want_live=True)
    assert live == 0 and not got.any()
    out = h.push(np.ascontiguousarray(x[:, 1400:1900]))
    assert out.shape == (B, want_n) and want_n > 0
    orc = PlaybackOracle(B, 44100.0, 22050.0)
    orc.push(out)
    got = h.pull(60)
    assert _same(got, orc.pull(60)[0]) and _same(got[:, 0], out[:, 0])
    assert h.playback_buffered() == len(orc)
    h.close()


# ---- 9 -------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_handle_untouched():
    import torch
    B = 2
    x = _data(B, 2 * PUSH, seed=9)
    h = _mk(B, 48000.0, 44100.0)
    L = h._L
    orc = PlaybackOracle(B, 48000.0, 44100.0)
    orc.push(h.push(x))
    d = torch.zeros((B, 64), device="cuda")
    torch.cuda.synchronize()
    live = C.c_long(-5)
    bad = [
        ("n_frames < 0", (h._h, -1, 1, 0, d.data_ptr(), 64)),
        ("above the limit", (h._h, (1 << 24) + 1, 1, 0, d.data_ptr(), 1 << 25)),
        ("channels", (h._h, 8, 0, 0, d.data_ptr(), 64)),
        ("channels", (h._h, 8, 9, 0, d.data_ptr(), 128)),
        ("format", (h._h, 8, 1, 3, d.data_ptr(), 64)),
        ("format", (h._h, 8, 1, -1, d.data_ptr(), 64)),
        ("out_stride", (h._h, 8, 2, 0, d.data_ptr(), 15)),
        ("NULL", (h._h, 8, 1, 0, None, 64)),
        ("NULL handle", (None, 8, 1, 0, d.data_ptr(), 64)),
    ]
    plain = _mk(B)                                              # never configured for playback
    assert plain.playback_buffered() == 0
    bad.append(("not configured", (plain._h, 8, 1, 0, d.data_ptr(), 64)))
    oh = np.zeros((B, 64), np.float32)
    for k, (what, args) in enumerate(bad):
        assert L.crispy_rn_pull_device(*args, C.byref(live), None) == -1, what
        msg = L.crispy_last_error().decode()
        assert "crispy_rn_pull_device" in msg and what in msg, (what, msg)
        hargs = args[:4] + (oh.ctypes.data if args[4] else None,) + args[5:]
        assert L.crispy_rn_pull(*hargs, C.byref(live)) == -1, what
        msg = L.crispy_last_error().decode()
        assert "crispy_rn_pull:" in msg and what in msg, (what, msg)
        if k % 3 == 0:                                          # a valid pull in between: as if the bad calls had not happened
            got, n_live = h.pull(37, want_live=True)
            want, want_live = orc.pull(37)
            assert _same(got, want) and n_live == want_live == 37 and h.playback_buffered() == len(orc), what
    assert L.crispy_rn_playback_configure(h._h, 0.0) == -1 and L.crispy_rn_playback_configure(h._h, float("inf")) == -1
    assert L.crispy_rn_pull_device(h._h, 0, 1, 0, None, 0, C.byref(live), None) == 0 and live.value == 0      # n_frames == 0: a no-op
    assert h.playback_buffered() == len(orc)
    d.fill_(float("nan"))
    torch.cuda.synchronize()
    assert h.pull_device(40, d.data_ptr(), 64) == 40
    h.synchronize()
    want, _ = orc.pull(40)
    got = d.cpu().numpy()
    assert _same(got[:, :40], want) and np.isnan(got[:, 40:]).all()
    assert h.playback_buffered() == len(orc)
    h.close()
    plain.close()


# ---- 10 ------------------------------------------------------------------------------------------------------------
def test_pull_block_equals_next_sample():
    """B = 2, 44.1 kHz -> 44.1 kHz, six frames' worth of capture samples in blocks of 441 (480 samples at 48 kHz: one frame
    per block); after every block 400 output frames are read."""
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import RnnNoiseProcessor
    B, rate, block, n_pull = 2, 44100.0, 441, 400
    n = 6 * block
    x = _data(B, n, seed=10)
    single = RnnNoiseProcessor(synthetic_weights(0), rate, rate, 1.0, n_streams=B)
    blocks = RnnNoiseProcessor(synthetic_weights(0), rate, rate, 1.0, n_streams=B)
    want, got = [], []
    for p in range(0, n, block):
        for i in range(p, p + block):
            single.push_sample(x[:, i])
        want.append(np.stack([single.next_sample() for _ in range(n_pull)], axis=1))
        blocks.push_block(np.ascontiguousarray(x[:, p:p + block]))
        got.append(blocks.pull_block(n_pull))
        assert blocks.denoise.playback_buffered() == len(single.output_buf)
    want, got = np.concatenate(want, axis=1), np.concatenate(got, axis=1)
    assert want.shape == got.shape == (B, 6 * n_pull) and want.any()
    assert not want[:, :n_pull].any() and want[:, -n_pull:].any()         # nothing buffered after the first block; live at the end
    assert _same(got, want.astype(np.float32))

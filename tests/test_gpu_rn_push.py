"""GPU tests of the capture-rate adapter, crispy_rn_push* (include/crispy_hip.h): RnnNoiseProcessor::push_sample
(src-tauri/src/audio.rs:242-295) for a block of raw capture samples of every stream at once.

Everything is compared bit for bit (np.array_equal on the bytes): the frames that enter process_frame against the Python
mirror of the reference's LinearResampler (crispy_amd.denoise.LinearResampler, audio.rs:73-134) run per stream, x32768, cut
into 480-sample frames; the samples that come out against crispy_rn_process on a second handle fed those frames, followed by
the reference's / 32768, clamp, volume and first-frame drop in numpy f32."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FRAME = 480
BLOCKS = (1, 7, 441, 480, 1000, 4410)       # then the rest
VOL0, VOL1, VOL_AT = 0.8, 0.3, 4            # volume 0.8, set to 0.3 in front of push number 4


def _mk(B):
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState
    return DenoiseState(synthetic_weights(0), B, 0)


def _data(B, n, seed=0):
    """Every stream its own random samples in +-0.5; the last stream at amplitude 1.5, so that the clamp has work."""
    x = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(B, n)).astype(np.float32)
    x[-1] *= np.float32(3.0)
    return x


def _split(n, blocks=BLOCKS):
    out, left = [], n
    for b in blocks:
        if left > b:
            out.append(b)
            left -= b
    return out + [left]


@functools.lru_cache(maxsize=None)
def _reference48(B, rate, n, seed=0):
    """(ref [B, n48] f32: the 48 kHz samples of every stream, acc [n + 1]: how many there are after k inputs)."""
    from crispy_amd.denoise import LinearResampler
    x = _data(B, n, seed)
    rows, acc = [], None
    for b in range(B):
        rs, out, counts = LinearResampler(rate, 48000.0), [], [0]
        for s in x[b]:
            rs.process_sample(s, out.append)
            counts.append(len(out))
        rows.append(np.array(out, dtype=np.float32))
        assert acc is None or acc == counts      # lock-stepped streams: the positions do not depend on the samples
        acc = counts
    ref = np.stack(rows)
    ref.setflags(write=False)
    return ref, tuple(acc)


@functools.lru_cache(maxsize=None)
def _pushed(B, rate, n, blocks=BLOCKS, seed=0):
    """The n samples of _data pushed through crispy_rn_push_device in `blocks`.  Per push: n_out, crispy_rn_push_out_len
    asked just before, and what arrived in d_out / d_frames48 / d_vad (buffers pre-filled with NaN, so the extent written is
    visible).  Shared by the tests below and never changed."""
    import torch
    x = _data(B, n, seed)
    ds = _mk(B)
    ds.adapter_configure(rate, VOL0)
    d_x = torch.from_numpy(x).cuda()
    pushes, pos = [], 0
    for k, nb in enumerate(_split(n, blocks)):
        if k == VOL_AT:
            ds.adapter_set_volume(VOL1)
        cap = (FRAME + int(nb * 48000.0 / rate) + 8) // FRAME * FRAME           # more than any push of nb samples completes
        d_in = d_x[:, pos:pos + nb].contiguous()
        d_out = torch.full((B, cap), float("nan"), device="cuda")
        d_frames = torch.full((B, cap), float("nan"), device="cuda")
        d_vad = torch.full((cap // FRAME, B), float("nan"), device="cuda")
        torch.cuda.synchronize()
        want = ds.push_out_len(nb)
        n_out = ds.push_device(d_in.data_ptr(), nb, nb, d_out.data_ptr(), cap, d_frames.data_ptr(), cap, d_vad.data_ptr())
        ds.synchronize()
        pushes.append(dict(n_in=nb, want=want, n_out=n_out, out=d_out.cpu().numpy(), frames=d_frames.cpu().numpy(),
                           vad=d_vad.cpu().numpy(), volume=VOL0 if k < VOL_AT else VOL1))
        pos += nb
    ds.close()
    return pushes


def _frames_written(p):
    """Frames a push completed = the extent of d_frames48 that is no longer NaN (the same for every stream)."""
    written = ~np.isnan(p["frames"])
    assert (written == written[0]).all()
    nf = int(written[0].sum())
    assert nf % FRAME == 0 and written[0, :nf].all()
    return nf // FRAME


def _check_frames(B, rate, n):
    ref, acc = _reference48(B, rate, n)
    pushes = _pushed(B, rate, n)
    got = np.concatenate([p["frames"][:, :_frames_written(p) * FRAME] for p in pushes], axis=1)
    n_frames = ref.shape[1] // FRAME
    assert n_frames >= 4 and got.shape == (B, n_frames * FRAME), (got.shape, ref.shape)
    want = ref[:, :n_frames * FRAME] * np.float32(32768.0)
    for b in range(B):
        assert np.array_equal(got[b].view(np.uint32), want[b].view(np.uint32)), (rate, "stream", b, np.nonzero(got[b] != want[b])[0][:8])
    # n_out of every push: what crispy_rn_push_out_len said just before, and what the reference's counts give
    pos, done, first = 0, 0, True
    for p in pushes:
        pos += p["n_in"]
        frames = acc[pos] // FRAME - done
        done += frames
        expect = (frames - (1 if first and frames else 0)) * FRAME
        first = first and not frames
        assert p["n_out"] == p["want"] == expect, (rate, p["n_in"], p["n_out"], p["want"], expect)
        assert _frames_written(p) == frames
    assert any(p["n_out"] == 0 for p in pushes)


@pytest.mark.parametrize("rate,n", [(44100.0, 11025), (16000.0, 4800), (96000.0, 4800), (47999.0, 4800), (48000.0, 4800)])
def test_frames_are_the_references_bit_for_bit(rate, n):
    _check_frames(3, rate, n)


def _check_output(B, rate, n):
    pushes = _pushed(B, rate, n)
    twin = _mk(B)
    first, clamped = True, 0
    for p in pushes:
        nf = _frames_written(p)
        assert np.isnan(p["out"][:, p["n_out"]:]).all() and np.isnan(p["vad"][nf:]).all()
        if nf == 0:
            continue
        frames = np.ascontiguousarray(p["frames"][:, :nf * FRAME]).reshape(B, nf, FRAME)
        y, vad = twin.process(frames, layout="btf")                # the same number of frames per call as the push completed
        want = (np.clip(y / np.float32(32768.0), np.float32(-1.0), np.float32(1.0)) * np.float32(p["volume"])).astype(np.float32)
        want = want.reshape(B, nf * FRAME)[:, (FRAME if first else 0):]
        clamped += int((np.abs(y) >= 32768.0).sum())
        first = False
        got = p["out"][:, :p["n_out"]]
        assert got.shape == want.shape
        for b in range(B):
            assert np.array_equal(got[b].view(np.uint32), want[b].view(np.uint32)), (rate, "stream", b, p["n_in"])
        assert np.array_equal(p["vad"][:nf].view(np.uint32), vad.view(np.uint32))
    print(f"[rn push] B={B} rate={rate}: {clamped} samples clamped")
    twin.close()


@pytest.mark.parametrize("rate,n", [(44100.0, 11025), (16000.0, 4800), (96000.0, 4800), (47999.0, 4800), (48000.0, 4800)])
def test_output_is_process_frames_bit_for_bit(rate, n):
    _check_output(3, rate, n)


def test_splitting_does_not_matter():
    whole = _pushed(3, 44100.0, 11025, blocks=())
    assert len(whole) == 1
    split = _pushed(3, 44100.0, 11025)
    a = whole[0]["frames"][:, :_frames_written(whole[0]) * FRAME]
    b = np.concatenate([p["frames"][:, :_frames_written(p) * FRAME] for p in split], axis=1)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert whole[0]["n_out"] == sum(p["n_out"] for p in split)


def test_width_seventy_streams():
    """B is not a multiple of the wave; every stream has its own data and is checked on its own."""
    _check_frames(70, 44100.0, 2400)
    _check_output(70, 44100.0, 2400)


def test_host_entry_point_equals_the_device_one():
    B, rate, n = 3, 44100.0, 11025
    x = _data(B, n)
    ds = _mk(B)
    ds.adapter_configure(rate, VOL0)
    pos = 0
    for k, (nb, p) in enumerate(zip(_split(n), _pushed(B, rate, n))):
        if k == VOL_AT:
            ds.adapter_set_volume(VOL1)
        xin = np.ascontiguousarray(x[:, pos:pos + nb])
        nf = _frames_written(p)
        out = np.full((B, p["n_out"] + 5), np.nan, np.float32)            # a stride longer than the data
        vad = np.full((nf + 1, B), np.nan, np.float32)
        got = C.c_long(-1)
        rc = ds._L.crispy_rn_push(ds._h, xin.ctypes.data, nb, nb, out.ctypes.data, out.shape[1], vad.ctypes.data, C.byref(got))
        assert rc == 0, ds._L.crispy_last_error()
        assert got.value == p["n_out"]
        assert np.array_equal(out[:, :got.value].view(np.uint32), p["out"][:, :got.value].view(np.uint32))
        assert np.isnan(out[:, got.value:]).all()
        assert np.array_equal(vad[:nf].view(np.uint32), p["vad"][:nf].view(np.uint32)) and np.isnan(vad[nf:]).all()
        pos += nb
    ds.close()


def test_configure_resets_adapter_and_denoiser():
    B, rate = 3, 44100.0
    x = _data(B, 1441, seed=5)
    fresh = _mk(B)
    fresh.adapter_configure(rate, VOL0)
    want, want_vad = fresh.push(x, want_vad=True)
    assert want.shape == (B, 2 * FRAME) and want_vad.shape == (3, B)       # 1568 samples at 48 kHz: three frames, the first dropped
    used = _mk(B)
    used.adapter_configure(16000.0, 0.5)
    assert used.push(_data(B, 700, seed=6)).shape == (B, 3 * FRAME)        # leaves carried samples, resampler and denoiser state
    assert used.adapter_produced_rate_hz() == 48000.0
    used.adapter_configure(rate, VOL0)
    assert used.push_out_len(1441) == 2 * FRAME
    got, got_vad = used.push(x, want_vad=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_vad.view(np.uint32), want_vad.view(np.uint32))
    # a handle that was never configured: 48 kHz, volume 1
    plain, conf = _mk(B), _mk(B)
    conf.adapter_configure(48000.0, 1.0)
    assert plain.adapter_produced_rate_hz() == 48000.0 and plain.push_out_len(1000) == FRAME
    a, b = plain.push(x), conf.push(x)
    assert a.shape == (B, 2 * FRAME) and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    conf.adapter_configure(48000.4, 2.0)                                   # within 1 Hz: no resampler; volume clamped to 1
    assert conf.adapter_produced_rate_hz() == np.float32(48000.4)
    assert np.array_equal(conf.push(x).view(np.uint32), a.view(np.uint32))
    for h in (fresh, used, plain, conf):
        h.close()


def test_invalid_arguments_leave_the_handle_untouched():
    import torch
    B, n = 2, 1200
    x = _data(B, 2 * n, seed=9)
    h, twin = _mk(B), _mk(B)
    L = h._L
    d_x = torch.from_numpy(x).cuda()
    d_out = torch.zeros((B, 4 * FRAME), device="cuda")
    d_fr = torch.zeros((B, 4 * FRAME), device="cuda")
    torch.cuda.synchronize()
    got = C.c_long(-1)
    stride = d_x.shape[1]

    def push(hh, d_in, in_stride, n_in, out, out_stride, fr=None, fr_stride=0):
        return L.crispy_rn_push_device(hh._h, d_in, in_stride, n_in, out, out_stride, fr, fr_stride, None, C.byref(got), None)

    # first valid push on both: 1200 samples at 48 kHz = two frames, the first dropped
    for hh in (h, twin):
        assert push(hh, d_x.data_ptr(), stride, n, d_out.data_ptr(), 4 * FRAME) == 0 and got.value == FRAME
    bad = [
        ("n_in < 0", (d_x.data_ptr(), stride, -1, d_out.data_ptr(), 4 * FRAME)),
        ("in_stride", (d_x.data_ptr(), n - 1, n, d_out.data_ptr(), 4 * FRAME)),
        ("out_stride", (d_x.data_ptr(), stride, n, d_out.data_ptr(), 3 * FRAME - 1)),       # 240 carried + 1200: three frames
        ("frames_stride", (d_x.data_ptr(), stride, n, d_out.data_ptr(), 4 * FRAME, d_fr.data_ptr(), 3 * FRAME - 1)),
        ("NULL", (None, stride, n, d_out.data_ptr(), 4 * FRAME)),
        ("NULL", (d_x.data_ptr(), stride, n, None, 4 * FRAME)),
        ("overlaps", (d_x.data_ptr(), stride, n, d_x.data_ptr() + 64, stride)),
        ("overlaps", (d_x.data_ptr() + 64, stride, n, d_x.data_ptr(), stride)),
    ]
    for what, args in bad:
        assert push(h, *args) == -1, what
        msg = L.crispy_last_error().decode()
        assert "crispy_rn_push_device" in msg and what in msg, (what, msg)
    xh = np.ascontiguousarray(x[:, :n])
    oh = np.zeros((B, 4 * FRAME), np.float32)
    for what, args in [("n_in < 0", (xh.ctypes.data, n, -1, oh.ctypes.data, 4 * FRAME)), ("in_stride", (xh.ctypes.data, n - 1, n, oh.ctypes.data, 4 * FRAME)),
                       ("out_stride", (xh.ctypes.data, n, n, oh.ctypes.data, FRAME)), ("NULL", (None, n, n, oh.ctypes.data, 4 * FRAME)),
                       ("NULL", (xh.ctypes.data, n, n, None, 4 * FRAME))]:
        assert L.crispy_rn_push(h._h, *args, None, C.byref(got)) == -1, what
        msg = L.crispy_last_error().decode()
        assert "crispy_rn_push:" in msg and what in msg, (what, msg)
    assert L.crispy_rn_push_out_len(h._h, -1) < 0
    assert push(h, d_x.data_ptr(), stride, 0, d_out.data_ptr(), 4 * FRAME) == 0 and got.value == 0      # n_in == 0: a no-op
    # the next valid push gives the same bytes as on the untouched twin
    outs = []
    for hh in (h, twin):
        d_out.fill_(float("nan"))
        torch.cuda.synchronize()
        assert hh.push_out_len(n) == 3 * FRAME
        assert push(hh, d_x.data_ptr() + 4 * n, stride, n, d_out.data_ptr(), 4 * FRAME) == 0 and got.value == 3 * FRAME
        hh.synchronize()
        outs.append(d_out.cpu().numpy())
    assert not np.isnan(outs[0][:, :3 * FRAME]).any() and np.isnan(outs[0][:, 3 * FRAME:]).all()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    h.close()
    twin.close()


def test_process_does_not_touch_the_adapter_state():
    """crispy_rn_process on a configured handle equals an unconfigured twin fed the same frames, and a push around it
    continues with the carried samples it had."""
    B = 2
    frames = (_data(B, 3 * FRAME, seed=11) * np.float32(20000.0)).reshape(B, 3, FRAME)
    x = _data(B, 700, seed=12)
    conf, plain = _mk(B), _mk(B)
    conf.adapter_configure(44100.0, 0.5)
    a, va = conf.process(frames, layout="btf")
    b, vb = plain.process(frames, layout="btf")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    # 300 + (process) + 400 samples against 700 at once: the same frames reach process_frame
    import torch
    res = []
    for pieces in ((300, 400), (700,)):
        h = _mk(B)
        h.adapter_configure(44100.0, 0.5)
        d_x = torch.from_numpy(x).cuda()
        d_fr = torch.full((B, 2 * FRAME), float("nan"), device="cuda")
        d_out = torch.zeros((B, 2 * FRAME), device="cuda")
        torch.cuda.synchronize()
        pos, cols = 0, 0
        for nb in pieces:
            if pos:
                h.process(frames, layout="btf")
            h.push_device(d_x.data_ptr() + 4 * pos, 700, nb, d_out.data_ptr(), 2 * FRAME, d_fr.data_ptr() + 4 * cols, 2 * FRAME)
            h.synchronize()
            cols = int((~torch.isnan(d_fr[0])).sum())
            pos += nb
        res.append(d_fr.cpu().numpy())
        h.close()
    assert not np.isnan(res[1][:, :FRAME]).any() and np.isnan(res[1][:, FRAME:]).all()
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    conf.close()
    plain.close()


def test_push_block_equals_push_sample():
    """RnnNoiseProcessor.push_block against push_sample called sample by sample on a twin: B = 2, 44.1 kHz, 2205 samples in
    pieces of 400 (435 or 436 samples at 48 kHz: at most one frame per piece, as push_sample completes them)."""
    import torch
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import RnnNoiseProcessor
    B, rate, n, vol = 2, 44100.0, 2205, 0.7
    x = _data(B, n, seed=21)
    block = RnnNoiseProcessor(synthetic_weights(0), rate, 48000.0, vol, n_streams=B)
    single = RnnNoiseProcessor(synthetic_weights(0), rate, 48000.0, vol, n_streams=B)
    fed = []
    inner = single.denoise.process_frame
    single.denoise.process_frame = lambda out, inp: (fed.append(inp.copy()), inner(out, inp))[1]
    want = [o for o in (single.push_sample(x[:, i]) for i in range(n)) if o is not None]
    want = np.concatenate(want, axis=0).T                                  # [B, n_out]
    got = np.concatenate([block.push_block(x[:, p:p + 400]) for p in range(0, n, 400)], axis=1)
    assert want.shape == got.shape == (B, 3 * FRAME)                       # 2399 samples at 48 kHz: four frames, the first dropped
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    # the frames process_frame saw, through the entry point push_block is built on
    h = _mk(B)
    h.adapter_configure(rate, vol)
    d_x = torch.from_numpy(x).cuda()
    d_fr = torch.full((B, 5 * FRAME), float("nan"), device="cuda")
    d_out = torch.zeros((B, 5 * FRAME), device="cuda")
    torch.cuda.synchronize()
    h.push_device(d_x.data_ptr(), n, n, d_out.data_ptr(), 5 * FRAME, d_fr.data_ptr(), 5 * FRAME)
    h.synchronize()
    frames = d_fr.cpu().numpy()[:, :4 * FRAME].reshape(B, 4, FRAME)
    assert len(fed) == 4
    for t in range(4):
        assert np.array_equal(frames[:, t].view(np.uint32), np.ascontiguousarray(fed[t]).view(np.uint32)), t
    h.close()

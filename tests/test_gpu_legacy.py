"""GPU tests of NsState's Legacy arm and of the model switch (crispy_rn_model_configure, include/crispy_hip.h): SharedAudio
(src-tauri/src/audio.rs:136-200) behind crispy_rn_push* / crispy_rn_pull* / crispy_rn_capture*, push_mono_to_buffers' recording
resampler behind the push (audio.rs:701-726), and set_monitoring_model (audio.rs:942-967), for every stream of a handle at once.

Everything is compared bit for bit against tests/legacy_oracle.py (where the oracle's value is a NaN, the GPU's is a NaN); the
RNNoise steps of a script against a second handle that never heard of models.  Sizes are the smallest at which each mechanism
can go wrong: 1, 3, 4, 7 (a lane's group of four and its partial forms), 1025 (the push tile is 1024), rows with and without
16-byte alignment, 70 001 samples for the high bits of the jump-ahead, a ring of 16 000 for the eviction."""
import ctypes as C

import numpy as np
import pytest

from tests import capture_oracle as CO
from tests import legacy_oracle as LO
from tests import playback_oracle as PO
from tests import record_oracle as RO

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID = -1           # CRISPY_ERR_INVALID_ARG
SIZES = (1, 3, 4, 7, 480, 1025, 4410)
RNNOISE, DUMMY, NOISY = 0, 1, 2


def _mk(B, rate, volume, model=None, output_rate=None, ring_samples=None, bypass=None):
    from crispy_amd import synthetic_weights
    from crispy_amd.denoise import DenoiseState
    ds = DenoiseState(synthetic_weights(0), B, 0)
    ds.adapter_configure(rate, volume)
    if output_rate is not None:
        ds.playback_configure(output_rate)
    if ring_samples is not None:
        ds.record_configure(ring_samples)
    if bypass is not None:
        ds.bypass_configure(bypass)
    if model is not None:
        ds.model_configure(model)
    return ds


def _data(B, n, seed=0):
    """Every stream its own samples in +-1.5, beyond +-1 so that the output clamps have work."""
    return np.random.default_rng(seed).uniform(-1.5, 1.5, size=(B, n)).astype(F32)


def _check(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    for b in range(want.shape[0]):
        assert LO.same_bits(got[b], want[b]), (what, "stream", b, np.nonzero(got[b] != want[b])[0][:8])


def _push_dev(ds, x, in_stride, out_stride):
    """One crispy_rn_push_device over device copies with those row strides -> out [B, n_out]; the rest of every row must stay
    as it was."""
    import torch
    B, n = x.shape
    rows = np.full((B, in_stride), 7.0, dtype=F32)
    rows[:, :n] = x
    d_in = torch.from_numpy(rows).cuda()
    d_out = torch.full((B, out_stride), -9.0, dtype=torch.float32, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    assert ds.push_out_len(n) == n
    torch.cuda.synchronize()              # the handle enqueues on a stream of its own
    n_out = ds.push_device(d_in.data_ptr(), in_stride, n, d_out.data_ptr(), out_stride)
    ds.synchronize()
    out = d_out.cpu().numpy()
    assert n_out == n and (out[:, n_out:] == F32(-9.0)).all()
    return np.ascontiguousarray(out[:, :n_out])


def _pull_dev(ds, n_frames, channels, fmt, stride):
    """One crispy_rn_pull_device into rows of `stride` elements -> (out [B, n_frames * channels], n_live)."""
    import torch
    dtype = {"f32": np.float32, "i16": np.int16, "u16": np.uint16}[fmt]
    item, n = np.dtype(dtype).itemsize, n_frames * channels
    d_out = torch.full((ds.n_streams, stride * item), 0x7F, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    live = ds.pull_device(n_frames, d_out.data_ptr(), stride, channels, fmt)
    ds.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[:, n * item:] == 0x7F).all()
    return np.ascontiguousarray(raw[:, :n * item]).view(dtype), live


def _strides(n):
    """(rows that stay 16-byte aligned, rows that do not)."""
    return (n + 3) // 4 * 4, (n + 3) // 4 * 4 + 1


# ---- 1: the dummy push is x * volume ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,volume", [(3, 1.0), (3, 0.37), (3, 0.0), (5, 0.37)])
def test_dummy_push_is_x_times_volume(B, volume):
    ds = _mk(B, 48000.0, volume, DUMMY)
    assert ds.model() == DUMMY and ds.adapter_produced_rate_hz() == 48000.0
    for k, n in enumerate(SIZES):
        x = _data(B, n, seed=k)
        x[0, 0] = F32(-0.0)
        if n >= 4:
            x[1, 1], x[B - 1, 2], x[0, 3], x[1, n - 1] = F32(np.inf), F32(-np.inf), F32(np.nan), F32(-0.0)
        with np.errstate(invalid="ignore"):
            want = x * F32(volume)
        for in_stride, out_stride in (_strides(n), _strides(n)[::-1], (_strides(n)[0],) * 2, (_strides(n)[1],) * 2):
            _check(_push_dev(ds, x, in_stride, out_stride), want, (n, in_stride, out_stride))
        _check(ds.push(x), want, ("host", n))
    assert ds.playback_buffered() == 0          # no playback configured: nothing is kept
    ds.close()


# ---- 2: the noisy push ------------------------------------------------------------------------------------------------------
def test_noisy_pushes_back_to_back_carry_the_lcg():
    """The sizes back to back, so that a push starts anywhere in the sequence (not at a multiple of 4), alternately through
    aligned and unaligned rows; then 70 001 samples in one push: tiles from the 69th on use the jump-ahead's bit 16."""
    B, volume = 3, 0.37
    ds = _mk(B, 44100.0, volume, NOISY, output_rate=48000.0)
    orc = LO.SharedAudioOracle(B, 44100.0, 48000.0, True, volume)
    for k, n in enumerate(SIZES + (70001,)):
        x = _data(B, n, seed=10 + k)
        s = _strides(n)
        got = _push_dev(ds, x, s[k % 2], s[(k + 1) % 2]) if k % 3 else ds.push(x)
        _check(got, orc.push(x), n)
        assert ds.playback_buffered() == len(orc)
    assert orc.rng == LO.lcg_after(LO.LCG_SEED, sum(SIZES) + 70001) and orc.evictions > 0
    ds.close()


def test_noisy_push_at_volume_zero_is_the_noise_term():
    B = 3
    ds = _mk(B, 48000.0, 0.0, NOISY)
    L = ds._L
    state = LO.LCG_SEED
    for n in (1, 7, 1025):
        noise = np.empty(n, dtype=F32)
        nxt = L.crispy_ns_noise_state(state, n, noise.ctypes.data)
        got = ds.push(_data(B, n, seed=n))
        assert nxt == LO.lcg_naive(state, n)
        x = _data(B, n, seed=n)
        _check(got, x * F32(0.0) + (noise * F32(0.05))[None, :], n)
        state = nxt
    ds.close()


# ---- 3: playback ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [DUMMY, NOISY])
@pytest.mark.parametrize("in_rate,out_rate", [(44100.0, 48000.0), (48000.0, 44100.0), (16000.0, 48000.0), (48000.0, 48000.0)])
def test_playback_is_next_sample(in_rate, out_rate, model):
    B = 3
    ds = _mk(B, in_rate, 0.8, model, output_rate=out_rate)
    orc = LO.SharedAudioOracle(B, in_rate, out_rate, model == NOISY, 0.8)
    assert ds.adapter_produced_rate_hz() == in_rate

    def push(n, seed):
        x = _data(B, n, seed)
        _check(ds.push(x), orc.push(x), ("push", n))
        assert ds.playback_buffered() == len(orc)

    def pull(n, channels=1, fmt="f32", stride=None):
        want, want_live = orc.pull(n)
        if stride is None:
            got, live = ds.pull(n, channels, fmt, want_live=True)
        else:
            got, live = _pull_dev(ds, n, channels, fmt, stride)
        _check(got, PO.convert(want, fmt, channels), ("pull", n, channels, fmt, stride))
        assert live == want_live and ds.playback_buffered() == len(orc)
        return live

    # before any push, and with one sample: zeros -- 32767 as u16
    assert pull(5) == 0
    got = ds.pull(3, 2, "u16")
    assert (got == 32767).all()
    orc.pull(3)
    push(1, 0)
    assert pull(4, 2, "i16") == 0
    push(300, 1)
    assert pull(100) == 100
    ds.adapter_set_volume(0.37)           # the ring holds raw samples: the pull takes the new volume
    orc.set_volume(0.37)
    assert pull(50, 2, "i16") == 50
    # runs dry part way: a live prefix, then zeros that advance neither the position nor the LCG
    live = pull(1200, 8, "u16")
    assert 0 < live < 1200 and orc.zeros > 0
    rng_before = orc.rng
    assert pull(3) == 0 and orc.rng == rng_before
    push(37, 2)                           # Noisy: the next push's noise is the oracle's
    push(900, 3)
    ds.adapter_set_volume(1.0)
    orc.set_volume(1.0)
    seen = set()
    for channels in (1, 2, 8):
        for fmt in ("f32", "i16", "u16"):
            n = 33
            aligned = (n * channels + 15) // 16 * 16
            pull(n, channels, fmt, stride=aligned)            # 16-byte stores with a partial last piece
            pull(9, channels, fmt, stride=9 * channels + 1)   # rows that are not aligned
            seen.add((channels, fmt))
    assert len(seen) == 9
    # single-frame pulls: the first frame of a pull pops what the frame before left -- several samples when the step is above 1
    push(200, 4)
    drops = []
    for _ in range(40):
        before = len(orc)
        pull(1)
        drops.append(before - len(orc))
    assert max(drops) >= (2 if in_rate > out_rate else 1), drops
    ds.close()


# ---- 4: eviction ------------------------------------------------------------------------------------------------------------
def test_ring_eviction_keeps_the_last_second():
    """Rate 16 000: the ring holds 16 000 raw samples.  Three pushes of 7000 -- the third wraps and evicts --, then one of
    20 000, of which only the last 16 000 survive; pulls in between move the head."""
    B = 3
    ds = _mk(B, 16000.0, 0.9, NOISY, output_rate=48000.0)
    orc = LO.SharedAudioOracle(B, 16000.0, 48000.0, True, 0.9)
    for k, n in enumerate((7000, 7000, 7000, 20000)):
        x = _data(B, n, seed=20 + k)
        _check(ds.push(x), orc.push(x), ("push", k))
        assert ds.playback_buffered() == len(orc)
        want, want_live = orc.pull(901)
        got, live = ds.pull(901, want_live=True)
        _check(got, want, ("pull", k))
        assert live == want_live == 901 and ds.playback_buffered() == len(orc)
    assert orc.evictions >= 4000 + 1 and len(orc) < 16000
    x = _data(B, 16000, seed=30)          # exactly the cap: everything that was there goes
    _check(ds.push(x), orc.push(x), "cap")
    want, _ = orc.pull(3 * 16000 + 10)    # ... and the whole ring read back, to the underrun
    got, live = ds.pull(3 * 16000 + 10, want_live=True)
    _check(got, want, "all")
    assert ds.playback_buffered() == len(orc) and 0 < live < 3 * 16000 + 10
    ds.close()


@pytest.mark.parametrize("rate", [16000.0, 44100.0])
def test_playback_configured_on_a_legacy_handle_sizes_the_ring_from_the_raw_rate(rate):
    """crispy_rn_playback_configure AFTER the model: the ring of a Legacy handle holds `rate as usize` raw samples, not the
    48 000 the RNNoise arm of a resampling handle has.  One sample more than the cap evicts exactly one; blocks that are
    multiples of four at an aligned tail take the push's 16-byte ring stores, the odd ones its single stores."""
    B, cap = 3, int(rate)
    ds = _mk(B, rate, 0.9)
    ds.model_configure(DUMMY)
    ds.playback_configure(48000.0)
    orc = LO.SharedAudioOracle(B, rate, 48000.0, False, 0.9)
    for k, n in enumerate((cap - 8, 8, 1, 4, 1023, cap + 5)):
        x = _data(B, n, seed=90 + k)
        _check(ds.push(x), orc.push(x), ("push", n))
        assert ds.playback_buffered() == len(orc) == min(cap, sum((cap - 8, 8, 1, 4, 1023, cap + 5)[:k + 1]))
    assert orc.evictions == 1 + 4 + 1023 + cap + 5
    n_pull = 3 * cap + 10                     # the whole ring read back, to the underrun
    want, want_live = orc.pull(n_pull)
    got, live = ds.pull(n_pull, want_live=True)
    _check(got, want, "all")
    assert live == want_live and 0 < live < n_pull and ds.playback_buffered() == len(orc)
    ds.close()


# ---- 5: the model switch ----------------------------------------------------------------------------------------------------
def test_model_switch_script():
    """set_monitoring_model on a 44.1 kHz handle with playback and recording.  The RNNoise steps are checked against a twin
    handle that never heard of models and is given a fresh processor (crispy_rn_adapter_configure) where the script switches
    to RNNoise; the Legacy steps and the recording resampler behind every step against the oracle."""
    B, rate, vol = 3, 44100.0, 0.8
    ds = _mk(B, rate, vol, output_rate=48000.0, ring_samples=0)
    twin = _mk(B, rate, vol, output_rate=48000.0)
    rec = RO.RecordOracle(B)
    cb = LO.CallbackOracle(B, rate, rec)
    state = dict(orc=None, seed=40)

    def fresh(model):
        ds.model_configure(model)
        assert ds.model() == model and ds.playback_buffered() == 0
        if model == RNNOISE:
            twin.adapter_configure(rate, vol)
            state["orc"] = None
            assert ds.adapter_produced_rate_hz() == 48000.0
        else:
            state["orc"] = LO.SharedAudioOracle(B, rate, 48000.0, model == NOISY, vol)
            assert ds.adapter_produced_rate_hz() == rate

    def push(n):
        state["seed"] += 1
        x = _data(B, n, state["seed"])
        orc = state["orc"]
        assert ds.push_out_len(n) == (n if orc is not None else twin.push_out_len(n))
        got = ds.push(x)
        if orc is not None:
            _check(got, orc.push(x), ("legacy push", n))
            cb.feed(orc.produced_rate_hz(), got)
            assert ds.playback_buffered() == len(orc)
        else:
            _check(got, twin.push(x), ("rnnoise push", n))
            cb.feed(48000.0, got)
            assert ds.playback_buffered() == twin.playback_buffered()
        assert ds.record_buffered()[0] == len(rec.mic)
        return got.shape[1]

    def pull(n):
        orc = state["orc"]
        want, want_live = orc.pull(n) if orc is not None else twin.pull(n, want_live=True)
        got, live = ds.pull(n, want_live=True)
        _check(got, want, ("pull", n))
        assert live == want_live

    assert ds.model() == RNNOISE
    assert push(2000) > 0 and cb.resets == 1          # RNNoise at 44.1 kHz produces 48000: the resampler passes through
    fresh(DUMMY)
    push(1000)
    assert cb.resets == 2                             # ... and 44100 again: reset at the first Legacy sample
    pull(200)
    fresh(NOISY)
    push(777)
    pull(100)
    assert cb.resets == 2                             # dummy <-> noisy at one rate: no reset, the positions carry on
    rng_used = state["orc"].rng
    fresh(NOISY)                                      # another fresh processor: the LCG restarts, the ring is empty
    assert rng_used != LO.LCG_SEED
    push(3)
    pull(2)
    fresh(NOISY)
    fresh(RNNOISE)                                    # a double switch with no push in between
    assert push(500) == 0 and cb.resets == 2          # the first frame is dropped: nothing returned, the resampler is left alone
    fresh(DUMMY)
    push(301)
    assert cb.resets == 2                             # so this push continues where the noisy one stopped
    fresh(RNNOISE)
    assert push(2000) > 0 and cb.resets == 3
    pull(300)
    fresh(NOISY)
    push(1153)
    assert cb.resets == 4
    # the mic ring, by a drain at the end
    want = rec.drain()            # (no app audio: the worker trims the mic deque to 2400 samples, two frames)
    assert want.shape[1] == 2 * RO.FRAME * 2 and rec.mic_trim > 3000
    _check(ds.record_drain(), want, "drain")
    assert ds.record_buffered()[0] == len(rec.mic)
    ds.close()
    twin.close()


# ---- 6: capture in the Legacy arm -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100.0, 48000.0])
@pytest.mark.parametrize("fmt,channels", [("i16", 2), ("f32", 1)])
def test_capture_is_mono_level_and_the_legacy_push(fmt, channels, rate):
    import torch
    B, vol = 3, 0.6
    cap = _mk(B, rate, vol, NOISY, output_rate=48000.0, ring_samples=0)
    ref = _mk(B, rate, vol, NOISY, output_rate=48000.0, ring_samples=0)       # conversion on the host, crispy_rn_level, crispy_rn_push
    orc = LO.SharedAudioOracle(B, rate, 48000.0, True, vol)
    rec = RO.RecordOracle(B)
    cb = LO.CallbackOracle(B, rate, rec)
    rng = np.random.default_rng(50)
    for k, n in enumerate((1, 441, 1025)):
        if fmt == "i16":
            x = rng.integers(-32768, 32768, size=(B, n * channels)).astype(np.int16)
        else:
            x = rng.uniform(-1.5, 1.5, size=(B, n * channels)).astype(F32)
        mono = CO.capture_mono(x, channels)
        want = orc.push(mono)
        cb.feed(rate, want)
        assert cap.capture_out_len(n) == n
        if k == 1:      # device pointers, with the mono handed out
            d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            d_out = torch.full((B, n + 2), -9.0, dtype=torch.float32, device="cuda")
            d_mono = torch.full((B, n + 3), -9.0, dtype=torch.float32, device="cuda")
            d_rms = torch.full((B,), -9.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            n_out = cap.capture_device(d_in.data_ptr(), n * channels, n, channels, fmt, d_out.data_ptr(), n + 2, d_mono.data_ptr(), n + 3,
                                       d_rms.data_ptr())
            cap.synchronize()
            assert n_out == n
            out, got_mono, rms = d_out.cpu().numpy(), d_mono.cpu().numpy(), d_rms.cpu().numpy()
            assert (out[:, n:] == F32(-9.0)).all() and (got_mono[:, n:] == F32(-9.0)).all()
            _check(np.ascontiguousarray(got_mono[:, :n]), mono, "mono")
            out = np.ascontiguousarray(out[:, :n])
        else:
            out, rms = cap.capture(x, channels)
        _check(out, want, ("out", n))
        _check(rms[None, :], RO.level(mono)[None, :], ("rms", n))
        _check(ref.level(mono)[None, :], rms[None, :], ("level", n))
        _check(ref.push(mono), want, ("ref push", n))
        assert cap.playback_buffered() == ref.playback_buffered() == len(orc)
        assert cap.record_buffered() == ref.record_buffered() == (len(rec.mic), 0)
    # the handle afterwards is as after conversion + crispy_rn_level + crispy_rn_push
    want, want_live = orc.pull(200)
    for ds in (cap, ref):
        got, live = ds.pull(200, want_live=True)
        _check(got, want, "pull")
        assert live == want_live
    mono = _data(B, 3000, 51)
    want = orc.push(mono)
    cb.feed(rate, want)
    _check(cap.push(mono), want, "push after")
    _check(ref.capture(mono, 1)[0], want, "capture after")
    want = rec.drain()
    assert want.shape[1] >= RO.FRAME * 2
    _check(cap.record_drain(), want, "drain")
    _check(ref.record_drain(), want, "ref drain")
    cap.close()
    ref.close()


def test_a_bypassed_capture_ignores_the_model():
    B, rate = 3, 44100.0
    ds = _mk(B, rate, 0.6, NOISY, output_rate=48000.0, ring_samples=0, bypass=rate)
    rec = RO.RecordOracle(B)
    orc = CO.BypassOracle(B, rate, rec)
    for n in (7, 1025):
        x = _data(B, n, 60 + n)
        out, _ = ds.capture(x, 1)
        _check(out, orc.capture(CO.capture_mono(x, 1)), n)
    assert ds.playback_buffered() == 0 and ds.record_buffered()[0] == len(rec.mic) and ds.model() == NOISY
    ds.close()


# ---- 7: nothing changes for RNNoise -----------------------------------------------------------------------------------------
def test_rnnoise_model_is_the_handle_as_it_was():
    """One 44.1 kHz script on a handle told to be CRISPY_NS_RNNOISE and on one that never heard of models: identical bytes from
    push / pull / capture / drain, and the pushes equal the RnnNoiseProcessor restatement tests/test_gpu_rn_push.py uses: the
    Python LinearResampler per stream, x 32768, crispy_rn_process on a third handle, / 32768, clamp, volume, first frame dropped."""
    from crispy_amd.denoise import LinearResampler
    B, rate, vol, FRAME = 3, 44100.0, 0.8, 480
    told = _mk(B, rate, vol, output_rate=48000.0, ring_samples=0)
    told.model_configure(RNNOISE)
    plain = _mk(B, rate, vol, output_rate=48000.0, ring_samples=0)
    assert told.model() == plain.model() == RNNOISE
    x = _data(B, 441 + 1000 + 4410, 70)
    x16 = np.random.default_rng(71).integers(-32768, 32768, size=(B, 2 * 900)).astype(np.int16)
    outs = []
    for ds in (told, plain):
        got, pos = [], 0
        for n in (441, 1000, 4410):
            assert ds.push_out_len(n) % FRAME == 0
            got.append(ds.push(x[:, pos:pos + n]))
            pos += n
        got.append(ds.pull(700, 2, "i16"))
        got.append(ds.capture(x16, 2)[0])
        got.append(ds.capture(x16, 2)[1][None, :])
        got.append(ds.pull(100))
        got.append(ds.record_drain())
        outs.append(got)
        assert ds.adapter_produced_rate_hz() == 48000.0
    for k, (a, b) in enumerate(zip(*outs)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    assert outs[0][2].shape[1] > 0 and outs[0][7].shape[1] > 0
    # the restatement of the pushes
    rows, acc = [], None
    for b in range(B):
        rs, out, counts = LinearResampler(rate, 48000.0), [], [0]
        for s in x[b]:
            rs.process_sample(s, out.append)
            counts.append(len(out))
        rows.append(np.array(out, dtype=F32))
        assert acc is None or acc == counts      # lock-stepped streams: the positions do not depend on the samples
        acc = counts
    ref48 = np.stack(rows)
    twin = _mk(B, 48000.0, 1.0)
    done, first, pos = 0, True, 0
    for k, n in enumerate((441, 1000, 4410)):
        pos += n
        nf = acc[pos] // FRAME - done            # frames this push completed
        assert outs[0][k].shape[1] == (nf - (1 if first and nf else 0)) * FRAME
        if nf == 0:
            continue
        frames = np.ascontiguousarray(ref48[:, done * FRAME:(done + nf) * FRAME] * F32(32768.0)).reshape(B, nf, FRAME)
        y, _ = twin.process(frames, layout="btf")
        want = (np.clip(y / F32(32768.0), F32(-1.0), F32(1.0)) * F32(vol)).astype(F32).reshape(B, nf * FRAME)[:, (FRAME if first else 0):]
        first = False
        done += nf
        _check(outs[0][k], want, ("restated push", k))
    assert done >= 10
    for ds in (told, plain, twin):
        ds.close()


# ---- 8: errors leave the state alone ----------------------------------------------------------------------------------------
def test_errors_leave_the_state_alone():
    import torch
    B = 3
    ds = _mk(B, 44100.0, 0.7, NOISY, output_rate=48000.0)
    orc = LO.SharedAudioOracle(B, 44100.0, 48000.0, True, 0.7)
    L = ds._L

    def valid(n, seed):
        x = _data(B, n, seed)
        _check(ds.push(x), orc.push(x), ("push", n))
        want, want_live = orc.pull(n // 2)
        got, live = ds.pull(n // 2, want_live=True)
        _check(got, want, ("pull", n))
        assert live == want_live and ds.playback_buffered() == len(orc)

    valid(100, 80)
    d_in = torch.zeros((B, 8), dtype=torch.float32, device="cuda")
    d_out = torch.full((B, 8), -9.0, dtype=torch.float32, device="cuda")
    d_side = torch.full((B, 480), -9.0, dtype=torch.float32, device="cuda")
    got = C.c_long(5)
    torch.cuda.synchronize()
    for frames48, vad in ((d_side.data_ptr(), None), (None, d_side.data_ptr())):
        rc = L.crispy_rn_push_device(ds._h, d_in.data_ptr(), 8, 8, d_out.data_ptr(), 8, frames48, 480, vad, C.byref(got), None)
        assert rc == INVALID and got.value == 0
        assert L.crispy_last_error().decode().startswith("crispy_rn_push_device:")
    host_in, host_out, host_vad = np.zeros((B, 8), F32), np.zeros((B, 8), F32), np.zeros((1, B), F32)
    assert L.crispy_rn_push(ds._h, host_in.ctypes.data, 8, 8, host_out.ctypes.data, 8, host_vad.ctypes.data, C.byref(got)) == INVALID
    assert L.crispy_last_error().decode().startswith("crispy_rn_push:")
    ds.synchronize()
    assert (d_out.cpu().numpy() == F32(-9.0)).all() and (d_side.cpu().numpy() == F32(-9.0)).all()
    valid(57, 81)
    assert L.crispy_rn_model_configure(ds._h, 3) == INVALID
    assert L.crispy_last_error().decode().startswith("crispy_rn_model_configure:") and ds.model() == NOISY
    valid(33, 82)
    # a pull on a Legacy handle without playback
    bare = _mk(B, 44100.0, 0.7, DUMMY)
    out = np.zeros((B, 4), F32)
    assert L.crispy_rn_pull(bare._h, 4, 1, 0, out.ctypes.data, 4, None) == INVALID
    assert L.crispy_last_error().decode().startswith("crispy_rn_pull:")
    x = _data(B, 9, 83)
    _check(bare.push(x), x * F32(0.7), "bare")
    ds.close()
    bare.close()

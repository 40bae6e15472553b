"""The log-mel front end (crispy_amd/csrc/mel_kernels.hip, fft_lds.h, the table builder of crispy_mel_create) held to
float32 accuracy stage by stage, beside the parity tests of tests/test_gpu_logmel.py, which allow 1e-4 of the peak.

Signals, both references and the statistic are those of tests/mel_cases.py (checked on the CPU by tests/test_mel_cases.py).
The bound is the project's rule for a float32 stage (tests/test_gpu_diar_*): D_gpu <= FACTOR x D of a float32 restatement on
the same clip, FACTOR = 4.  Clips are scaled by a power of two until nothing clamps; then the public output gives back the
frame kernel's floats bit for bit, raw = 4 out - 4.  (a) the edges of the framing, the tiles and the batch; (b) the
transform bin by bin through identity filter banks; (c) every filter tap and the sparse table's limits; (d) the clip
maximum from every position of a wave, a tile and the batch; (e) the same clips loud, through the clamp; (f) the frame
kernel's log10 through crispy_mel_stage_log10_device against float64."""
import numpy as np
import pytest

from tests import mel_cases as MC

pytestmark = pytest.mark.gpu

FACTOR = MC.FACTOR
PAD = -1.5                   # (-10 + 4) / 4: a frame of zeros where nothing clamps
ERR_INVALID_ARG, ERR_BAD_MODEL = -1, -5


@pytest.fixture(scope="module")
def mel():
    """bank name -> (LogMel, filters), one handle per bank for the module"""
    from crispy_amd.asr import LogMel
    made = {}

    def get(b):
        if b not in made:
            F = MC.bank(b)
            made[b] = (LogMel(F.shape[0], F), F)
        return made[b]
    yield get
    for lm, _ in made.values():
        lm.close()


_quiet = {}


def quiet_edge_clips(b, F):
    """(a)'s clips at the quiet scale, their exponents and references: computed once per bank, shared by (a) and (e)"""
    if b not in _quiet:
        xs, ks = zip(*(MC.quiet(MC.edge_clip(n), F) for n in MC.LENGTHS))
        _quiet[b] = (list(xs), list(ks), [MC.Ref(x, F) for x in xs])
    return _quiet[b]


def run(lm, clips, transposed=False):
    """One crispy_mel_compute_device call -> d_out [B, n_mel, 3000] (and d_out_t [B, 3002, n_mel]), device tensors"""
    import torch
    lens = np.array([c.size for c in clips], np.int32)
    pcm = np.zeros((len(clips), int(lens.max())), np.float32)
    for i, c in enumerate(clips):
        pcm[i, :c.size] = c
    d_pcm = torch.from_numpy(pcm).cuda()
    d_out = torch.empty(len(clips), lm.n_mel, 3000, device="cuda")
    d_out_t = None
    if transposed:
        d_out_t = torch.full((len(clips), 3002, lm.n_mel), 7.0, device="cuda")
        d_out_t[:, 0] = 0.0
        d_out_t[:, -1] = 0.0
    torch.cuda.synchronize()
    lm.compute_device(d_pcm.data_ptr(), pcm.shape[1], lens, d_out=d_out.data_ptr(),
                      d_out_t=d_out_t.data_ptr() if transposed else 0)
    lm.synchronize()
    return (d_out, d_out_t) if transposed else d_out


def check(what, raw, ref):
    """The floor rule and D_gpu <= FACTOR x D_float32 for one clip; raw [n_mel, ref.T] float32.  -> the ratio"""
    assert raw.shape == ref.M.shape and raw.dtype == np.float32
    d = ref.D(raw)
    print(f"{what}: D gpu {d:.2e}, float32 reference {ref.D32:.2e}, ratio {d / ref.D32:.2f}")
    assert MC.floor_ok(raw, ref.M), what
    assert d <= FACTOR * ref.D32, (what, d, ref.D32)
    return d / ref.D32


def quiet_raw(d_out_b, ref, what):
    """The frame kernel's floats of a quiet clip from its output; every frame past the audio is the floor."""
    import torch
    assert bool(torch.all(d_out_b[:, ref.T:] == PAD)), what
    return MC.out_to_raw(d_out_b[:, :ref.T].cpu().numpy())


# ---- (a) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ["80", "128"])
def test_a_frame_kernel_at_every_edge(mel, b):
    """Lengths 1 .. 40123: the reflected start (below 201 samples it runs past the clip's end), less than one frame, a last
    frame that sees one sample (9881, 10041), the first tile's last frame and the next (9880 | 9881 .. 10040 | 10041 samples:
    63 | 64 | 65 live frames), the 16-frame wave shares and 4-frame groups.  Every clip alone and inside one ragged batch of all: the same bits; the frame-major copy: the
    same bits transposed."""
    import torch
    lm, F = mel(b)
    clips, _, refs = quiet_edge_clips(b, F)
    d_out, d_out_t = run(lm, clips, transposed=True)
    assert torch.equal(d_out_t[:, 1:-1], d_out.transpose(1, 2))
    assert bool(torch.all(d_out_t[:, 0] == 0)) and bool(torch.all(d_out_t[:, -1] == 0))
    for i, (n, x, ref) in enumerate(zip(MC.LENGTHS, clips, refs)):
        assert ref.T == MC.live_frames(n)
        check(f"(a) {b} mels, {n} samples", quiet_raw(d_out[i], ref, n), ref)
        solo = run(lm, [x])
        assert torch.equal(solo[0].view(torch.int32), d_out[i].view(torch.int32)), f"{n} samples: alone and in the batch differ"


@pytest.mark.parametrize("b", ["80", "128"])
def test_a_long_path_windows(mel, b):
    """485000 samples (3033 live frames, rows of 48 tiles) through crispy_mel_compute_long_device, windows at seek 0 and 2990."""
    import torch
    lm, F = mel(b)
    x, _ = MC.quiet(MC.edge_clip(MC.N_LONG), F)
    ref = MC.Ref(x, F)
    assert ref.T == 3033
    d_pcm = torch.from_numpy(x).cuda()
    w = torch.empty(2, lm.n_mel, 3000, device="cuda")
    torch.cuda.synchronize()
    lm.compute_long_device(d_pcm.data_ptr(), x.size, np.array([x.size], np.int32))
    for k, seek in enumerate((0, 2990)):
        lm.window_device([0], [seek], d_out=w[k].data_ptr())
    lm.synchronize()
    w = w.cpu().numpy()
    assert np.array_equal(w[1][:, :10].view(np.uint32), w[0][:, 2990:].view(np.uint32))
    assert np.all(w[1][:, ref.T - 2990:] == np.float32(PAD))
    raw = MC.out_to_raw(np.concatenate([w[0], w[1][:, 10:ref.T - 2990]], axis=1))
    check(f"(a) {b} mels, {MC.N_LONG} samples, long path", raw, ref)


# ---- (b) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ["id0", "id73"])
def test_b_transform_bin_by_bin(mel, b):
    """Identity banks: row m is the power of bin m (id0) or 73 + m (id73).  A noise-plus-chirp clip, and single samples at
    offsets 1, 2, 199, 200, 201, 398, 399 of interior frames -- both members of the (x[2m], x[2m + 1]) packing; the frames
    that see an impulse under hann[1] or hann[399] lie below the floor and must be exactly -10.  Per clip as everywhere,
    and every bin on its own within FACTOR x the float32 reference's worst bin."""
    lm, F = mel(b)
    clips = [MC.quiet(MC.signal(5, 8000), F)[0], MC.quiet(MC.impulse_clip(), F)[0]]
    d_out = run(lm, clips)
    for i, what in enumerate(("signal", "impulses")):
        ref = MC.Ref(clips[i], F)
        raw = quiet_raw(d_out[i], ref, what)
        check(f"(b) {b} {what}", raw, ref)
        rows, rows32 = ref.D(raw, per_row=True), ref.D(ref.r32, per_row=True)
        q = rows / np.maximum(rows32, 1e-300)
        print(f"    per bin, gpu / float32 reference of the same bin: least {q.min():.2f}, median {np.median(q):.2f}, largest {q.max():.2f}")
        bad = np.flatnonzero(rows > FACTOR * rows32.max())
        assert bad.size == 0, (b, what, "bins", (bad + (73 if b == "id73" else 0)).tolist())
        if what == "impulses":
            dead = ref.M.max(0) <= MC.DEAD_MAX
            assert dead.sum() > ref.T // 2 and np.all(raw[:, dead] == np.float32(MC.FLOOR))


# ---- (c) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ["80", "128", "limits"])
def test_c_every_filter_tap(mel, b):
    """201 clips of 1200 samples in one batch, clip k = a cos(2 pi k n / 400): its power sits in bins k - 1, k, k + 1, so every
    tap of every row dominates some element.  `limits`: a 64-tap row from bin 0, an all-zero row, a row with zeros inside
    its span, a row ending at bin 200, MEL_FW_MAX taps in all."""
    lm, F = mel(b)
    clips = [MC.quiet(x, F)[0] for x in MC.tone_clips()]
    d_out = run(lm, clips)
    T = MC.live_frames(1200)
    assert bool((d_out[:, :, T:] == PAD).all())
    raws = MC.out_to_raw(d_out[:, :, :T].cpu().numpy())
    ratios, ds = [], []
    for k, x in enumerate(clips):
        ref = MC.Ref(x, F)
        d = ref.D(raws[k])
        ratios.append(d / ref.D32)
        ds.append((d, ref.D32))
        assert MC.floor_ok(raws[k], ref.M), (b, k)
    k = int(np.argmax(ratios))
    print(f"(c) {b}: 201 tones, D gpu / D float32: median {np.median(ratios):.2f}, largest {ratios[k]:.2f} at tone {k} "
          f"({ds[k][0]:.2e} / {ds[k][1]:.2e}); D gpu {min(d for d, _ in ds):.2e} - {max(d for d, _ in ds):.2e}, "
          f"D float32 {min(d for _, d in ds):.2e} - {max(d for _, d in ds):.2e}")
    for k, (d, d32) in enumerate(ds):
        assert d <= FACTOR * d32, (b, k, d, d32)
    if b == "limits":
        assert np.all(raws[:, 1] == np.float32(MC.FLOOR))


def test_c_table_limits_are_refused_and_the_handle_lives(mel):
    from crispy_amd import _native as N
    from crispy_amd.asr import LogMel
    lm, F = mel("limits")
    x = MC.quiet(MC.tone_clips()[50], F)[0]
    before = lm([x])
    too_long = np.zeros((128, 201), np.float32)
    too_long[5, 20:85] = 0.01                                   # 65 taps
    too_many = F.copy()
    too_many[1, 77] = 0.01                                      # MEL_FW_MAX + 1, no row above 64
    assert MC.bank_taps(too_long) == (65, 65) and MC.bank_taps(too_many) == (MC.MEL_FW_MAX + 1, 64)
    for n_mel, bad in ((128, too_long), (128, too_many), (0, np.zeros((0, 201), np.float32)), (129, np.zeros((129, 201), np.float32))):
        with pytest.raises(N.CrispyError) as e:
            LogMel(n_mel, bad)
        assert e.value.code == ERR_BAD_MODEL, (n_mel, e.value)
    assert np.array_equal(lm([x]).view(np.uint32), before.view(np.uint32))


# ---- (d) ---------------------------------------------------------------------------------------------------------------
def floor_check(what, floor_out, ref):
    """The clamp floor a window shows, ((max - 8) + 4) / 4, against the float64 maximum: FACTOR x D_float32 / w_max + 1/2 ulp"""
    m, t = np.unravel_index(ref.r64.argmax(), ref.r64.shape)
    expect = ((ref.r64[m, t] - 8.0) + 4.0) / 4.0
    tol = FACTOR * ref.D32 / MC.weight(ref.M, ref.Tp)[m, t] + 0.5 * MC.ulp32(expect)
    print(f"{what}: floor {floor_out:.7f}, from the float64 maximum (row {m}, frame {t}) {expect:.7f}, tolerance {tol:.1e}")
    assert abs(float(floor_out) - expect) <= tol, (what, floor_out, expect, tol)


@pytest.mark.parametrize("hz", [200.0, 7000.0])
@pytest.mark.parametrize("b", ["80", "128"])
def test_d_clip_maximum_from_every_position(mel, b, hz):
    """A 5 ms tone two decades above a clip at -40 dB, centred on frame 0, 3, 15, 63, 64 and at the clip's end (70 live frames): the
    maximum comes from lane -> wave -> atomicMax, and the clamp floor of the padding shows which value arrived.  200 Hz lands
    in a low row, 7 kHz in a row >= 64 (the second trip of m += 64: lanes 0-15 only with 80 mels).  One batch, a different
    position per clip, and each clip alone."""
    import torch
    lm, F = mel(b)
    clips = [MC.burst_clip(w, hz)[0] for w in MC.BURST_FRAMES]
    d_out = run(lm, clips)
    for i, w in enumerate(MC.BURST_FRAMES):
        ref = MC.Ref(clips[i], F)
        assert float(d_out[i][:, 2990:].max()) == float(d_out[i].min())       # the padding sits on the floor
        floor_check(f"(d) {b} mels, {hz:g} Hz, {w}", float(d_out[i].min()), ref)
        solo = run(lm, [clips[i]])
        assert torch.equal(solo[0].view(torch.int32), d_out[i].view(torch.int32)), w


@pytest.mark.parametrize("b", ["80", "128"])
def test_d_negative_maximum_through_the_long_path(mel, b):
    """Every raw value negative, the maximum between -2 and 0: float_order_key's negative branch, and the long path's
    clip_max that starts from the key of -10.  The floor, max - 8, is above -10 and shows in the padding."""
    import torch
    lm, F = mel(b)
    x = np.ldexp(MC.quiet(MC.edge_clip(40123), F)[0], 2).astype(np.float32)
    ref = MC.Ref(x, F)
    assert -2.0 < ref.r64.max() < -0.5
    d_pcm = torch.from_numpy(x).cuda()
    w = torch.empty(lm.n_mel, 3000, device="cuda")
    torch.cuda.synchronize()
    lm.compute_long_device(d_pcm.data_ptr(), x.size, np.array([x.size], np.int32))
    lm.window_device([0], [0], d_out=w.data_ptr())
    lm.synchronize()
    assert float(w[:, 2000:].max()) == float(w.min())
    floor_check(f"(d) {b} mels, negative maximum, long path", float(w.min()), ref)


# ---- (e) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", ["80", "128"])
def test_e_loud_clips_through_the_clamp(mel, b):
    """(a)'s clips at their own level, x_loud = x_quiet 2^-k exactly, so every filter sum is the quiet one times 4^-k exactly and
    raw_loud = raw_quiet - 2 k log10(2) within 1/2 ulp(raw_quiet) + 1/2 ulp(raw_loud) + 2e-12 -- the exponent path of
    log10_to_float.  A sum on the floor at either level is -10 or whatever lies between.  The output is that through
    max(., maximum - 8) and (x + 4) / 4, rounded once: an interval for every element, nothing measured."""
    lm, F = mel(b)
    clips, ks, _ = quiet_edge_clips(b, F)
    loud = [np.ldexp(x, -k).astype(np.float32) for x, k in zip(clips, ks)]
    out_q, out_l = run(lm, clips).cpu().numpy(), run(lm, loud).cpu().numpy()
    for i, (n, k) in enumerate(zip(MC.LENGTHS, ks)):
        assert np.array_equal(loud[i], MC.edge_clip(n))
        raw_q = MC.out_to_raw(out_q[i]).astype(np.float64)
        s = -2.0 * k * np.log10(2.0)
        e = raw_q + s
        ulp_e = np.maximum(MC.ulp32(e), MC.ulp32(e * (1.0 + 2.0 ** -20)))       # the larger one next to a binade's edge
        tol = 0.5 * MC.ulp32(raw_q) + 0.5 * ulp_e + 2e-12
        on_floor = raw_q == MC.FLOOR                                             # sum <= 1e-10 when quiet: <= 4^-k 1e-10 when loud
        top = MC.FLOOR + max(s, 0.0)
        lo = np.where(on_floor, MC.FLOOR, np.maximum(MC.FLOOR, e - tol))
        hi = np.where(on_floor, top + 0.5 * MC.ulp32(top) + 2e-12, np.maximum(MC.FLOOR, e + tol))
        o_lo = (np.maximum(lo, lo.max() - 8.0) + 4.0) / 4.0
        o_hi = (np.maximum(hi, hi.max() - 8.0) + 4.0) / 4.0
        got = out_l[i].astype(np.float64)
        ok = (got >= o_lo - 0.5 * MC.ulp32(o_lo)) & (got <= o_hi + 0.5 * MC.ulp32(o_hi))
        width = float((o_hi - o_lo)[~on_floor].max())
        print(f"(e) {b} mels, {n} samples: 2^{-k}, maximum {lo.max():.3f}, {int(on_floor[:, :MC.live_frames(n)].sum())} live-frame elements "
              f"on the quiet floor, widest interval elsewhere {width:.1e}")
        assert ok.all(), (b, n, int((~ok).sum()), np.argwhere(~ok)[:4].tolist())


# ---- (f) ---------------------------------------------------------------------------------------------------------------
def test_f_log10_to_float_against_float64(mel):
    """About 6 10^6 doubles through crispy_mel_stage_log10_device, which runs the frame kernel's own function: 2^16 mantissas in
    every binade from 2^-34 to 2^40, the m > sqrt(2) switch in every binade, every power of two with its neighbours, both
    sides of the floor at 1e-10, 10^6 log-uniform values, 10^5 within 2^-10 of 1.0 -- against numpy's float64 log10."""
    import torch
    from crispy_amd import _native as N
    lm, _ = mel("80")
    s, near1 = MC.log10_inputs()
    d_s = torch.from_numpy(np.concatenate([s, near1])).cuda()
    d_y = torch.full((d_s.numel(),), float("nan"), device="cuda")
    torch.cuda.synchronize()
    lm.stage_log10_device(d_s.data_ptr(), d_y.data_ptr(), d_s.numel())
    lm.synchronize()
    y_all = d_y.cpu().numpy()
    y, y1 = y_all[:s.size], y_all[s.size:]
    floor = s <= 1e-10
    assert floor.sum() > 40000 and np.all(y[floor] == np.float32(MC.FLOOR))      # most of the binade of 2^-34, and 1e-10's neighbours
    assert np.all(np.diff(y) >= 0), "not monotone: the clip maximum relies on order"
    sv, yv = s[~floor], y[~floor].astype(np.float64)
    ref = np.log10(sv)
    err = np.abs(yv - ref)
    worst = float((err - 0.5 * MC.ulp32(ref)).max())
    print(f"(f) {sv.size} values: largest |y - log10 s| - 1/2 ulp {worst:.2e}")
    assert np.all(err <= 0.5 * MC.ulp32(ref) + 1e-12)
    ref1 = np.log10(near1)
    u1 = float((np.abs(y1.astype(np.float64) - ref1) / MC.ulp32(ref1)).max())
    print(f"(f) within 2^-10 of 1.0: largest error {u1:.3f} ulp of the value")
    assert u1 <= 2.0
    # results that are not the correctly rounded float, away from ties the float64 reference cannot decide
    cr = ref.astype(np.float32)
    mid = np.stack([(cr.astype(np.float64) + np.nextafter(cr, np.float32(o)).astype(np.float64)) / 2 for o in (-np.inf, np.inf)])
    decided = np.abs(ref[None, :] - mid).min(0) > 4.0 * np.spacing(np.abs(ref))
    wrong = (y[~floor] != cr) & decided
    rate = wrong.sum() / decided.sum()
    print(f"(f) not the correctly rounded float: {int(wrong.sum())} of {int(decided.sum())} = {rate:.2e} ({int((~decided).sum())} undecided ties left out)")
    assert rate <= 1e-4
    # the entry's own checks
    assert y_all.size == s.size + near1.size and not np.isnan(y_all).any()
    lm.stage_log10_device(0, 0, 0)
    for args in ((0, d_y.data_ptr(), 4), (d_s.data_ptr(), 0, 4)):
        with pytest.raises(N.CrispyError) as e:
            lm.stage_log10_device(*args)
        assert e.value.code == ERR_INVALID_ARG

"""CPU tests of the resampler oracle (oracle/resample_oracle.py): rubato FftFixedIn-style FFT resampler."""
import numpy as np


def test_unity_gain_delay_and_alias_rejection():
    from oracle import resample_oracle as R
    n = 48000
    t = np.arange(n) / 48000.0
    y = R.resample_48k_to_16k(np.sin(2 * np.pi * 1000 * t).astype(np.float32))
    assert y.size == (-(-n // 1024) * 1024) // 1026 * 342
    tt = np.arange(2000, 6000) / 16000.0
    A = np.stack([np.sin(2 * np.pi * 1000 * tt), np.cos(2 * np.pi * 1000 * tt)], 1)
    c, *_ = np.linalg.lstsq(A, y[2000:6000], rcond=None)
    assert abs(np.hypot(*c) - 1.0) < 1e-4                      # unity pass-band gain
    delay = (-np.arctan2(c[1], c[0]) / (2 * np.pi * 1000) * 16000) % 16
    assert abs(delay - (171 % 16)) < 0.05                       # group delay = 513 input = 171 output samples
    y2 = R.resample_48k_to_16k(np.sin(2 * np.pi * 10000 * t).astype(np.float32))
    assert np.sqrt((y2[2000:6000] ** 2).mean()) < 1e-3           # 10 kHz is above the new Nyquist


def test_fft_block_equals_circulant_operator():
    """The GPU applies each block as a GEMM with g[(3n - j) mod 2052]; same operator as the FFT route."""
    from oracle import resample_oracle as R
    F = R.filter_spectrum()
    g = R.operator_g()
    assert g.shape == (2052,) and g.dtype == np.float64
    blk = np.random.default_rng(0).standard_normal(1026)
    M = g[(3 * np.arange(684)[:, None] - np.arange(1026)[None, :]) % 2052]
    buf = np.zeros(2052)
    buf[:1026] = blk
    o = np.zeros(343, complex)
    o[:342] = (np.fft.rfft(buf) * F)[:342]
    assert np.abs(M @ blk - np.fft.irfft(o, 684) * 684).max() < 1e-12


def test_wav_s16_roundtrip_matches_reference_writer_tests():
    """recording.rs:483-504: clamp then x32767 truncated toward zero."""
    from oracle import resample_oracle as R
    x = np.array([0.0, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 1e-5], np.float32)
    q = (R.wav_s16_roundtrip(x) * 32768).astype(np.int32)
    assert q.tolist() == [0, 32767, -32767, 32767, -32767, 16383, -16383, 0]


def test_time_domain_polyphase_derivation_agrees_with_the_fft_route():
    """Independent second derivation of the operator (VERDICT r1 #2e).  The FFT route -- zero-pad a 1026-sample
    block to 2052, multiply by the filter's spectrum, keep 342 bins, inverse FFT of 684, overlap-add -- is a linear
    convolution with the 1026-tap BlackmanHarris^2-windowed sinc followed by an ideal (circular) band limit and
    decimation by 3.  Derived again in the time domain, with no FFT and no blocks: y[n] = sum_j h[3n - j] x[j] over the
    whole zero-padded signal, i.e. a direct-form FIR decimator.  The two differ only by what aliases in the FIR route
    and is cut off in the FFT route.  For input below the transition band (faded tones under 7 kHz) that is only the
    broadband edge transient each 1026-sample block acquires by being cut out of the signal: the FFT route band-limits
    every block on its own before the overlap-add, the FIR route sums the blocks first (where the edges cancel) --
    measured 2-5e-5 of the signal, largest exactly at block boundaries (n = 342 k).  Agreement at 1e-4 therefore pins the
    block alignment, the overlap-add, the gain (1/2052 x 684 x 3 = 1) and the group delay of the restatement.  For
    white noise the difference is the filter's transition band around 8 kHz (cutoff 7.89 kHz, keep-band edge 8 kHz),
    a few 1e-4 of the signal."""
    from oracle import resample_oracle as R
    rng = np.random.default_rng(4)
    n = 48000 + 777                                   # not a multiple of 1024: exercises the zero-padded last chunk
    t = np.arange(n) / 48000.0
    x = (0.4 * np.sin(2 * np.pi * 700.0 * t) + 0.2 * np.sin(2 * np.pi * 3100.0 * t + 1.0)
         + 0.1 * np.sin(2 * np.pi * 6900.0 * t + 2.0))
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.minimum(1.0, np.minimum(np.arange(n), n - 1 - np.arange(n)) / 4800.0))
    x = (x * ramp).astype(np.float32)                # 100 ms fades: an abrupt edge is broadband, not "below 7 kHz"
    y_fft = R.resample_48k_to_16k(x).astype(np.float64)
    # the filter, restated from its definition (not through filter_spectrum())
    cutoff = (0.4 ** (16.0 / 1026)) * 342 / 1026
    k = np.arange(1026) - 513
    arg = np.arange(1026) / 1026.0
    bh = 0.35875 - 0.48829 * np.cos(2 * np.pi * arg) + 0.14128 * np.cos(4 * np.pi * arg) - 0.01168 * np.cos(6 * np.pi * arg)
    h = bh * bh * np.sinc(k * cutoff)
    h /= h.sum()
    n_pad = -(-n // 1024) * 1024
    xp = np.zeros(n_pad)
    xp[:n] = x
    n_out = (n_pad // 1026) * 342
    full = np.convolve(xp[:(n_pad // 1026) * 1026], h)            # only whole 1026-blocks are ever transformed
    y_td = full[::3][:n_out]
    assert y_fft.size == n_out == R.resample_48k_to_16k(x).size
    e = np.abs(y_fft - y_td)
    assert e.max() < 1e-4 * np.abs(y_td).max(), e.max()
    assert int(e.argmax()) % 342 in (0, 1, 341)                   # ... and the residual is the block-edge effect
    # white noise: the transition-band energy the FIR route aliases and the FFT route removes
    w = rng.standard_normal(1026 * 8).astype(np.float32)
    a = R.resample_48k_to_16k(w).astype(np.float64)
    b = np.convolve(w.astype(np.float64), h)[::3][:a.size]
    rel = np.abs(a - b).max() / np.abs(b).max()
    assert 1e-6 < rel < 1e-2, rel


def test_out_len_formula_matches_the_chunk_loop():
    """crispy_resampler_out_len: floor(ceil(n / 1024) * 1024 / 1026) * 342 -- what the reference's loop of 1024-sample
    process() calls (last one zero-padded, commands/transcription.rs:314-357) hands to the chunker when FftFixedIn
    buffers its input in 1026-sample FFT blocks [UPSTREAM-RECALL rubato 0.16.2 synchro.rs: input_buffers + saved_frames]."""
    from crispy_amd import _native as N
    from oracle import resample_oracle as R
    for n in (1, 1023, 1024, 1025, 1026, 2052, 48000, 1_440_000, 1_440_000 + 5):
        want = (-(-n // 1024) * 1024) // 1026 * 342
        assert N.lib().crispy_resampler_out_len(n) == want
        if n <= 48000:
            assert R.resample_48k_to_16k(np.zeros(n, np.float32)).size == want


def test_operator_g_columns_are_the_fft_routes_impulse_responses():
    """operator_g against the FFT route at 1e-12, coefficient by coefficient: column j of the circulant is what the FFT
    route makes of a unit impulse at j -- first, last and middle columns, and through the whole chunk loop (own-block rows,
    overlap rows, the never-flushed tail) as tests/resample_cases.py builds its impulse expectations."""
    from oracle import resample_oracle as R
    from tests import resample_cases as RC
    g = R.operator_g()
    F = R.filter_spectrum()
    for j in (0, 1, 341, 342, 512, 513, 1023, 1025):
        buf = np.zeros(2052)
        buf[j] = 1.0
        o = np.zeros(343, complex)
        o[:342] = (np.fft.rfft(buf) * F)[:342]
        assert np.abs(g[(3 * np.arange(684) - j) % 2052] - np.fft.irfft(o, 684) * 684).max() < 1e-12, j
    for pos in RC.IMPULSE_POS:
        x = np.zeros(RC.IMPULSE_N_IN)
        x[pos] = 1.0
        assert np.abs(RC.impulse_expected(pos) - R.resample_48k_to_16k_f64(x)).max() < 1e-12, pos
    # what the one absolute bar of the other oracle comparisons cannot see (the figures the edge tests were written for)
    assert abs(np.abs(g).max() - 0.3285) < 1e-4 and 0.15 < (np.abs(g) < 1e-5).mean() < 0.18
    assert 0.75 < (np.abs(g) < 2.0 ** -14).mean() < 0.80


def test_float64_path_rounds_to_the_float32_output_bit_for_bit():
    """resample_48k_to_16k_f64 is resample_48k_to_16k before its rounding.  The loop below is the float32 function as it
    stood before the float64 path existed, restated, so that the default return cannot drift."""
    from oracle import resample_oracle as R

    def before(x):
        x = np.asarray(x, dtype=np.float64)
        n_pad = -(-x.size // 1024) * 1024
        xp = np.zeros(n_pad)
        xp[:x.size] = x
        n_blk = n_pad // 1026
        F = R.filter_spectrum()
        out = np.zeros(n_blk * 342)
        overlap = np.zeros(342)
        for b in range(n_blk):
            buf = np.zeros(2052)
            buf[:1026] = xp[b * 1026:(b + 1) * 1026]
            o = np.zeros(343, dtype=complex)
            o[:342] = (np.fft.rfft(buf) * F)[:342]
            y = np.fft.irfft(o, 684) * 684
            out[b * 342:(b + 1) * 342] = y[:342] + overlap
            overlap = y[342:]
        return out.astype(np.float32)

    rng = np.random.default_rng(8)
    for n in (1, 1025, 4096, 48000 + 777):
        x = (0.3 * rng.standard_normal(n)).astype(np.float32)
        y32, y64 = R.resample_48k_to_16k(x), R.resample_48k_to_16k_f64(x)
        assert y32.dtype == np.float32 and y64.dtype == np.float64 and y32.shape == y64.shape
        assert y32.tobytes() == before(x).tobytes() == y64.astype(np.float32).tobytes(), n


def test_wav_s16_roundtrip_reads_a_nan_as_zero():
    """recording.rs:109-110: `(x.clamp(-1.0, 1.0) * 32767.0) as i16` -- f32::clamp keeps a NaN, `as i16` makes it 0."""
    from oracle import resample_oracle as R
    x = np.array([np.nan, 0.25, -np.nan, np.inf, -np.inf, -0.0], np.float32)
    with np.errstate(all="raise"):                 # no undefined NaN -> int16 cast on the way
        y = R.wav_s16_roundtrip(x)
    assert y.dtype == np.float32
    assert (y * 32768).astype(np.int32).tolist() == [0, 8191, 0, 32767, -32767, 0]


def test_edge_case_builder_keeps_its_own_conditions():
    """tests/resample_cases.py: the row counts of the table, impulse positions in range, no dense case near zero, the
    quiet reference above 1e-5, every form on the output stride that selects it."""
    from tests import resample_cases as RC
    assert [(n, b, RC.pair_rows(b, n)) for n, b, _ in RC.ROW_TABLE] == list(RC.ROW_TABLE)
    assert [(c.n_in, c.batch, c.rows) for c in RC.case_set("rows")] == list(RC.ROW_TABLE)
    assert sorted(m for _, _, m in RC.ROW_TABLE) == [1, 127, 129, 387, 512, 1023, 1025, 1025, 1539]
    assert 1539 == 8 * 192 + 3 == 6 * 256 + 3
    assert all(0 <= p < RC.IMPULSE_N_IN for p in RC.IMPULSE_POS) and len(set(RC.IMPULSE_POS)) == 15
    assert RC.out_len(RC.IMPULSE_N_IN) == 1026
    imp = {c.name: c for c in RC.case_set("impulse")}
    assert imp["impulse_hd_pair"].rows == 59 and imp["impulse_hd2_pair"].rows >= RC.HD2_FROM_ROWS
    for c in imp.values():
        assert c.bar == 2.0 ** -24 and c.out_stride % 2 == (c.form == "f32")
        never = [i for i in range(c.batch) if RC.IMPULSE_POS[i % 15] >= 3078]
        assert list(c.exact_zero) == never and len(never) == 2 * c.batch // 15
        assert all(np.all(c.want[i] == 0.0) for i in never)
        for i in range(c.batch):
            p = RC.IMPULSE_POS[i % 15]
            if p + 513 < 3078:                     # group delay 513: the main lobe is in the output (0.27 between two output samples)
                assert np.abs(c.want[i]).max() > 0.25, p
            elif p < 3078:                         # only the tail in front of the lobe: the small coefficients alone
                assert 0.0 < np.abs(c.want[i]).max() < 1e-3, p
    names = set()
    for name in RC.SETS:
        for c in RC.case_set(name):
            names.add(c.name)
            assert (c.out_stride % 2 == 0) == (c.form == "pair"), c.name
            if c.dense:
                assert c.out_len > 0 and np.nanmax(np.abs(c.want), axis=1).min() > 0.05, c.name
            if name != "handoff":
                assert np.all(np.isfinite(c.x[:, :c.n_in])) and np.all(np.isfinite(c.want)), c.name
    assert len(names) == sum(len(RC.case_set(n)) for n in RC.SETS if n != "tile")                 # one name, one case
    assert {c.name for c in RC.case_set("tile")} <= names
    assert all(c.form == "pair" and (c.rows >= RC.HD2_FROM_ROWS or c.n_in == 4096) for c in RC.case_set("tile"))
    for c in RC.case_set("lengths"):
        assert c.x.shape == (3, c.n_in + 37) and np.all(np.isnan(c.x[:, c.n_in:])) and c.out_pad == (2 if c.form == "pair" else 3)
        assert (c.out_len == 0) == (c.n_in <= 1024)
    v = RC.crafted_values()
    assert np.isinf(v).sum() == 2 and (v == 0).sum() == 2 and np.signbit(v[v == 0]).sum() == 1 and not np.isnan(v).any()
    q = {c.name: c for c in RC.case_set("quiet")}
    assert np.abs(q["quiet_lsb_pair"].want).max() > 1e-5
    x = q["quiet_lsb_pair"].x
    assert set(np.unique(x * 32768).tolist()) == {-1.0, 0.0, 1.0}
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)                             # exact subnormal halves
    for name in ("nan_m0_pair", "nan_m1_f32"):
        c = {k.name: k for k in RC.case_set("handoff")}[name]
        assert np.isnan(c.x).sum() == 1 and np.isnan(c.want).sum() == 684 and np.all(np.isnan(c.want[1, 342:1026]))
    assert not np.isnan({k.name: k for k in RC.case_set("handoff")}["nan_m2_pair"].want).any()

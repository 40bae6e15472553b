"""GPU tests of the Parakeet encoder with attention mode 1 (crispy_pk_set_attention_precision: f16 operands and f32 sums in the
attention's three products) through crispy_pk_encode, alone and together with precision mode 1 of the GEMMs, against
tests/pk_attn_f16_oracle.py.  The kernel itself is held at its edges in tests/test_gpu_parakeet_attn_f16_stage.py.

As in tests/test_gpu_parakeet_f16.py the numerics test stops at the tap of block 0 (bound over the whole ragged call, gap to the
same GEMM mode with attention mode 0 per clip); the deeper tensors are a wiring test."""
import numpy as np
import pytest

from tests import pk_attn_f16_oracle as AO
from tests import pk_f16_oracle as FO
from tests import pk_oracle as PO
from tests.test_gpu_parakeet_f16 import FACTOR, GAP, ROWS, bits, check_wiring, per_clip, rms

pytestmark = pytest.mark.gpu

GEMM_MODES = (1, 0)
# The ragged call: the six clips of tests/test_gpu_parakeet_f16.py, then the clips that stand in for them in the gap (rows, seed):
# six for GEMM mode 0, then six for GEMM mode 1.
EXTRA = ((9, 709), (13, 713), (15, 715), (17, 517), (19, 719), (29, 729),
         (16, 3486), (14, 3194), (14, 3534), (12, 3302), (10, 3550), (10, 3600))
ALL_ROWS = ROWS + tuple(r for r, _s in EXTRA)
# The clips (indices into the call) on which the gap is asserted, per GEMM mode: those that reach 8 on the reference alone
# (`gap / yardstick` of every clip is printed by test_numerics_of_block_0 and can be recomputed from the oracles).
#
# The gap is the float64 oracle's distance from the same GEMM mode with attention mode 0: 9e-5 at one frame, 3e-5 ... 9e-5 at 2 ... 5
# frames, then falling as 1 / sqrt(keys) (1.8e-5 at 10 frames, 1.1e-5 at 33, 8e-6 at 65).  The yardstick is the float32 oracle's
# distance to the float64 one: 1e-7 ... 4e-7 for a clip none of whose f16 operands sits on a tie within an f32 ulp, 1e-6 ... 8e-5 for
# a clip with such a flip (docstring of tests/test_gpu_parakeet_f16.py).  Which clips have one depends on the host's float32 BLAS
# and libm, so the stand-ins are clips whose yardstick is at the flip-free level with a margin of 40 x or more over the factor.
#   GEMM mode 0: rows 1 stays (gap / yardstick about 400 ... 500).  Replaced: rows 257 (7.7) and 513 (4.5), which cannot reach 8 at
#     their length, and rows 9, 33 and 73 (10 ... 180, 15 ... 17, 6 ... 12), whose margin is a flip or less.
#   GEMM mode 1: all six are replaced.  Rows 1: the gap is 0 (one key gives f16(v), which o_proj rounds to f16 anyway).  Rows 33 ... 513
#     (1.0 ... 1.8): with f16 GEMM operands every row of a clip of 5 frames or more holds a flip, and the yardstick, 2e-5 ... 3e-5,
#     is the size of the gap.  Rows 9 seed 109 (1.3 ... 160) has one on some hosts.  Of clips of two frames about four in ten are
#     flip-free (ratio 300 ... 800); six of those stand in (400 ... 830).
GAP_CLIPS = {1: (12, 13, 14, 15, 16, 17), 0: (0, 6, 7, 8, 9, 10, 11)}


@pytest.fixture(scope="module")
def weights():
    return PO.make_weights(PO.TINY, 1)


@pytest.fixture(scope="module")
def clips():
    return [PO.clip(r, 128, 100 + r) for r in ROWS] + [PO.clip(r, 128, s) for r, s in EXTRA]


@pytest.fixture(scope="module")
def key_tile():
    from crispy_amd import _native as N
    return N.PK_ATTN_KEY_TILE


@pytest.fixture(scope="module")
def refs(weights, clips, key_tile):
    """per GEMM mode: (float64 oracle of the combination, its float32 form, the float64 oracle of the same GEMM mode with attention
    mode 0); shared, unchanged"""
    import torch
    out = {}
    for gemm in GEMM_MODES:
        att = lambda dtype: AO.Encoder(PO.TINY, weights, dtype, key_tile, attention=True, gemm=bool(gemm)).forward(clips)
        out[gemm] = (att(torch.float64), att(torch.float32), FO.Encoder(PO.TINY, weights, torch.float64, hooks=bool(gemm)).forward(clips))
    return out


@pytest.fixture(scope="module")
def enc(weights):
    from crispy_amd import ParakeetEncoder
    e = ParakeetEncoder(0)
    e.load(PO.TINY.as_dict(), weights)
    assert e.attention_precision == 0 and e.precision == 0
    yield e
    e.close()


@pytest.fixture(scope="module")
def gpu(enc, clips):
    """attention mode 1's (frames, subsampling, tap, position table) of all clips in one ragged call, per GEMM mode and tap layer;
    the handle is left in (0, 0)"""
    out = {}
    enc.set_attention_precision(1)
    for gemm in GEMM_MODES:
        enc.set_precision(gemm)
        assert enc.precision == gemm and enc.attention_precision == 1      # neither switch moves the other
        out[gemm] = {layer: enc.encode(clips, taps=True, tap_layer=layer) for layer in (0, 1, 2)}
    enc.set_precision(0)
    enc.set_attention_precision(0)
    assert enc.precision == 0 and enc.attention_precision == 0
    return out


@pytest.mark.parametrize("gemm", GEMM_MODES, ids=["gemm1", "gemm0"])
def test_numerics_of_block_0(gpu, refs, gemm):
    """the tap of block 0: the device's rms distance to the float64 oracle of the combination is within 4 x the float32 oracle's own
    over the whole call, and per clip the combination's distance from the same GEMM mode with attention mode 0 is at least 8 x that
    yardstick"""
    r64, r32, base = refs[gemm]
    sq_yard = sq_err = n = 0.0
    for c, rows in enumerate(ALL_ROWS):
        g, a, b, x = gpu[gemm][0][2][c], r64[c][2][0], r32[c][2][0], base[c][2][0]
        assert g.shape == a.shape and np.isfinite(g).all()
        yard, err, gap = rms(b.astype(np.float64) - a), rms(g.astype(np.float64) - a), rms(a - x)
        print(f"pk attn f16 gemm mode {gemm} rows {rows} tap0: float32 oracle {yard:.3e}, GPU {err:.3e}, gap to attention mode 0 {gap:.3e} "
              f"(ratio {err / yard:.2f}, gap / yardstick {gap / yard:.1f})")
        if c in GAP_CLIPS[gemm]:
            assert gap >= GAP * yard, (rows, gap, yard)
            # ... so attention mode 0's result is outside the bound: the device's distance from that oracle must be, too
            assert rms(g.astype(np.float64) - x) > FACTOR * yard, (rows, "the device is within the bound of attention mode 0's oracle")
        sq_yard, sq_err, n = sq_yard + yard * yard * a.size, sq_err + err * err * a.size, n + a.size
    yard, err = float(np.sqrt(sq_yard / n)), float(np.sqrt(sq_err / n))
    print(f"pk attn f16 gemm mode {gemm} whole call tap0: float32 oracle {yard:.3e}, GPU {err:.3e} (ratio {err / yard:.2f}, bound {FACTOR:g})")
    assert err <= FACTOR * yard


@pytest.mark.parametrize("gemm", GEMM_MODES, ids=["gemm1", "gemm0"])
@pytest.mark.parametrize("c", range(len(ROWS)))
def test_wiring_of_the_deeper_blocks(gpu, refs, gemm, c):
    """frames and the taps of blocks 1 and 2 within 4 x the float32 oracle's distance to the float64 one, max and rms"""
    r64, r32, _base = refs[gemm]
    for layer in (1, 2):
        check_wiring(per_clip(gpu[gemm][layer], c), r64[c], r32[c], layer, f"attn f16 gemm mode {gemm} rows {ROWS[c]} tap {layer}")


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for pa, pb in zip(a[:3], b[:3]) for x, y in zip(pa, pb))


def test_switching_back_before_the_load_and_across_a_reload(weights, clips, gpu, enc):
    from crispy_amd import ParakeetEncoder
    for gemm in GEMM_MODES:
        never, back = ParakeetEncoder(0), ParakeetEncoder(0)
        try:
            never.load(PO.TINY.as_dict(), weights)
            never.set_precision(gemm)
            back.set_attention_precision(1)      # before the load
            back.set_precision(gemm)
            back.load(PO.TINY.as_dict(), weights)
            assert back.attention_precision == 1 and back.precision == gemm and never.attention_precision == 0
            one = back.encode(clips, taps=True, tap_layer=0)
            assert same(one, gpu[gemm][0])      # set before the load or after it: the same bytes
            back.load(PO.TINY.as_dict(), weights)
            assert back.attention_precision == 1 and back.precision == gemm      # both survive a reload
            assert same(back.encode(clips, taps=True, tap_layer=0), one)
            back.set_attention_precision(0)
            assert back.attention_precision == 0 and back.precision == gemm
            a, b = never.encode(clips, taps=True, tap_layer=0), back.encode(clips, taps=True, tap_layer=0)
            assert same(a, b)      # mode 1 then 0: the bytes of a handle that never saw the call
            for c in range(len(ALL_ROWS)):
                if not (gemm == 1 and ALL_ROWS[c] == 1):      # one key under f16 GEMMs: f16(v) is rounded again by o_proj, the same bytes
                    assert not np.array_equal(bits(a[0][c]), bits(one[0][c]))
        finally:
            never.close()
            back.close()


def test_transcribe_with_both_switches_equals_the_three_stages(weights):
    from crispy_amd import Parakeet
    from tests import pk_mel_oracle as MO
    from tests import pk_tdt_oracle as TO
    state = {"encoder." + k: v for k, v in weights.items()}
    state.update(TO.make_tdt_weights(TO.TINY_TDT, 3))
    pcm = [MO.speechlike(16000, 81), MO.noise(4003, 82), MO.speechlike(9100, 83)]
    pk = Parakeet(0)
    try:
        pk.load(PO.TINY.as_dict(), TO.TINY_TDT.as_dict(), state)
        feats = pk.encoder.features(pcm)
        pk.set_precision(1)
        frames_gemm = pk.encoder.encode(feats)
        pk.set_attention_precision(1)
        assert pk.encoder.attention_precision == 1 and pk.encoder.precision == 1
        frames = pk.encoder.encode(feats)
        assert any(not np.array_equal(bits(a), bits(b)) for a, b in zip(frames_gemm, frames))
        want = pk.decoder.decode(frames)
        got = pk.transcribe(pcm)
        for g, w in zip(got, want):
            assert np.array_equal(g["steps"], w)
        assert sum(len(g["steps"]) for g in got) > 0
    finally:
        pk.close()


def test_catalog_widths_one_block(key_tile):
    """H 1024, 8 heads: one block at the catalog widths with both switches at 1, clips of 300 and 9 rows"""
    import torch
    from crispy_amd import ParakeetEncoder
    cfg = PO.with_flags(PO.CATALOG_V3, layers=1)
    w = PO.make_weights(cfg, 3)
    clips = [PO.clip(300, 128, 31), PO.clip(9, 128, 32)]
    e = ParakeetEncoder(0)
    try:
        e.load(cfg.as_dict(), w)
        e.set_precision(1)
        e.set_attention_precision(1)
        got = e.encode(clips, taps=True, tap_layer=0)
    finally:
        e.close()
    r64 = AO.Encoder(cfg, w, torch.float64, key_tile, gemm=True).forward(clips)
    r32 = AO.Encoder(cfg, w, torch.float32, key_tile, gemm=True).forward(clips)
    for c in range(2):
        check_wiring(per_clip(got, c), r64[c], r32[c], 0, f"attn f16 catalog widths rows {clips[c].shape[0]}")


def test_limits(enc):
    from crispy_amd import _native as N
    enc.set_attention_precision(1)
    try:
        for mode in (2, -1):
            with pytest.raises(N.CrispyError, match=f"mode {mode}") as e:
                enc.set_attention_precision(mode)
            assert e.value.code == -1
        assert enc.attention_precision == 1 and enc.precision == 0      # a refused mode changes nothing
    finally:
        enc.set_attention_precision(0)

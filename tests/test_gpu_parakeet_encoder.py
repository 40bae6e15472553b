"""GPU tests of the Parakeet FastConformer encoder (crispy_pk_*, include/crispy_hip.h) against tests/pk_oracle.py: the frames, the
subsampling output and block taps on ragged clips over every edge of the attention tiles and of the depthwise kernel, the
position table bit for bit, neighbours 1e4 times larger, batch, position and call independence byte for byte, the flags at 0 and
80 mel bins, one block at the catalog widths, silent and constant clips, the limits, a reload, and the host form.

The bound (the rule of tests/test_gpu_diar_emb.py): per clip and per tensor, the GPU's largest distance to float64 stays within
4 x the float32 oracle's.  Both are f32 arithmetic on the same operands; a different but equally valid summation order lands
within a small multiple of another implementation's error."""
import numpy as np
import pytest

from tests import pk_oracle as PO

pytestmark = pytest.mark.gpu

FACTOR = 4.0
# rows -> T' {1, 1, 2, 2, 3, 4, 4, 5, 9, 10, 31, 32, 33, 65}: one frame, fewer frames than the depthwise half-kernel (4), exactly the
# kernel (9), one below, on and one above the attention's query and key tile (both 32), and three tiles with a last one of one frame
ROWS = (1, 8, 9, 16, 17, 25, 32, 33, 65, 73, 241, 249, 257, 513)
NAMES = ("frames", "subsampling", "tap")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracles(cfg, weights):
    import torch
    return PO.Encoder(cfg, weights, torch.float64), PO.Encoder(cfg, weights, torch.float32)


@pytest.fixture(scope="module")
def weights():
    return PO.make_weights(PO.TINY, 1)


@pytest.fixture(scope="module")
def tiny_oracles(weights):
    return oracles(PO.TINY, weights)


@pytest.fixture(scope="module")
def enc(weights):
    from crispy_amd import ParakeetEncoder
    e = ParakeetEncoder(0)
    e.load(PO.TINY.as_dict(), weights)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ragged():
    return [PO.clip(r, 128, 100 + r) for r in ROWS]


@pytest.fixture(scope="module")
def ragged_gpu(enc, ragged):
    """(frames, subsampling, tap, position table) of all clips in one ragged call, for the taps at blocks 0 and 2; shared, unchanged"""
    return {layer: enc.encode(ragged, taps=True, tap_layer=layer) for layer in (0, 2)}


@pytest.fixture(scope="module")
def ragged_ref(tiny_oracles, ragged):
    return tiny_oracles[0].forward(ragged), tiny_oracles[1].forward(ragged)


def check(got, r64, r32, tap_layer, what):
    """got = (frames, subsampling, tap) of the GPU on one clip; r64, r32 = the oracles' (out, sub, taps) -> asserts GPU / float32 oracle"""
    rows = []
    for name, g, a, b in zip(NAMES, got, (r64[0], r64[1], r64[2][tap_layer]), (r32[0], r32[1], r32[2][tap_layer])):
        assert g.shape == a.shape, (what, name, g.shape, a.shape)
        assert np.isfinite(g).all(), (what, name)
        yard = float(np.abs(b.astype(np.float64) - a).max())
        err = float(np.abs(g.astype(np.float64) - a).max())
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
        print(f"pk {what} {name}{tap_layer if name == 'tap' else ''}: float32 oracle {yard:.3e}, GPU {err:.3e} from float64 "
              f"(ratio {ratio:.2f}, bound {FACTOR:g})")
        rows.append((name, err, yard))
    for name, err, yard in rows:
        assert err <= FACTOR * yard, (what, name, err, yard)


def per_clip(got, c):
    return got[0][c], got[1][c], got[2][c]


@pytest.mark.parametrize("c", range(len(ROWS)))
def test_ragged_values(enc, ragged_gpu, ragged_ref, c):
    assert enc.loaded and enc.config == PO.TINY.as_dict()
    for layer in (0, 2):
        got = per_clip(ragged_gpu[layer], c)
        assert got[0].shape == (PO.frames(ROWS[c]), 256)
        check(got, ragged_ref[0][c], ragged_ref[1][c], layer, f"rows {ROWS[c]}")
    assert np.array_equal(bits(ragged_gpu[2][2][c]), bits(ragged_gpu[2][0][c]))      # the last block's tap is the output
    assert np.array_equal(bits(ragged_gpu[0][0][c]), bits(ragged_gpu[2][0][c]))


def test_position_table_bit_for_bit(enc, ragged_gpu):
    tmax = max(PO.frames(r) for r in ROWS)
    pos = ragged_gpu[0][3]
    assert pos.shape == (2 * tmax - 1, 256) and np.array_equal(bits(pos), bits(PO.pos_table(tmax, 256)))
    # the longest clip the call takes: d up to +-4999, where a fast sine is wrong
    import torch
    long = torch.zeros((40000, 128), dtype=torch.float32, device="cuda")
    _out, _sub, _tap, pos = enc.encode_device([long], taps=True)
    assert np.array_equal(bits(pos.cpu().numpy()), bits(PO.pos_table(5000, 256)))


def test_neighbours_do_not_reach_a_clip(enc):
    mine = PO.clip(12, 128, 5)      # T' = 2
    assert PO.frames(12) == 2
    loud = [PO.clip(r, 128, 6 + r, scale=1e4) for r in (73, 40)]
    alone = enc.encode([mine], taps=True, tap_layer=0)
    among = enc.encode([loud[0], mine, loud[1]], taps=True, tap_layer=0)
    for a, b in zip(per_clip(alone, 0), per_clip(among, 1)):
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b))


def test_bytes_alone_in_a_batch_and_in_a_second_call(enc, ragged, ragged_gpu):
    for r in (257, 73):
        c = ROWS.index(r)
        mine = ragged[c]
        alone = enc.encode([mine], taps=True, tap_layer=2)
        first = enc.encode([mine, ragged[0], ragged[9]], taps=True, tap_layer=2)
        last = enc.encode(ragged[c + 1:] + ragged[:c + 1], taps=True, tap_layer=2)      # the ragged list rotated: last of 14
        again = enc.encode([ragged[3], mine], taps=True, tap_layer=2)                   # a second call after another batch
        for a, f, l, g, m in zip(per_clip(alone, 0), per_clip(first, 0), per_clip(last, len(ROWS) - 1), per_clip(again, 1),
                                 per_clip(ragged_gpu[2], c)):      # in the middle of the ragged call
            for other in (f, l, g, m):
                assert np.array_equal(bits(a), bits(other))


def test_host_form_equals_device_form(enc, ragged, ragged_gpu):
    import torch
    dev = enc.encode_device([torch.from_numpy(x).cuda() for x in ragged], taps=True, tap_layer=2)
    for part_d, part_h in zip(dev[:3], ragged_gpu[2][:3]):
        for a, b in zip(part_d, part_h):
            assert np.array_equal(bits(a.cpu().numpy()), bits(b))
    assert np.array_equal(bits(dev[3].cpu().numpy()), bits(ragged_gpu[2][3]))
    plain = enc.encode(ragged)
    for a, b in zip(plain, ragged_gpu[2][0]):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("change", [dict(attention_bias=0), dict(convolution_bias=0), dict(scale_input=0), dict(mel_bins=80)],
                         ids=["attention_bias0", "convolution_bias0", "scale_input0", "mel80"])
def test_flags_and_mel_bins(change):
    from crispy_amd import ParakeetEncoder
    cfg = PO.with_flags(PO.TINY, **change)
    w = PO.make_weights(cfg, 2)
    o64, o32 = oracles(cfg, w)
    clips = [PO.clip(r, cfg.mel_bins, 200 + r) for r in (17, 73, 249)]
    e = ParakeetEncoder(0)
    try:
        e.load(cfg.as_dict(), w)
        assert e.config == cfg.as_dict()
        got = e.encode(clips, taps=True, tap_layer=1)
    finally:
        e.close()
    r64, r32 = o64.forward(clips), o32.forward(clips)
    for c in range(len(clips)):
        check(per_clip(got, c), r64[c], r32[c], 1, f"{change} rows {clips[c].shape[0]}")


def test_catalog_widths_one_block():
    """H 1024, 8 heads, ffn 4096, C 256, M 128: the real K-loop lengths and the real [C * 16] flatten"""
    from crispy_amd import ParakeetEncoder
    cfg = PO.with_flags(PO.CATALOG_V3, layers=1)
    w = PO.make_weights(cfg, 3)
    o64, o32 = oracles(cfg, w)
    clips = [PO.clip(300, 128, 31), PO.clip(9, 128, 32)]
    e = ParakeetEncoder(0)
    try:
        e.load(cfg.as_dict(), w)
        got = e.encode(clips, taps=True, tap_layer=0)
    finally:
        e.close()
    r64, r32 = o64.forward(clips), o32.forward(clips)
    for c in range(2):
        check(per_clip(got, c), r64[c], r32[c], 0, f"catalog widths rows {clips[c].shape[0]}")


def test_silent_and_constant_clips(enc, tiny_oracles):
    cases = {"all zeros": np.zeros((40, 128), np.float32),
             "constant over time": np.repeat(np.random.default_rng(7).uniform(-2, 2, (1, 128)).astype(np.float32), 64, 0),
             "constant over time and mel": np.full((33, 128), 0.75, np.float32)}
    got = enc.encode(list(cases.values()), taps=True, tap_layer=1)
    r64, r32 = tiny_oracles[0].forward(list(cases.values())), tiny_oracles[1].forward(list(cases.values()))
    for c, what in enumerate(cases):
        check(per_clip(got, c), r64[c], r32[c], 1, what)


def test_limits_are_refused_before_a_launch(enc):
    from crispy_amd import _native as N
    ok = PO.clip(9, 128, 1)
    for bad, text in (([ok, np.zeros((0, 128), np.float32)], "clip 1 has 0 rows"), ([np.zeros((40001, 128), np.float32)], "40001 rows"),
                      ([], "n_clips 0"), ([np.zeros((1, 128), np.float32)] * 4097, "n_clips 4097")):
        with pytest.raises(N.CrispyError, match=text) as e:
            enc.encode(bad)
        assert e.value.code == -1
    for layer in (-1, 3):
        with pytest.raises(N.CrispyError, match=f"tap_layer {layer}") as e:
            enc.encode([ok], taps=True, tap_layer=layer)
        assert e.value.code == -1
    assert enc.encode([ok])[0].shape == (2, 256)      # the handle still works


def test_encode_before_load_and_reload_at_another_config(weights, tiny_oracles):
    from crispy_amd import ParakeetEncoder
    from crispy_amd import _native as N
    clips = [PO.clip(r, 128, 300 + r) for r in (9, 65)]
    e = ParakeetEncoder(0)
    try:
        assert not e.loaded
        with pytest.raises(N.CrispyError, match="no encoder is loaded") as err:
            e.encode(clips)
        assert err.value.code == -1
        with pytest.raises(N.CrispyError, match="no encoder is loaded"):
            _ = e.config
        e.load(PO.TINY.as_dict(), weights)
        first = e.encode(clips, taps=True, tap_layer=1)
        r64, r32 = tiny_oracles[0].forward(clips), tiny_oracles[1].forward(clips)
        for c in range(2):
            check(per_clip(first, c), r64[c], r32[c], 1, f"first load, clip {c}")
        cfg = PO.Config(hidden=128, layers=2, heads=1, ffn=256, conv_kernel=5, mel_bins=80, sub_channels=64, attention_bias=0)
        w2 = PO.make_weights(cfg, 4)
        e.load(cfg.as_dict(), w2)
        assert e.config == cfg.as_dict()
        clips2 = [PO.clip(r, 80, 400 + r) for r in (9, 65)]
        second = e.encode(clips2, taps=True, tap_layer=1)
        assert second[0][1].shape == (9, 128)
        o64, o32 = oracles(cfg, w2)
        r64, r32 = o64.forward(clips2), o32.forward(clips2)
        for c in range(2):
            check(per_clip(second, c), r64[c], r32[c], 1, f"second load (H 128, K 5, M 80, C 64), clip {c}")
    finally:
        e.close()

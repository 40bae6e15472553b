"""GPU tests of the Parakeet encoder's attention as a stage (crispy_pk_stage_attention_device; no model load), mode 1 (f16 operands, f32
sums, soft-max in key tiles of N.PK_ATTN_KEY_TILE) against tests/pk_attn_f16_oracle.py and mode 0 against the exact attention.

The lengths sit at every edge of a 32- or 64-key tile and of a 32- or 128-query tile.  FACTOR bounds the device's rms distance to
the float64 oracle by the float32 oracle's own over the whole ragged call: single f16 tie flips of a soft-max weight make a
per-clip bound a coin toss on either side.  GAP holds the oracle's own distance from the exact float64 attention per clip, so mode
0's bytes, or a rounding in the wrong place, fail the bound."""
import numpy as np
import pytest
import torch

from tests import pk_attn_f16_oracle as AO

pytestmark = pytest.mark.gpu

FACTOR = 4.0
GAP = 8.0
HEAD = AO.HEAD
LENGTHS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def cut(a, lengths):
    at = np.concatenate([[0], np.cumsum(lengths)])
    return [a[at[c]:at[c + 1]] for c in range(len(lengths))]


def operands(lengths, heads, seed, tmax=None, q_scale=1.0):
    """random normal q | k | v, r, and biases about 0.1: scores of standard deviation about 1.4 x q_scale"""
    tmax = tmax or max(lengths)
    rng = np.random.default_rng(seed)
    H = heads * HEAD
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    qkv = f(sum(lengths), 3 * H)
    qkv[:, :H] *= np.float32(q_scale)
    return qkv, f(2 * tmax - 1, H), 0.1 * f(H), 0.1 * f(H), tmax


def one_hot_v(qkv, lengths, heads):
    """V row j of every clip and head = e_j (clips of at most 128 frames): out[i][j] is the weight of key j"""
    H = heads * HEAD
    at = 0
    for n in lengths:
        assert n <= HEAD
        qkv[at:at + n, 2 * H:] = 0.0
        for h in range(heads):
            qkv[at + np.arange(n), 2 * H + h * HEAD + np.arange(n)] = 1.0
        at += n
    return qkv


@pytest.fixture(scope="module")
def enc():
    from crispy_amd import ParakeetEncoder
    e = ParakeetEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def key_tile():
    from crispy_amd import _native as N
    return N.PK_ATTN_KEY_TILE


@pytest.mark.parametrize("mode", [1, 0])
def test_masks_exactly(enc, mode):
    """q = u = v = r = 0 and V of small integers: every row is the float64 mean of its own clip's V rows rounded to f32, bit for bit,
    for every length 1 ... 130 in one ragged call beside a 257-frame neighbour (tmax > n)"""
    heads = 2
    lengths = list(range(1, 131)) + [257]
    qkv, r, u, v, tmax = operands(lengths, heads, 1)
    H = heads * HEAD
    qkv[:, :H] = 0.0
    qkv[:, 2 * H:] = np.random.default_rng(2).integers(-8, 9, (sum(lengths), H)).astype(np.float32)
    out = enc.stage_attention(mode, qkv, 0 * r, 0 * u, 0 * v, lengths, heads, tmax)
    for n, o, x in zip(lengths, cut(out, lengths), cut(qkv[:, 2 * H:], lengths)):
        want = np.broadcast_to(x.astype(np.float64).mean(0).astype(np.float32), o.shape)
        assert np.array_equal(bits(o), bits(want)), n


@pytest.mark.parametrize("q_scale", [1.0, 4.0], ids=["q1", "q4"])
def test_soft_max_weights_read_through_one_hot_v(enc, key_tile, q_scale):
    """n <= 128 and V rows one-hot: out[i][j] = f16(p_ij) / l_i, against the float64 oracle; at 4 x larger q most weights are f16
    subnormals or zero"""
    heads = 2
    lengths = [n for n in LENGTHS if n <= HEAD]
    qkv, r, u, v, tmax = operands(lengths, heads, 3, q_scale=q_scale)
    qkv = one_hot_v(qkv, lengths, heads)
    out = enc.stage_attention(1, qkv, r, u, v, lengths, heads, tmax)
    o64 = AO.stage(qkv, r, u, v, lengths, heads, tmax, key_tile, torch.float64)
    o32 = AO.stage(qkv, r, u, v, lengths, heads, tmax, key_tile, torch.float32)
    assert np.isfinite(out).all()
    yard, err = rms(o32 - o64), rms(out - o64)
    small = float(np.mean((o64 > 0) & (o64 < 2.0 ** -14)))
    print(f"pk attn f16 one-hot q x {q_scale:g}: float32 oracle {yard:.3e}, GPU {err:.3e} (ratio {err / yard:.2f}); weights below 2^-14: {small:.2f}")
    assert err <= FACTOR * yard
    for n, o in zip(lengths, cut(out, lengths)):      # the columns behind the clip's last key hold no weight
        assert not o.reshape(n, heads, HEAD)[:, :, n:].any(), n


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("extra", [0, 70], ids=["tmax_n", "tmax_n70"])
def test_position_index(enc, mode, extra):
    """k = 0, u = 0 and an R whose row for the distance d0 alone aligns with q + v: read through one-hot V, query i's largest weight
    sits at key i - d0"""
    n, heads = 97, 1
    tmax = n + extra
    rng = np.random.default_rng(5)
    w = rng.standard_normal(HEAD).astype(np.float32)
    vb = (0.1 * rng.standard_normal(HEAD)).astype(np.float32)
    for d0 in (-(n - 1), -33, -32, -31, -1, 0, 1, 31, 32, 33, n - 1):
        qkv = np.zeros((n, 3 * HEAD), np.float32)
        qkv[:, :HEAD] = w - vb      # q + v = w in every query
        qkv = one_hot_v(qkv, [n], heads)
        r = np.zeros((2 * tmax - 1, HEAD), np.float32)
        r[d0 + tmax - 1] = w      # score(i, i - d0) = |w|^2 / sqrt(128), about 11; every other score 0
        out = enc.stage_attention(mode, qkv, r, np.zeros(HEAD, np.float32), vb, [n], heads, tmax)
        for i in range(n):
            if 0 <= i - d0 < n:
                assert int(np.argmax(out[i])) == i - d0 and out[i, i - d0] > 0.9, (d0, i)


@pytest.fixture(scope="module")
def ragged():
    """random operands, one ragged call of all the lengths; the references are shared and unchanged"""
    heads = 2
    qkv, r, u, v, tmax = operands(LENGTHS, heads, 9)
    return dict(heads=heads, args=(qkv, r, u, v), tmax=tmax)


@pytest.fixture(scope="module")
def ragged_refs(ragged, key_tile):
    a = ragged["args"]
    st = lambda dtype, f16: AO.stage(*a, LENGTHS, ragged["heads"], ragged["tmax"], key_tile, dtype, f16)
    return dict(o64=st(torch.float64, True), o32=st(torch.float32, True), x64=st(torch.float64, False), x32=st(torch.float32, False))


@pytest.fixture(scope="module")
def ragged_gpu(enc, ragged):
    return {mode: enc.stage_attention(mode, *ragged["args"], LENGTHS, ragged["heads"], ragged["tmax"]) for mode in (0, 1)}


def test_random_operands_mode_1(ragged, ragged_refs, ragged_gpu):
    out, o64, o32, x64 = ragged_gpu[1], ragged_refs["o64"], ragged_refs["o32"], ragged_refs["x64"]
    assert out.shape == o64.shape and np.isfinite(out).all()
    v = ragged["args"][0][:, 2 * ragged["heads"] * HEAD:]
    for n, g, a, b, x, vc in zip(LENGTHS, cut(out, LENGTHS), cut(o64, LENGTHS), cut(o32, LENGTHS), cut(x64, LENGTHS), cut(v, LENGTHS)):
        yard, err, gap = rms(b - a), rms(g - a), rms(a - x)
        print(f"pk attn f16 stage n {n}: float32 oracle {yard:.3e}, GPU {err:.3e}, gap to the exact attention {gap:.3e} "
              f"(ratio {err / max(yard, 1e-30):.2f}, gap / yardstick {gap / max(yard, 1e-30):.1f})")
        if n == 1:      # one key: the weight is 1, the row is f16(v)
            assert yard == 0.0 and np.array_equal(bits(g), bits(vc.astype(np.float16).astype(np.float32)))
        else:
            assert gap >= GAP * yard, (n, gap, yard)
    yard, err = rms(o32 - o64), rms(out - o64)
    print(f"pk attn f16 stage whole call: float32 oracle {yard:.3e}, GPU {err:.3e} (ratio {err / yard:.2f}, bound {FACTOR:g})")
    assert err <= FACTOR * yard


def test_random_operands_mode_0(ragged_refs, ragged_gpu):
    out, x64, x32 = ragged_gpu[0], ragged_refs["x64"], ragged_refs["x32"]
    yard, err = rms(x32 - x64), rms(out - x64)
    print(f"pk attn stage mode 0 whole call: float32 exact oracle {yard:.3e}, GPU {err:.3e} (ratio {err / yard:.2f}, bound {FACTOR:g})")
    assert np.isfinite(out).all() and err <= FACTOR * yard
    for g0, g1 in zip(cut(out, LENGTHS), cut(ragged_gpu[1], LENGTHS)):
        assert not np.array_equal(bits(g0), bits(g1))


def test_bytes_alone_in_a_batch_rotated_and_in_a_second_call(enc, ragged, ragged_gpu):
    qkv, r, u, v = ragged["args"]
    heads, tmax = ragged["heads"], ragged["tmax"]
    parts, whole = cut(qkv, LENGTHS), cut(ragged_gpu[1], LENGTHS)
    run = lambda idx, t: cut(enc.stage_attention(1, np.concatenate([parts[c] for c in idx], 0), r, u, v, [LENGTHS[c] for c in idx], heads, t), [LENGTHS[c] for c in idx])
    for n in (129, 65, 33):
        c = LENGTHS.index(n)
        alone = run([c], tmax)[0]
        first = run([c, 0, 3], tmax)[0]
        order = list(range(c + 1, len(LENGTHS))) + list(range(c + 1))
        last = run(order, tmax)[-1]
        again = run([1, c], tmax)[1]
        for other in (first, last, again, whole[c]):
            assert np.array_equal(bits(alone), bits(other)), n


def test_neighbours_1e4_times_larger(enc):
    lengths, heads = [40, 70, 33], 2
    qkv, r, u, v, tmax = operands(lengths, heads, 13)
    parts = cut(qkv, lengths)
    alone = enc.stage_attention(1, parts[1], r, u, v, [70], heads, tmax)
    loud = np.concatenate([parts[0] * np.float32(8e4), parts[1], parts[2] * np.float32(8e4)], 0)      # unit-deviation operands x 8e4 (1e4 alone reaches 4.5e4 at most and does not overflow f16)
    among = cut(enc.stage_attention(1, loud, r, u, v, lengths, heads, tmax), lengths)
    assert np.isfinite(alone).all() and np.array_equal(bits(alone), bits(among[1]))
    assert not np.isfinite(among[0]).all() and not np.isfinite(among[2]).all()


def test_limits(enc):
    import ctypes as C
    from crispy_amd import _native as N
    L = N.lib()
    heads, tmax = 1, 8
    dev = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    qkv, r, u, v, out = dev(12, 3 * HEAD), dev(2 * tmax - 1, HEAD), dev(HEAD), dev(HEAD), dev(12, HEAD)
    off = lambda *a: (C.c_long * len(a))(*a)
    torch.cuda.synchronize()
    good = dict(h=enc._h, mode=1, qkv=qkv.data_ptr(), r=r.data_ptr(), u=u.data_ptr(), v=v.data_ptr(), off=off(0, 4, 12), n=2, heads=heads, tmax=tmax,
                out=out.data_ptr())
    call = lambda **kw: (lambda a: L.crispy_pk_stage_attention_device(a["h"], a["mode"], a["qkv"], a["r"], a["u"], a["v"], a["off"], a["n"], a["heads"],
                                                                       a["tmax"], a["out"]))({**good, **kw})
    assert call() == 0
    for kw, word in ((dict(h=None), "NULL handle"), (dict(mode=2), "mode 2"), (dict(mode=-1), "mode -1"), (dict(qkv=None), "d_qkv"), (dict(r=None), "d_r"),
                     (dict(u=None), "d_bias_u"), (dict(v=None), "d_bias_v"), (dict(out=None), "d_out"), (dict(off=None), "frame_offset"),
                     (dict(n=0), "n_clips"), (dict(n=4097), "n_clips"), (dict(heads=0), "heads"), (dict(tmax=7), "clip 1"),
                     (dict(off=off(0, 4, 4)), "clip 1"), (dict(off=off(0, 0, 12)), "clip 0")):
        assert call(**kw) == -1, kw
        assert word in L.crispy_last_error().decode(), (kw, L.crispy_last_error())

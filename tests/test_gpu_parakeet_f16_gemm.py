"""GPU tests of the GEMM of the Parakeet encoder's precision mode 1 (pk_gemm_f16.hip) through crispy_pk_stage_gemm_device, which
runs a weight in the state-dict layout through the load's transposition, mode 1's pack kernel and the encoder's own launch_gemm
dispatch: exact operands bit for bit in both modes, random operands in all four epilogues, the rounding of both operands at
ties, subnormals, the largest finite f16 and overflow, the independence of a row from its place and its call, and the fused
q | k | v and GLU column orders.

Shapes: M one row, one below / on / one above the 128-row tile and two tiles + 1; K every odd and even multiple of 32 the
encoder meets (C * M / 8 = 160 among them) up to ffn 4096; N one and three column tiles.

The bound for random operands: mode 1's largest distance to float64 on the f16-rounded operands stays within
4 x the float32 torch product's own distance on the same rounded operands -- both are f32 sums of identical exact products."""
import numpy as np
import pytest

from crispy_amd import _native as N

pytestmark = pytest.mark.gpu

FACTOR = 4.0
TILE = N.PK_F16_TILE_M
MS = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
KS = (32, 96, 160, 64, 512, 1024, 4096)
NS = (128, 384)
EPI = {"scale": N.PK_GEMM_SCALE, "silu": N.PK_GEMM_SILU, "residual": N.PK_GEMM_RESIDUAL, "glu": N.PK_GEMM_GLU}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def f16(a):
    """a rounded once to binary16 by torch's cast, as f32"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float16).to(torch.float32).numpy()


@pytest.fixture(scope="module")
def enc():
    from crispy_amd import ParakeetEncoder
    e = ParakeetEncoder(0)      # no load: the stage needs none
    yield e
    e.close()


def reference(name, a, w, bias, alpha, res, dtype):
    """the stage in numpy at `dtype` on the operands as given: a [M][K], w [cols][K]"""
    a, w = a.astype(dtype), w.astype(dtype)
    v = a @ w.T
    if bias is not None:
        v = v + bias.astype(dtype)
    one = dtype(1.0)
    if name == "glu":
        n = w.shape[0] // 2
        return v[:, :n] / (one + np.exp(-v[:, n:]))
    if name == "silu":
        return v / (one + np.exp(-v))
    if name == "residual":
        return res.astype(dtype) + dtype(alpha) * v
    return v * dtype(alpha)


def random_case(name, M, K, n, seed):
    rng = np.random.default_rng(seed)
    cols = 2 * n if name == "glu" else n
    a = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((cols, K)) / np.sqrt(K)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(cols)).astype(np.float32)
    res = rng.standard_normal((M, n)).astype(np.float32) if name == "residual" else None
    alpha = {"scale": 16.0, "residual": 0.5}.get(name, 1.0)
    return a, w, bias, alpha, res


@pytest.mark.parametrize("K", KS)
def test_exact_operands_bit_for_bit(enc, K):
    """small integers times a power of two: every partial sum is exact in f32, so any order gives the float64 result's bits"""
    rng = np.random.default_rng(K)
    for n in NS:
        w = (rng.integers(-8, 9, (n, K)) * 2.0 ** -3).astype(np.float32)
        bias = (rng.integers(-16, 17, n) * 2.0 ** -2).astype(np.float32)
        for M in MS:
            a = (rng.integers(-8, 9, (M, K)) * 2.0 ** -2).astype(np.float32)
            res = (rng.integers(-64, 65, (M, n)) * 2.0 ** -2).astype(np.float32)
            for name, alpha in (("scale", 0.25), ("residual", 0.5)):
                want = reference(name, a, w, bias, alpha, res, np.float64)
                assert np.array_equal(want, want.astype(np.float32).astype(np.float64))
                for mode in (1, 0):
                    got = enc.stage_gemm(mode, EPI[name], a, w, bias, alpha, res if name == "residual" else None)
                    assert got.shape == (M, n)
                    assert np.array_equal(bits(got), bits(want.astype(np.float32))), (mode, name, M, K, n)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(EPI))
def test_random_operands_every_epilogue(enc, name, K):
    worst = 0.0
    for n in NS:
        for M in MS:
            a, w, bias, alpha, res = random_case(name, M, K, n, 1000 * K + 10 * M + n)
            ar, wr = f16(a), f16(w)
            r64 = reference(name, ar, wr, bias, alpha, res, np.float64)
            r32 = reference(name, ar, wr, bias, alpha, res, np.float32)
            got = enc.stage_gemm(1, EPI[name], a, w, bias, alpha, res)
            assert got.shape == r64.shape and np.isfinite(got).all()
            yard = float(np.abs(r32.astype(np.float64) - r64).max())
            err = float(np.abs(got.astype(np.float64) - r64).max())
            print(f"pk f16 gemm {name} M {M} K {K} N {n}: float32 product {yard:.3e}, mode 1 {err:.3e} from float64 (ratio {err / yard:.2f})")
            worst = max(worst, err / yard)
            # and the bound tells mode 1 from mode 0: the unrounded operands' float64 result lies far outside it
            plain = reference(name, a, w, bias, alpha, res, np.float64)
            assert np.abs(plain - r64).max() > 8 * FACTOR * yard, (name, M, K, n)
    assert worst <= FACTOR, (name, K, worst)


def special_values():
    """f32 values on f16 ties, just either side of them, f16 subnormals and the largest finite f16"""
    t = np.float32(2.0 ** -11)      # half an ulp of f16 at 1.0
    vals = [1.0 + t, np.nextafter(np.float32(1.0 + t), np.float32(2)), np.nextafter(np.float32(1.0 + t), np.float32(0)), 1.0 + 3 * t,
            np.nextafter(np.float32(1.0 + 3 * t), np.float32(2)), np.nextafter(np.float32(1.0 + 3 * t), np.float32(0)), -(1.0 + t), -(1.0 + 3 * t),
            2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 3 * 2.0 ** -25,
            2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), -(2.0 ** -24), 2.0 ** -26, 65504.0, -65504.0, 65519.0, 0.333333, -1e-3, 0.0]
    return np.asarray(vals, np.float32)


def test_rounding_of_a(enc):
    """W the identity: row m of the result is row m of A after the rounding"""
    K = n = 128
    vals = special_values()
    a = np.zeros((TILE + 2, K), np.float32)
    a[0, :len(vals)] = vals
    a[1, :len(vals)] = vals[::-1]
    a[TILE + 1, 7:7 + len(vals)] = vals
    a[5] = np.random.default_rng(3).standard_normal(K).astype(np.float32)
    w = np.eye(n, K, dtype=np.float32)
    want = f16(a)
    assert (want[0, 8:11] != 0).all() and want[0, 11] == 0      # torch's cast keeps the subnormals and rounds 2^-25 to even
    got = enc.stage_gemm(1, EPI["scale"], a, w)
    assert np.array_equal(bits(got), bits(want))
    # a value that rounds to infinity: its row is non-finite, every other row keeps its bytes
    over = a.copy()
    over[3, 17] = 65520.0
    over[TILE, 0] = -1e9
    got2 = enc.stage_gemm(1, EPI["scale"], over, w)
    for r in (3, TILE):
        assert not np.isfinite(got2[r]).any()
    keep = [r for r in range(a.shape[0]) if r not in (3, TILE)]
    assert np.isfinite(got2[keep]).all() and np.array_equal(bits(got2[keep]), bits(got[keep]))
    # mode 0 on the same call does not round
    assert np.array_equal(bits(enc.stage_gemm(0, EPI["scale"], a, w)), bits(a))


def test_rounding_of_w(enc):
    """A the identity: column n of the result is row n of W after the rounding"""
    K = M = 128
    n = 128
    vals = special_values()
    w = np.zeros((n, K), np.float32)
    w[0, :len(vals)] = vals
    w[33, 40:40 + len(vals)] = vals
    w[127, 128 - len(vals):] = vals
    w[64] = np.random.default_rng(4).standard_normal(K).astype(np.float32) * 1e-6      # mostly f16 subnormals
    a = np.eye(M, K, dtype=np.float32)
    got = enc.stage_gemm(1, EPI["scale"], a, w)
    want = f16(w).T + np.float32(0.0)      # a weight that rounds to -0 gives +0: the sum of a -0 product and the +0 ones
    bad = np.argwhere(bits(got) != bits(want))
    print(f"pk f16 gemm rounding of W: {len(bad)} differing values", [(int(m), int(c), float(got[m, c]), float(want[m, c])) for m, c in bad[:8]])
    assert len(bad) == 0


def test_rows_do_not_depend_on_place_or_call(enc):
    K, n, M = 160, 384, 2 * TILE + 1
    a, w, bias, alpha, res = random_case("residual", M, K, n, 77)
    whole = enc.stage_gemm(1, EPI["residual"], a, w, bias, alpha, res)
    again = enc.stage_gemm(1, EPI["residual"], a, w, bias, alpha, res)
    assert np.array_equal(bits(whole), bits(again))
    for r in (0, 1, 31, 32, 63, 64, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE):
        alone = enc.stage_gemm(1, EPI["residual"], a[r:r + 1], w, bias, alpha, res[r:r + 1])
        assert np.array_equal(bits(alone[0]), bits(whole[r])), r
    moved = enc.stage_gemm(1, EPI["residual"], a[::-1].copy(), w, bias, alpha, res[::-1].copy())      # every row at another place of the tiles
    assert np.array_equal(bits(moved[::-1]), bits(whole))
    loud = a.copy()
    loud[1::2] *= 1e4      # neighbours 1e4 times larger
    mixed = enc.stage_gemm(1, EPI["residual"], loud, w, bias, alpha, res)
    assert np.array_equal(bits(mixed[0::2]), bits(whole[0::2]))


@pytest.mark.parametrize("name", ["scale", "glu"])
def test_column_orders_as_mode_0(enc, name):
    """the fused q | k | v matrix (three H x H blocks side by side) and pointwise_conv1's value / gate order: on f16-representable
    operands both modes compute the same products, and both stay within the bound of float64 in the state dict's own order"""
    H, M = 128, TILE + 1
    rng = np.random.default_rng(11)
    cols = 3 * H if name == "scale" else 2 * H
    n = cols // 2 if name == "glu" else cols
    a = f16(rng.standard_normal((M, H)))
    w = f16(rng.standard_normal((cols, H)) / np.sqrt(H)) * (1 + np.arange(cols, dtype=np.float32)[:, None] % 3)      # blocks told apart
    w = f16(w)
    bias = (0.1 * rng.standard_normal(cols)).astype(np.float32)
    r64 = reference(name, a, w, bias, 1.0, None, np.float64)
    yard = float(np.abs(reference(name, a, w, bias, 1.0, None, np.float32).astype(np.float64) - r64).max())
    got1, got0 = enc.stage_gemm(1, EPI[name], a, w, bias), enc.stage_gemm(0, EPI[name], a, w, bias)
    assert got1.shape == (M, n)
    e1, e0 = float(np.abs(got1 - r64).max()), float(np.abs(got0 - r64).max())
    print(f"pk f16 gemm column order {name}: float32 product {yard:.3e}, mode 1 {e1:.3e}, mode 0 {e0:.3e} from float64")
    assert e1 <= FACTOR * yard and e0 <= FACTOR * yard
    assert float(np.abs(got1.astype(np.float64) - got0).max()) <= 2 * FACTOR * yard


def test_argument_errors(enc):
    a = np.zeros((4, 64), np.float32)
    w = np.zeros((128, 64), np.float32)
    for mode in (2, -1):
        with pytest.raises(N.CrispyError, match=f"mode {mode}") as e:
            enc.stage_gemm(mode, EPI["scale"], a, w)
        assert e.value.code == -1
    with pytest.raises(N.CrispyError, match="epilogue 4"):
        enc.stage_gemm(1, 4, a, w)
    with pytest.raises(N.CrispyError, match="K 48"):
        enc.stage_gemm(1, EPI["scale"], np.zeros((4, 48), np.float32), np.zeros((128, 48), np.float32))
    with pytest.raises(N.CrispyError, match="columns"):
        enc.stage_gemm(1, EPI["scale"], a, np.zeros((192, 64), np.float32))
    with pytest.raises(N.CrispyError, match="d_res"):
        enc.stage_gemm(1, EPI["residual"], a, w)
    assert enc.stage_gemm(1, EPI["scale"], a, w).shape == (4, 128)      # the handle still works

"""Encoder self-attention in the PEAKED regime: a one-layer model whose attention operands are exact, and what the tests
derive from it.

Pure numpy and importable without a GPU: tests/test_enc_attn_cases.py asserts this builder's own conditions on the CPU,
tests/test_gpu_encoder_attention.py runs the cases through attn_enc_h_kernel<false> (precision mode 1), attn_enc_h_kernel<true>
(mode 2) and attn_enc_kernel (mode 0).

Why a fixture of its own.  With the suite's seeded weights the soft-max rows of the encoder are nearly uniform (row maximum
minus row median of t = score x log2(e): 3.5), so the reference exponent of the mode-1 kernel is raised after key tile 0 on 20 of
9000 rows, once each, and nothing it multiplies ever leaves the normal f16 range.  Scaling q and k of such a model makes the
rows peaked but the comparison blunt: in modes 1 and 2 GPU and oracle round LN(x), q, k and v to f16 from values that agree
to f32 accuracy only, ~0.1 % land on the other side of a rounding boundary, and at t ~ 100 one f16 step on a q or k entry
moves a probability by a few percent.  Here every operand that reaches the attention kernel is EXACTLY representable, so kernel
and oracle see the same bits and what is left is the attention's own arithmetic:

  encoder.conv2.* = 0        GELU(0) = 0 in both GELU forms: the residual stream entering the layer is the positional
                             embedding, a weight the test owns -- the table P [1500][d] below.  (The output does not depend
                             on the audio.)
  rows of P                  +-1 with as many +1 as -1: mean 0, variance 1, so with gamma = 1, beta = 0 LN(P) = +-0.999995,
                             which rounds to f16 +-1.0 from 2.4e-4 inside the boundary.
  query | key | value        sparse; entries are small integers times powers of two: every q, k, v entry is an exactly
                             computed integer or dyadic value that f16 holds (`operands(...).exact`).
  attn.out = identity, mlp.2 = 0, ln_post gamma 1 beta 0
                             the output is LN(P + h(att)); columns 64 h .. 64 h + 63 belong to head h.

Columns of P.  Position codes, each with its complement (the row balance), then seeded balanced random signs:
  CONST        +1                                 a key bias (k has none): the query's bias against it centres the row maximum
                                                  of t near 0, so that the f32 constant log2(e) / 8 of the kernels (1.3e-8 off)
                                                  moves no probability by more than the accumulation noise does
  TH_j         +1 if t >= 32 j, j = 1 .. 46       sum = 2 tile - 46: integer ramps over key tiles
  B_i          +1 if bit i of t % 32, i = 0 .. 4  sum 2^i B_i = 2 (t % 32) - 31: the ramp inside a tile; B_0 alternates from
                                                  query to query, i.e. inside every group of 32 queries (one wave)
  ONE          +1 at key 777 only

Heads (t = q.k / 8 x log2(e); u = log2(e) / 8 = 0.18 is t per unit of q.k).  Every head but H4 adds twelve +-1/2 x +-1 terms of
random columns (+-1.08 in t at the most), so that the rows of a head differ:
  H0  stale reference   t rises by 1.08 per tile (0.034 per key) over 49.8: the reference is raised every ~6th tile and
                        p = 2^(t - m) exceeds 1 in between
  H1  every tile        t rises by 7.9 per tile over tiles 20 .. 31
  H2  descending        t falls by 1.44 per tile from tile 0: the keys from tile 18 on are more than 25 below
  H3  tail tile         odd queries: maximum at key 1499 (the last key of the partial tile 1472 .. 1499), 4 above the rest, no
                        raise needed; even queries: maximum at key 1472, 32.8 above, raise needed (so far above that the other
                        tiles round to zero under the oracle's reference and under the kernel's: see the notebook on the
                        reference spread).  Inside a tile t moves by 7.2 per key.  The keys 1500 .. 1503 of the tile do not
                        exist; a kernel that let them in would give odd queries a larger maximum.
  H4  random peaked     q = +-3 | +-6 of one random column, k = 2 x one random column + another, in 62 dimensions (|q| is the
                        same in every row, so the row maxima stay within -11 .. +22 of the centre)
  H5  analytic          q = 0: uniform soft-max, every output row is the mean of v over the 1500 keys
  H6  (512) one key     key 777 leads every other by 46: the output row is v[777]
  H7  (512) mixed wave  H1's ramp with the sign of B_0(query): rising for odd queries, falling for even ones, in one wave
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T = 1500
TILE = 32
N_TILES = (T + TILE - 1) // TILE               # 47, the last one 1472 .. 1499
U = float(np.log2(np.e) / 8.0)                # t per unit of q.k
RAISE_ABOVE = 6.0                             # the kernel's rule: raise to ceil(max) when a tile maximum exceeds the reference by more
ONE_KEY = 777
NOISE = 3e-7                                  # relative, in front of the P and h(att) roundings (tests/test_gpu_whisper.py:
NOISE_SEEDS = 5                               # test_f16_operand_mode_matches_the_f16_operand_oracle documents the method)

# code columns of P; code c has its complement at N_CODES + c
CONST, TH0, B0, ONE = 0, 0, 47, 52           # TH_j = column TH0 + j, j = 1 .. 46; B_i = column B0 + i
N_CODES = 53

HEADS = {384: ("H0", "H1", "H2", "H3", "H4", "H5"), 512: ("H0", "H1", "H2", "H3", "H4", "H5", "H6", "H7")}
H1_TILES = range(20, 32)                      # thermometers of H1's ramp
H0_GAIN, H1_GAIN, H2_GAIN, H3_G, H3_g, H6_GAIN = 3, 22, 4, 91, 20, 128
H4_CENTRE = 273
N_JITTER = 12


def hparams(d: int):
    """One encoder layer of width d and the smallest decoder crispy_asr_create accepts (one layer of the smallest width, a
    vocabulary and a context of a few entries: nothing here decodes)."""
    from crispy_amd.whisper_weights import HParams
    assert d in HEADS
    return HParams(n_vocab=32, n_audio_ctx=T, n_audio_state=d, n_audio_head=d // 64, n_audio_layer=1, n_text_ctx=4,
                   n_text_state=384, n_text_head=6, n_text_layer=1, n_mels=80)


def position_table(d: int, seed: int = 0) -> np.ndarray:
    """P [1500][d], +-1, every row balanced."""
    t = np.arange(T)
    codes = -np.ones((T, N_CODES))
    codes[:, CONST] = 1.0
    for j in range(1, N_TILES):
        codes[t >= TILE * j, TH0 + j] = 1.0
    for i in range(5):
        codes[((t % TILE) >> i) & 1 == 1, B0 + i] = 1.0
    codes[ONE_KEY, ONE] = 1.0
    n_rand = d - 2 * N_CODES
    assert n_rand > 0 and n_rand % 2 == 0
    rng = np.random.default_rng([seed, d, 1])
    half = np.concatenate([np.ones(n_rand // 2), -np.ones(n_rand // 2)])
    rand = np.stack([rng.permutation(half) for _ in range(T)])
    return np.concatenate([codes, -codes, rand], axis=1).astype(np.float32)


@lru_cache(maxsize=None)
def build(d: int, seed: int = 0):
    """(hp, W) of the fixture.  W holds every tensor of tests' usual inventory; the decoder is all zeros."""
    from crispy_amd.whisper_weights import synthetic_tensor, tensor_shapes
    hp = hparams(d)
    W = {name: np.zeros(shape, dtype=np.float32) for name, shape in tensor_shapes(hp).items()}
    for name in ("encoder.conv1.weight", "encoder.conv1.bias"):           # any finite stem: conv2 = 0 cuts it off
        W[name] = synthetic_tensor(name, W[name].shape, seed)
    W["encoder.positional_embedding"] = position_table(d, seed)
    for name in W:
        if name.endswith("ln.weight") or name.endswith("ln_post.weight"):
            W[name][:] = 1.0
    p = "encoder.blocks.0.attn."
    W[p + "out.weight"] = np.eye(d, dtype=np.float32)
    Wq, bq, Wk, Wv, bv = (W[p + n] for n in ("query.weight", "query.bias", "key.weight", "value.weight", "value.bias"))
    rng = np.random.default_rng([seed, d, 2])
    n_rand = d - 2 * N_CODES
    rcol = lambda n: 2 * N_CODES + rng.choice(n_rand, size=n, replace=False)      # noqa: E731
    for h, name in enumerate(HEADS[d]):
        r = 64 * h                                                      # first row of the head in Wq | Wk | Wv
        centre = 0
        if name == "H0":
            bq[r], bq[r + 1] = H0_GAIN, H0_GAIN
            Wk[r, TH0 + 1:TH0 + N_TILES] = 1.0
            Wk[r + 1, B0:B0 + 5] = 2.0 ** (np.arange(5) - 5)
            centre = H0_GAIN * (N_TILES - 1)
        elif name in ("H1", "H7"):
            if name == "H1":
                bq[r] = H1_GAIN
            else:
                Wq[r, B0] = H1_GAIN
            Wk[r, [TH0 + j for j in H1_TILES]] = 1.0
            centre = H1_GAIN * len(H1_TILES)
        elif name == "H2":
            bq[r] = -H2_GAIN
            Wk[r, TH0 + 1:TH0 + N_TILES] = 1.0
            centre = H2_GAIN * (N_TILES - 1)
        elif name == "H3":
            bq[r] = H3_G
            Wk[r, TH0 + N_TILES - 1] = 1.0
            Wq[r + 1, B0] = H3_g
            Wk[r + 1, B0:B0 + 5] = 2.0 ** np.arange(5)
            centre = H3_G + 27 * H3_g
        elif name == "H4":
            for i, (a, c, e) in enumerate(zip(rcol(62), rcol(62), rcol(62))):      # |q| is the same for every row
                Wq[r + i, a] = 6.0 if i % 2 else 3.0
                Wk[r + i, c], Wk[r + i, e] = 2.0, 1.0
            bq[r + 62] = -H4_CENTRE
            Wk[r + 62, CONST] = 1.0
        elif name == "H6":
            bq[r] = H6_GAIN
            Wk[r, ONE] = 1.0
            centre = H6_GAIN
        if name not in ("H4", "H5"):
            bq[r + 2] = -centre
            Wk[r + 2, CONST] = 1.0
        if name != "H4":                                                # twelve +-1/2 x +-1 terms (H5: keys only, its q stays 0)
            for i, (a, b) in enumerate(zip(rcol(N_JITTER), rcol(N_JITTER))):
                if name != "H5":
                    Wq[r + 64 - N_JITTER + i, a] = 0.5
                Wk[r + 64 - N_JITTER + i, b] = 1.0
        for i, a in enumerate(rcol(64)):                                # v: dyadic, |v| <= 3.5 in steps of 1 / 4
            Wv[r + i, a] = (1.0, 2.0, 0.5)[i % 3]
            Wv[r + i, TH0 + 1 + (7 * i + h) % (N_TILES - 1)] = 0.5
            bv[r + i] = (i % 8 - 4) / 4.0
    for w in W.values():
        w.setflags(write=False)
    return hp, W


# ---- what the oracle makes of the fixture ------------------------------------------------------------------------------

@dataclass(frozen=True)
class Operands:
    P: np.ndarray            # float64 [1500][d]
    q: np.ndarray            # the f16-operand oracle's q, k, v (float64 holding f16 values)
    k: np.ndarray
    v: np.ndarray
    exact: dict              # name -> bool: the rounding to f16 changed nothing


@lru_cache(maxsize=None)
def operands(d: int, seed: int = 0) -> Operands:
    """q, k, v as oracle/whisper_oracle.py::encoder_forward_f16 computes them in layer 0 (the same expressions)."""
    from oracle import whisper_oracle as WO
    hp, W = build(d, seed)
    W64 = WO._f64(W)
    p = "encoder.blocks.0"
    P = W64["encoder.positional_embedding"]
    ln = WO._ln(P, W64[p + ".attn_ln.weight"], W64[p + ".attn_ln.bias"])
    xn = WO._h(ln)
    q0 = xn @ WO._h(W64[p + ".attn.query.weight"]).T + W64[p + ".attn.query.bias"]
    k0 = xn @ WO._h(W64[p + ".attn.key.weight"]).T
    v0 = xn @ WO._h(W64[p + ".attn.value.weight"]).T + W64[p + ".attn.value.bias"]
    q, k, v = WO._h(q0), WO._h(k0), WO._h(v0)
    exact = {"xn": bool(np.array_equal(np.abs(xn), np.ones_like(xn))) and float(np.abs(np.abs(ln) - 1.0).max()) < 1e-5,
             "q": bool(np.array_equal(q, q0)), "k": bool(np.array_equal(k, k0)), "v": bool(np.array_equal(v, v0)),
             "weights": all(np.array_equal(WO._h(W64[p + f".attn.{n}.weight"]), W64[p + f".attn.{n}.weight"])
                            for n in ("query", "key", "value", "out"))}
    return Operands(P, q, k, v, exact)


def t_matrix(q: np.ndarray, k: np.ndarray, h: int) -> np.ndarray:
    """t [query][key] of head h, the oracle's expression."""
    sl = slice(64 * h, 64 * h + 64)
    return (q[:, sl] @ k[:, sl].T) / np.sqrt(64) * np.log2(np.e)


def kernel_order(t: np.ndarray):
    """attn_enc_h_kernel's reference exponent, row by row, from t alone: the reference starts below everything, and a tile of 32
    keys whose maximum exceeds it by more than 6 raises it to ceil(max(reference, tile maximum)).  Returns (raises after
    tile 0 per row, rows where some p = 2^(t - reference) exceeds 1, the largest t - reference)."""
    n = t.shape[0]
    m = np.full(n, -1e30)
    raises = np.zeros(n, dtype=np.int64)
    above = np.zeros(n, dtype=bool)
    top = -np.inf
    for it in range(N_TILES):
        tt = t[:, it * TILE:(it + 1) * TILE]
        mloc = tt.max(-1)
        up = mloc > m + RAISE_ABOVE
        m = np.where(up, np.ceil(np.maximum(m, mloc)), m)
        if it:
            raises += up
        above |= mloc > m
        top = max(top, float((mloc - m).max()))
    return raises, above, top


def attention(t: np.ndarray, v: np.ndarray, mode: int, lower: float = 0.0, rng=None, round_p: bool = True) -> np.ndarray:
    """One head's attention output in front of its f16 rounding, with the oracle's expressions (mode 1: 2^(t - integer) rounded,
    the sum unrounded; mode 2: normalised, then rounded).  lower: the integer reference ceil(row max) lowered by this much
    (mode 1).  rng: relative noise of NOISE (uniform) in front of the P rounding.  round_p=False: the exact soft-max."""
    from oracle import whisper_oracle as WO
    rnd = WO._h if round_p else (lambda a: a)
    noise = (lambda a: a) if rng is None else (lambda a: a * (1.0 + NOISE * rng.uniform(-1.0, 1.0, a.shape)))
    if mode == 2:
        pe = np.exp2(t - t.max(-1, keepdims=True))
        return rnd(noise(pe / pe.sum(-1, keepdims=True))) @ v
    assert mode == 1
    pe = np.exp2(t - (np.ceil(t.max(-1, keepdims=True)) - lower))
    return (rnd(noise(pe)) @ v) / pe.sum(-1, keepdims=True)


def all_heads(d: int, mode: int, seed: int = 0, **kw) -> np.ndarray:
    """attention() of every head, [1500][d]."""
    op = operands(d, seed)
    return np.concatenate([attention(t_matrix(op.q, op.k, h), op.v[:, 64 * h:64 * h + 64], mode, **kw)
                           for h in range(d // 64)], axis=1)


def layer_output(P: np.ndarray, att: np.ndarray, rng=None, dtype=np.float64) -> np.ndarray:
    """LN(P + h(att)): the encoder's output on this fixture.  rng: relative noise in front of the h(att) rounding.  dtype: the
    precision of the final LayerNorm's arithmetic."""
    from oracle import whisper_oracle as WO
    if rng is not None:
        att = att * (1.0 + NOISE * rng.uniform(-1.0, 1.0, att.shape))
    x = (P + WO._h(att)).astype(dtype)
    return WO._ln(x, dtype(1.0), dtype(0.0), eps=dtype(1e-5)).astype(np.float64)


def f16_step(a: np.ndarray) -> np.ndarray:
    """The distance from |a| to the next f16 value above it."""
    return np.spacing(np.abs(a).astype(np.float16)).astype(np.float64)


def row_sigma(P: np.ndarray, att: np.ndarray) -> np.ndarray:
    from oracle import whisper_oracle as WO
    return np.sqrt((P + WO._h(att)).var(-1, keepdims=True) + 1e-5)


P_FLIP_TOP = 8


def p_flip_reach(d: int, mode: int, seed: int = 0) -> np.ndarray:
    """How far ONE probability that lands on the other side of an f16 boundary moves an attention output, [1500][d]: the f16
    spacing at the probability times |v| of that key (mode 1: over the row's sum), the largest over the keys -- the
    P_FLIP_TOP keys of largest probability one by one, the others through the largest |v| of the column.  Where a row leans on
    one or two keys this is 2^-11 x |v|, as much as one f16 step of the output at its largest and many steps of an output that
    is small because its terms cancel: `one f16 step of h(att)` alone is not a bound that holds for the oracle under noise
    (mode 2, width 384, noise seed 999: one flipped probability of row 921 moves 45 of H3's 64 outputs, 9 of them by 2 .. 10
    of their own steps)."""
    from oracle import whisper_oracle as WO
    op = operands(d, seed)
    out = np.empty((T, d))
    for h in range(d // 64):
        sl = slice(64 * h, 64 * h + 64)
        t, v = t_matrix(op.q, op.k, h), np.abs(op.v[:, sl])
        if mode == 2:
            pe = np.exp2(t - t.max(-1, keepdims=True))
            w, norm = pe / pe.sum(-1, keepdims=True), 1.0
        else:
            w = np.exp2(t - np.ceil(t.max(-1, keepdims=True)))
            norm = w.sum(-1, keepdims=True)
        ulp = np.spacing(WO._h(w).astype(np.float16)).astype(np.float64) / norm
        top = np.argpartition(-ulp, P_FLIP_TOP, axis=-1)[:, :P_FLIP_TOP + 1]
        u = np.take_along_axis(ulp, top, axis=-1)
        order = np.argsort(-u, axis=-1)
        top, u = np.take_along_axis(top, order, axis=-1), np.take_along_axis(u, order, axis=-1)
        reach = u[:, P_FLIP_TOP:] * v.max(0, keepdims=True)                # every key beyond the top ones
        for k in range(P_FLIP_TOP):
            reach = np.maximum(reach, u[:, k:k + 1] * v[top[:, k]])
        out[:, sl] = reach
    return out


def coarse_bound(d: int, mode: int, att: np.ndarray, seed: int = 0) -> np.ndarray:
    """What ANY output element may differ by, in front of the fine bar: one f16 step of h(att) and one flipped probability,
    carried through ln_post (over the row's sigma)."""
    op = operands(d, seed)
    return (f16_step(att) + p_flip_reach(d, mode, seed)) / row_sigma(op.P, att)


def measure_bars(d: int, mode: int, seed: int = 0) -> dict:
    """The CPU measurement behind the GPU file's bars (modes 1 and 2): the oracle against itself with relative noise of NOISE in
    front of its P rounding and its h(att) rounding, the worst of NOISE_SEEDS noise seeds.  Per head: `share` = the share of
    output elements whose h(att) came out as another f16 value, `unflipped` = the largest output difference on the others
    (what a flip elsewhere in the row does to the row's mean and variance); `ln32` = the final LayerNorm in single against
    double precision on the clean input."""
    from oracle import whisper_oracle as WO
    op = operands(d, seed)
    att = all_heads(d, mode, seed)
    ref = layer_output(op.P, att)
    ln32 = float(np.abs(layer_output(op.P, att, dtype=np.float32) - ref).max())
    H = d // 64
    share, unflipped = np.zeros(H), np.zeros(H)
    for s in range(NOISE_SEEDS):
        rng = np.random.default_rng([seed, d, mode, 100 + s])
        att_n = all_heads(d, mode, seed, rng=rng)
        noise = 1.0 + NOISE * rng.uniform(-1.0, 1.0, att_n.shape)
        same = WO._h(att_n * noise) == WO._h(att)
        out = layer_output(op.P, att_n * noise)
        for h in range(H):
            sl = slice(64 * h, 64 * h + 64)
            share[h] = max(share[h], 1.0 - same[:, sl].mean())
            unflipped[h] = max(unflipped[h], float(np.abs(out - ref)[:, sl][same[:, sl]].max()))
    return {"share": share, "unflipped": unflipped, "ln32": ln32}


FINE_FACTOR, CAP_FACTOR, CAP_MOST = 4.0, 3.0, 0.01


def bars(d: int, mode: int, seed: int = 0) -> dict:
    """Per head, from measure_bars (through the committed cache, tests/oracle_cache.py): `fine` = 4 x (unflipped + ln32), in
    units of the output; `cap` = 3 x share, at most 1 % of the head's elements."""
    from tests.oracle_cache import cached, fingerprint
    hp, W = build(d, seed)
    fp = fingerprint("enc_attn_bars", d, mode, seed, NOISE, NOISE_SEEDS, W["encoder.positional_embedding"],
                     {n: W["encoder.blocks.0.attn." + n] for n in ("query.weight", "query.bias", "key.weight", "value.weight", "value.bias")})
    m = cached(f"enc_attn_bars_{d}_mode{mode}", fp, lambda: measure_bars(d, mode, seed))
    share, unflipped = np.asarray(m["share"]), np.asarray(m["unflipped"])
    return {"fine": FINE_FACTOR * (unflipped + float(m["ln32"])), "cap": np.minimum(CAP_FACTOR * share, CAP_MOST),
            "share": share, "unflipped": unflipped, "ln32": float(m["ln32"])}


def closed_forms(d: int, mode: int, seed: int = 0) -> dict:
    """name -> [1][64]: what the analytic heads' attention must put out in every row, from v alone.  H5: the mean of v over the
    1500 keys; H6: v of key 777 (the other 1499 keys weigh 2^-46 each).  Modes 1 and 2: the f16-operand oracle's v; mode 0: v from
    LN(P) as it is (+-0.999995)."""
    from oracle import whisper_oracle as WO
    if mode == 0:
        hp, W = build(d, seed)
        W64 = WO._f64(W)
        p = "encoder.blocks.0"
        xn = WO._ln(W64["encoder.positional_embedding"], W64[p + ".attn_ln.weight"], W64[p + ".attn_ln.bias"])
        v = xn @ W64[p + ".attn.value.weight"].T + W64[p + ".attn.value.bias"]
    else:
        v = operands(d, seed).v
    h = HEADS[d].index("H5")
    out = {"H5": v[:, 64 * h:64 * h + 64].mean(0, keepdims=True)}
    if "H6" in HEADS[d]:
        h = HEADS[d].index("H6")
        out["H6"] = v[ONE_KEY:ONE_KEY + 1, 64 * h:64 * h + 64]
    return out


MODE0_BAR_FACTOR, MODE0_BAR_MOST, MODE0_GAP_MOST = 4.0, 1e-4, 2.5e-5


def mode0_bar(gap: float) -> float:
    """Precision mode 0 against the float64 oracle: 4 x the distance of the oracle's own single-precision run from it (of the
    peak), never above the project's 1e-4; a gap above 2.5e-5 means the inputs are too sharp for single precision itself."""
    assert gap < MODE0_GAP_MOST, gap
    return min(MODE0_BAR_FACTOR * gap, MODE0_BAR_MOST)


def zero_mel():
    return np.zeros((80, 3000))


def measure_mode0_gap(d: int, seed: int = 0) -> dict:
    from oracle import whisper_oracle as WO
    hp, W = build(d, seed)
    r64 = WO.encoder_forward(W, hp, zero_mel())
    r32 = WO.encoder_forward(W, hp, zero_mel(), dtype=np.float32)
    return {"gap": float(np.abs(r32 - r64).max() / np.abs(r64).max())}


def mode0_gap(d: int, seed: int = 0) -> float:
    from tests.oracle_cache import cached, fingerprint
    hp, W = build(d, seed)
    fp = fingerprint("enc_attn_mode0_gap", d, seed, W["encoder.positional_embedding"],
                     {n: W["encoder.blocks.0.attn." + n] for n in ("query.weight", "query.bias", "key.weight", "value.weight", "value.bias")})
    return float(cached(f"enc_attn_mode0_gap_{d}", fp, lambda: measure_mode0_gap(d, seed))["gap"])


# ---- the ordinary weights, and the ordinary model made peaked ----------------------------------------------------------------

def layer0_t(W, hp, mel):
    """t [head][query][key] of layer 0 as encoder_forward_f16 computes it (the same expressions up to the scores)."""
    from oracle import whisper_oracle as WO
    W64 = WO._f64(W)
    x = WO._h(mel)
    xp = np.pad(x, ((0, 0), (1, 1)))
    w1 = WO._h(W64["encoder.conv1.weight"])
    h1 = sum(w1[:, :, k] @ xp[:, k:k + 3000] for k in range(3)) + W64["encoder.conv1.bias"][:, None]
    hp1 = np.pad(WO._h(WO._gelu_ggml(h1)), ((0, 0), (1, 1)))
    w2 = WO._h(W64["encoder.conv2.weight"])
    h2 = sum(w2[:, :, k] @ hp1[:, k:k + 3000:2][:, :1500] for k in range(3)) + W64["encoder.conv2.bias"][:, None]
    x = WO._gelu_ggml(h2).T + W64["encoder.positional_embedding"]
    p = "encoder.blocks.0"
    xn = WO._h(WO._ln(x, W64[p + ".attn_ln.weight"], W64[p + ".attn_ln.bias"]))
    q = WO._h(xn @ WO._h(W64[p + ".attn.query.weight"]).T + W64[p + ".attn.query.bias"])
    k = WO._h(xn @ WO._h(W64[p + ".attn.key.weight"]).T)
    return np.stack([t_matrix(q, k, h) for h in range(hp.n_audio_head)])


CHAIN_CLIPS = ((0, 464000), (5, 130000), (7, 52000))     # (seed, samples) of synth_audio.clip16k_np; the third only fills the batch
CHAIN_ROWS = tuple(128 * i + (37 * i) % 128 for i in range(11)) + (1499,)     # encoder rows kept per clip in the cache: one per block
                                                         # of 128 queries (a workgroup of the attention kernels), the last row
CHAIN_SCALE = 2.0      # x 4 was asked for first: there the oracle in single precision is 6.6e-5 / 3.7e-5 of the peak from the one in
                       # double precision (clips 0 / 5), above MODE0_GAP_MOST; x 2 is the largest power of two below it (9.3e-7 / 1.07e-6)


def peaked_tiny(scale: float = CHAIN_SCALE, seed: int = 0):
    """(hp, W) of the suite's ordinary 4-layer tiny model with the encoder's query and key weights and the query bias times
    `scale`: sharper soft-max rows on operands that are NOT exact (see the GPU file)."""
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams.tiny()
    W = dict(synthetic_whisper_weights(hp, seed))
    for i in range(hp.n_audio_layer):
        for n in ("query.weight", "query.bias", "key.weight"):
            name = f"encoder.blocks.{i}.attn.{n}"
            W[name] = (W[name] * np.float32(scale)).astype(np.float32)
    return hp, W


def measure_chain(clip: int, scale: float = CHAIN_SCALE) -> dict:
    """The oracles of the peaked chain on one clip: float64, its single-precision gap, and the f16-operand one (the rows CHAIN_ROWS)."""
    from crispy_amd import synth_audio
    from crispy_amd.mel_filters import whisper_mel_filters
    from oracle import whisper_oracle as WO
    from tests import oracle_lib
    hp, W = peaked_tiny(scale)
    mel = oracle_lib.oracle_logmel(synth_audio.clip16k_np(*CHAIN_CLIPS[clip]), whisper_mel_filters(hp.n_mels))
    r64 = WO.encoder_forward(W, hp, mel)
    r32 = WO.encoder_forward(W, hp, mel, dtype=np.float32)
    r16 = WO.encoder_forward_f16(W, hp, mel)
    rows = np.array(CHAIN_ROWS, dtype=np.int64)
    peak = float(np.abs(r64).max())
    # kept as float32 (a third of a megabyte of text per clip otherwise): 6e-8 of a value, against bars from 4e-6 of the peak
    return {"rows": rows, "ref64": r64[rows].astype(np.float32), "ref16": r16[rows].astype(np.float32), "peak": peak,
            "gap": float(np.abs(r32 - r64).max() / peak)}


def chain_ref(clip: int, scale: float = CHAIN_SCALE) -> dict:
    from tests.oracle_cache import cached, fingerprint
    fp = fingerprint("enc_attn_chain", clip, CHAIN_CLIPS[clip], scale, CHAIN_ROWS)
    return cached(f"enc_attn_chain_clip{clip}", fp, lambda: measure_chain(clip, scale))

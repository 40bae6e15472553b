"""Oracle of the Parakeet encoder's attention mode 1 (crispy_pk_set_attention_precision, include/crispy_hip.h): tests/pk_oracle.py's
network with Attention.forward replaced by the definition below, in float64 or float32.

Definition, per (clip, head), over the clip's own n frames; q, k, v are the outputs of the fused projection, r the output of
relative_k_proj on the position table, u and vb the head's bias_u and bias_v.
  1. Five operands are rounded once to binary16 (torch.Tensor.to(torch.float16)): q + u and q + vb (the sums first), k, r and v.
  2. score(i, j) = (ac(i, j) + bd(i, i - j)) * f32(128^-1/2), ac = f16(q + u) . f16(k), bd(i, d) = f16(q + vb) . f16(r_d): the
     addition and the scale come after the sums.
  3. The soft-max runs over the keys in tiles of `key_tile`, ascending from key 0, with a running maximum and sum:
     m_new = max(m, tile max); alpha = exp(m - m_new); p = exp(score - m_new); l = l * alpha + sum(p) (p unrounded);
     o = o * alpha + f16(p) . f16(v); out = o / l.
The products and sums are those of the oracle's own precision (float64: exact; float32: the yardstick for f32 sums).  The tile
length is part of the definition: f16(p) is rounded relative to the running maximum, so the tile-32 and the tile-64 form differ
by far more than the float32 form's own error (tests/test_pk_attn_f16_oracle.py pins that).

`Encoder(c, weights, dtype, key_tile, attention, gemm)`: `attention` applies the definition, `gemm` also pk_f16_oracle's hooks (the
combined mode); with both off the class is pk_oracle.Encoder bit for bit."""
import types

import numpy as np
import torch

from tests import pk_f16_oracle as FO
from tests import pk_oracle as PO

HEAD = PO.HEAD
SCALE = float(np.float32(HEAD ** -0.5))      # the library's f32 constant
round_f16 = FO.round_f16


def attention(q, k, v, r, u, vb, tmax: int, key_tile: int, f16: bool = True):
    """q, k, v [heads][n][128], r [heads][2 tmax - 1][128] with row p for the distance d = p - (tmax - 1), u, vb [heads][128], all
    tensors of one dtype -> [heads][n][128].  With `f16` off: the exact attention of pk_oracle (one soft-max over all keys, no
    rounding), with the same scale."""
    n = q.shape[1]
    rd = round_f16 if f16 else (lambda x: x)
    qu, qv, kr, rr, vr = rd(q + u[:, None]), rd(q + vb[:, None]), rd(k), rd(r), rd(v)
    i = torch.arange(n)[:, None]
    j = torch.arange(n)[None, :]
    ac = qu @ kr.transpose(1, 2)
    bd = (qv @ rr.transpose(1, 2))[:, i, (i - j) + (tmax - 1)]
    score = (ac + bd) * SCALE
    if not f16:
        return torch.softmax(score, dim=-1) @ vr
    m = torch.full(score.shape[:2], -float("inf"), dtype=q.dtype)
    l = torch.zeros(score.shape[:2], dtype=q.dtype)
    o = torch.zeros_like(q)
    for j0 in range(0, n, key_tile):
        s = score[:, :, j0:j0 + key_tile]
        m_new = torch.maximum(m, s.max(dim=-1).values)
        alpha = torch.exp(m - m_new)
        p = torch.exp(s - m_new[..., None])
        l = l * alpha + p.sum(dim=-1)
        o = o * alpha[..., None] + round_f16(p) @ vr[:, j0:j0 + key_tile]
        m = m_new
    return o / l[..., None]


def stage(qkv, r, bias_u, bias_v, lengths, heads: int, tmax: int, key_tile: int, dtype=torch.float64, f16: bool = True) -> np.ndarray:
    """crispy_pk_stage_attention_device on numpy arrays: qkv [sum n][3 * heads * 128], r [2 tmax - 1][heads * 128], bias_u, bias_v
    [heads * 128] -> [sum n][heads * 128] in `dtype`"""
    H = heads * HEAD
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype)
    split = lambda y: y.reshape(y.shape[0], heads, HEAD).transpose(0, 1)
    rr, u, vb = split(t(r)), t(bias_u).reshape(heads, HEAD), t(bias_v).reshape(heads, HEAD)
    out, at = [], 0
    for n in lengths:
        x = t(qkv[at:at + n])
        o = attention(split(x[:, :H]), split(x[:, H:2 * H]), split(x[:, 2 * H:]), rr, u, vb, tmax, key_tile, f16)
        out.append(o.transpose(0, 1).reshape(n, H).numpy())
        at += n
    return np.concatenate(out, 0)


def _forward(self, x, pos, key_tile):      # Attention.forward with the definition; pos [2T - 1][H] for d = -(T - 1) ... T - 1
    t = x.shape[0]
    split = lambda y: y.view(y.shape[0], self.heads, HEAD).transpose(0, 1)
    q, k, v = split(self.q_proj(x)), split(self.k_proj(x)), split(self.v_proj(x))
    r = split(self.relative_k_proj(pos))      # row p: d = p - (T - 1)
    o = attention(q, k, v, r, self.bias_u, self.bias_v, t, key_tile)
    return self.o_proj(o.transpose(0, 1).reshape(t, -1))


class Encoder(FO.Encoder):
    """pk_oracle.Encoder with attention mode 1 (`attention`) and, with `gemm`, precision mode 1's GEMM hooks as well."""

    def __init__(self, c: PO.Config, weights: dict, dtype=torch.float64, key_tile: int = 32, attention: bool = True, gemm: bool = False):
        super().__init__(c, weights, dtype, hooks=gemm)
        self.key_tile = key_tile
        if attention:
            for blk in self.net.layers:
                blk.self_attn.forward = types.MethodType(lambda m, x, pos: _forward(m, x, pos, key_tile), blk.self_attn)

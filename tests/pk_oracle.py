"""Oracle of the Parakeet FastConformer encoder (crispy_pk_*, include/crispy_hip.h): the network as torch modules whose attribute
names give the state-dict keys of transformers' ParakeetEncoder, constructible in float32 and float64, on one clip at a time with
no mask.  The position table is part of the specification and the same numbers in both precisions.  tests/test_pk_oracle.py pins
this file on transformers.models.parakeet (where present) and on tests/golden/parakeet_enc_golden.npz."""
import math
from dataclasses import asdict, dataclass, replace

import numpy as np
import torch
from torch import nn

HEAD = 128


@dataclass(frozen=True)
class Config:
    hidden: int
    layers: int
    heads: int
    ffn: int
    conv_kernel: int
    mel_bins: int
    sub_channels: int
    attention_bias: int = 1
    convolution_bias: int = 1
    scale_input: int = 1

    def as_dict(self):
        return asdict(self)


TINY = Config(hidden=256, layers=3, heads=2, ffn=512, conv_kernel=9, mel_bins=128, sub_channels=32)
CATALOG_V3 = Config(hidden=1024, layers=24, heads=8, ffn=4096, conv_kernel=9, mel_bins=128, sub_channels=256)
with_flags = replace


def frames(rows: int) -> int:
    """T' for `rows` feature rows: L -> (L - 1) // 2 + 1 three times; 0 for rows < 1"""
    if rows < 1:
        return 0
    for _ in range(3):
        rows = (rows - 1) // 2 + 1
    return rows


def clip(rows: int, mel_bins: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """seeded feature rows f32 [rows][mel_bins]"""
    return (np.random.default_rng(seed).standard_normal((rows, mel_bins)) * scale).astype(np.float32)


GOLDEN_ROWS = (1, 8, 9, 17, 73, 300)      # tests/golden/parakeet_enc_golden.npz: TINY, make_weights(TINY, GOLDEN_SEED), clip(rows, 128, rows)
GOLDEN_SEED = 1


def pos_table(tmax: int, hidden: int) -> np.ndarray:
    """f32 [2 * tmax - 1][hidden], row p for d = p - (tmax - 1): inv_freq_k = f32(1 / 10000^(2k / H)) formed in double, arg the one
    f32 product f32(d) * inv_freq_k, sin / cos of double(arg) rounded to f32 into the even / odd columns."""
    k = np.arange(hidden // 2, dtype=np.float64)
    inv = (1.0 / np.power(10000.0, 2.0 * k / hidden)).astype(np.float32)
    d = np.arange(-(tmax - 1), tmax, dtype=np.float32)
    arg = (d[:, None] * inv[None, :]).astype(np.float32).astype(np.float64)
    out = np.empty((2 * tmax - 1, hidden), np.float32)
    out[:, 0::2] = np.sin(arg).astype(np.float32)
    out[:, 1::2] = np.cos(arg).astype(np.float32)
    return out


def rel_shift_direct(full: torch.Tensor) -> torch.Tensor:
    """full [heads][T][2T - 1] with column p for d = T - 1 - p (the library's order) -> [heads][T][T], entry (i, j) the one for d = i - j"""
    t = full.shape[1]
    i = torch.arange(t)[:, None]
    j = torch.arange(t)[None, :]
    return full[:, i, (t - 1) - (i - j)]


def rel_shift_pad(full: torch.Tensor) -> torch.Tensor:
    """the library's pad-and-reshape form of the same"""
    h, t, p = full.shape
    x = nn.functional.pad(full, pad=(1, 0)).view(h, -1, t)
    return x[:, 1:].view(h, t, p)[..., :t]


class Subsampling(nn.Module):
    def __init__(self, c: Config):
        super().__init__()
        ch = c.sub_channels
        self.layers = nn.ModuleList([nn.Conv2d(1, ch, 3, stride=2, padding=1), nn.ReLU()])
        for _ in range(2):
            self.layers.append(nn.Conv2d(ch, ch, 3, stride=2, padding=1, groups=ch))
            self.layers.append(nn.Conv2d(ch, ch, 1))
            self.layers.append(nn.ReLU())
        self.linear = nn.Linear(ch * (c.mel_bins // 8), c.hidden)

    def forward(self, x):      # [T][M]
        h = x[None, None]
        for layer in self.layers:
            h = layer(h)
        h = h.transpose(1, 2).reshape(1, h.shape[2], -1)      # [1][T'][C * M / 8], index c * M / 8 + f
        return self.linear(h)[0]


class FeedForward(nn.Module):
    def __init__(self, c: Config):
        super().__init__()
        self.linear1 = nn.Linear(c.hidden, c.ffn, bias=bool(c.attention_bias))
        self.linear2 = nn.Linear(c.ffn, c.hidden, bias=bool(c.attention_bias))

    def forward(self, x):
        return self.linear2(nn.functional.silu(self.linear1(x)))


class Attention(nn.Module):
    def __init__(self, c: Config):
        super().__init__()
        self.heads = c.heads
        self.bias_u = nn.Parameter(torch.zeros(c.heads, HEAD))
        self.bias_v = nn.Parameter(torch.zeros(c.heads, HEAD))
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            setattr(self, name, nn.Linear(c.hidden, c.hidden, bias=bool(c.attention_bias)))
        self.relative_k_proj = nn.Linear(c.hidden, c.hidden, bias=False)

    def forward(self, x, pos):      # x [T][H], pos [2T - 1][H] for d = -(T - 1) ... T - 1
        t = x.shape[0]
        split = lambda y: y.view(y.shape[0], self.heads, HEAD).transpose(0, 1)      # -> [heads][.][128]
        q, k, v = split(self.q_proj(x)), split(self.k_proj(x)), split(self.v_proj(x))
        r = split(self.relative_k_proj(pos.flip(0)))      # the library's order: d descending
        scale = HEAD ** -0.5
        bd = rel_shift_direct((q + self.bias_v[:, None]) @ r.transpose(1, 2)) * scale
        ac = ((q + self.bias_u[:, None]) @ k.transpose(1, 2)) * scale
        w = torch.softmax(ac + bd, dim=-1)
        return self.o_proj((w @ v).transpose(0, 1).reshape(t, -1))


class ConvModule(nn.Module):
    def __init__(self, c: Config):
        super().__init__()
        b = bool(c.convolution_bias)
        self.pointwise_conv1 = nn.Conv1d(c.hidden, 2 * c.hidden, 1, bias=b)
        self.depthwise_conv = nn.Conv1d(c.hidden, c.hidden, c.conv_kernel, padding=(c.conv_kernel - 1) // 2, groups=c.hidden, bias=b)
        self.norm = nn.BatchNorm1d(c.hidden)
        self.pointwise_conv2 = nn.Conv1d(c.hidden, c.hidden, 1, bias=b)

    def forward(self, x):      # [T][H]
        h = nn.functional.glu(self.pointwise_conv1(x.t()[None]), dim=1)
        h = nn.functional.silu(self.norm(self.depthwise_conv(h)))
        return self.pointwise_conv2(h)[0].t()


class Block(nn.Module):
    def __init__(self, c: Config):
        super().__init__()
        self.feed_forward1 = FeedForward(c)
        self.self_attn = Attention(c)
        self.conv = ConvModule(c)
        self.feed_forward2 = FeedForward(c)
        for name in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            setattr(self, name, nn.LayerNorm(c.hidden))

    def forward(self, x, pos):
        x = x + 0.5 * self.feed_forward1(self.norm_feed_forward1(x))
        x = x + self.self_attn(self.norm_self_att(x), pos)
        x = x + self.conv(self.norm_conv(x))
        x = x + 0.5 * self.feed_forward2(self.norm_feed_forward2(x))
        return self.norm_out(x)


class EncoderModules(nn.Module):
    def __init__(self, c: Config):
        super().__init__()
        self.cfg = c
        self.subsampling = Subsampling(c)
        self.layers = nn.ModuleList([Block(c) for _ in range(c.layers)])


def tensor_list(c: Config):
    """(key, element count) in state-dict order without num_batches_tracked"""
    return [(k, int(v.numel())) for k, v in EncoderModules(c).state_dict().items() if not k.endswith("num_batches_tracked")]


def make_weights(c: Config, seed: int) -> dict:
    """seeded f32 weights by state-dict key: matrices / sqrt(fan-in), biases and bias_u / bias_v about 0.1, LayerNorm and BatchNorm
    weights about 1, running_var in 0.5 ... 1.5"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, v in EncoderModules(c).state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        shape = tuple(v.shape)
        leaf = k.rsplit(".", 1)[-1]
        is_norm = ".norm" in k      # conv.norm and the five norm_* LayerNorms
        if leaf == "running_var":
            a = rng.uniform(0.5, 1.5, shape)
        elif leaf in ("bias", "bias_u", "bias_v", "running_mean"):
            a = 0.1 * rng.standard_normal(shape)
        elif is_norm:
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / math.sqrt(int(np.prod(shape[1:])))
        out[k] = a.astype(np.float32)
    return out


class Encoder:
    """The encoder with `weights` (make_weights' form) in `dtype`; forward takes clips [T][M] one at a time."""

    def __init__(self, c: Config, weights: dict, dtype=torch.float64):
        self.cfg, self.dtype = c, dtype
        self.net = EncoderModules(c).to(dtype).eval()
        sd = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dtype) for k, v in weights.items()}
        missing = self.net.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing

    @torch.no_grad()
    def forward(self, clips):
        """-> per clip (out [T'][H], sub [T'][H], [tap of every block]) as numpy arrays of the oracle's precision"""
        res = []
        for x in clips:
            x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.dtype)
            h = self.net.subsampling(x)
            if self.cfg.scale_input:
                h = h * math.sqrt(self.cfg.hidden)
            sub = h
            pos = torch.from_numpy(pos_table(h.shape[0], self.cfg.hidden)).to(self.dtype)
            taps = []
            for blk in self.net.layers:
                h = blk(h, pos)
                taps.append(h.numpy().copy())
            res.append((h.numpy().copy(), sub.numpy().copy(), taps))
        return res

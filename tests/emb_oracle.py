"""Oracle of the speaker-embedding network (crispy_diar_emb_*, include/crispy_hip.h): WeSpeaker CAMPPlus ("CAM++") restated as
torch.nn modules on the CPU, constructible in float32 and in float64, and seeded weights for it.  [UPSTREAM-RECALL]: restated
from memory of wespeaker's campplus.py and pooling_layers.py; module and attribute names are chosen so that state_dict() gives
wespeaker's keys (815 float tensors, num_batches_tracked aside).

  head (FCM) on [1][80][T], frequency strided, time never: Conv2d(1, 32, 3x3) BN ReLU -> two layers of two BasicResBlocks
  (32 channels; block .0 strides frequency by 2 and has a 1x1 convolution + BN shortcut) -> Conv2d(32, 32, 3x3, stride (2, 1))
  BN ReLU -> [320][T], channel c * 10 + f.
  xvector on [320][T]: tdnn Conv1d(320, 128, 5, stride 2, pad 2) BN ReLU -> three dense blocks (12, 24, 16 layers of growth 32
  at dilation 1, 2, 2), each followed by a transit (BN ReLU Conv1d(C, C / 2, 1)) -> BN ReLU -> statistics pooling (mean,
  sqrt(unbiased variance + 1e-7)) -> Conv1d(1024, dim, 1) -> BatchNorm without affine terms.
  A dense layer: BN ReLU Conv1d(Cin, 128, 1) BN ReLU = h; y = Conv1d(128, 32, 3, dilation d, pad d)(h);
  ctx = mean_t(h) + segmean_100(h); out = y * sigmoid(Conv1d(64, 32, 1)(relu(Conv1d(128, 64, 1)(ctx)))); x = cat(x, out).

Every constant of the network is here, once.  The weights come from numpy.random.default_rng(seed), never from torch's
generator; the same dict goes into the oracle and into Diarizer.load_embedding."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

FEAT_DIM, EMBED_DIM = 80, 512
BN_EPS, POOL_EPS = 1e-5, 1e-7
SEG_LEN, CAM_REDUCTION = 100, 2
HEAD_CH, HEAD_OUT = 32, 320
INIT_CH, GROWTH, BN_CH = 128, 32, 128
BLOCKS = ((12, 1), (24, 2), (16, 2))      # (layers, dilation)
TDNN_TAPS, TDNN_STRIDE = 5, 2
N_TENSORS = 815


def emb_frames(rows: int) -> int:
    """positions after the stride-2 tdnn (0 without rows)"""
    return (rows - 1) // TDNN_STRIDE + 1 if rows >= 1 else 0


def seg_mean(h, seg_len: int = SEG_LEN):
    """h [..., T] -> the mean over consecutive segments of seg_len positions, broadcast back over the segment; the last, shorter
    segment is averaged over its own count"""
    t = h.shape[-1]
    seg = F.avg_pool1d(h, seg_len, seg_len, ceil_mode=True)
    return seg.unsqueeze(-1).expand(*seg.shape, seg_len).reshape(*seg.shape[:-1], -1)[..., :t]


def nonlinear(c, affine=True, relu=True):
    mods = OrderedDict(batchnorm=torch.nn.BatchNorm1d(c, eps=BN_EPS, affine=affine))
    if relu:
        mods["relu"] = torch.nn.ReLU()
    return torch.nn.Sequential(mods)


class BasicResBlock(torch.nn.Module):
    def __init__(self, c, stride):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(c, c, 3, stride=(stride, 1), padding=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(c, eps=BN_EPS)
        self.conv2 = torch.nn.Conv2d(c, c, 3, stride=1, padding=1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(c, eps=BN_EPS)
        self.shortcut = torch.nn.Sequential()
        if stride != 1:
            self.shortcut = torch.nn.Sequential(torch.nn.Conv2d(c, c, 1, stride=(stride, 1), bias=False), torch.nn.BatchNorm2d(c, eps=BN_EPS))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return F.relu(out + self.shortcut(x))


class FCM(torch.nn.Module):
    def __init__(self):
        super().__init__()
        c = HEAD_CH
        self.conv1 = torch.nn.Conv2d(1, c, 3, stride=1, padding=1, bias=False)
        self.bn1 = torch.nn.BatchNorm2d(c, eps=BN_EPS)
        self.layer1 = torch.nn.Sequential(BasicResBlock(c, 2), BasicResBlock(c, 1))
        self.layer2 = torch.nn.Sequential(BasicResBlock(c, 2), BasicResBlock(c, 1))
        self.conv2 = torch.nn.Conv2d(c, c, 3, stride=(2, 1), padding=1, bias=False)
        self.bn2 = torch.nn.BatchNorm2d(c, eps=BN_EPS)

    def forward(self, x):      # [1][80][T]
        out = F.relu(self.bn1(self.conv1(x.unsqueeze(1))))
        out = self.layer2(self.layer1(out))
        out = F.relu(self.bn2(self.conv2(out)))
        return out.reshape(out.shape[0], out.shape[1] * out.shape[2], out.shape[3])


class TDNNLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = torch.nn.Conv1d(HEAD_OUT, INIT_CH, TDNN_TAPS, stride=TDNN_STRIDE, padding=TDNN_TAPS // 2, bias=False)
        self.nonlinear = nonlinear(INIT_CH)

    def forward(self, x):
        return self.nonlinear(self.linear(x))


class CAMLayer(torch.nn.Module):
    def __init__(self, dilation):
        super().__init__()
        self.linear_local = torch.nn.Conv1d(BN_CH, GROWTH, 3, padding=dilation, dilation=dilation, bias=False)
        self.linear1 = torch.nn.Conv1d(BN_CH, BN_CH // CAM_REDUCTION, 1)
        self.linear2 = torch.nn.Conv1d(BN_CH // CAM_REDUCTION, GROWTH, 1)

    def forward(self, h):
        y = self.linear_local(h)
        ctx = h.mean(-1, keepdim=True) + seg_mean(h)
        return y * torch.sigmoid(self.linear2(F.relu(self.linear1(ctx))))


class CAMDenseTDNNLayer(torch.nn.Module):
    def __init__(self, c_in, dilation):
        super().__init__()
        self.nonlinear1 = nonlinear(c_in)
        self.linear1 = torch.nn.Conv1d(c_in, BN_CH, 1, bias=False)
        self.nonlinear2 = nonlinear(BN_CH)
        self.cam_layer = CAMLayer(dilation)

    def forward(self, x):
        return self.cam_layer(self.nonlinear2(self.linear1(self.nonlinear1(x))))


class CAMDenseTDNNBlock(torch.nn.ModuleList):
    def __init__(self, n_layers, c_in, dilation):
        super().__init__()
        for i in range(n_layers):
            self.add_module(f"tdnnd{i + 1}", CAMDenseTDNNLayer(c_in + i * GROWTH, dilation))

    def forward(self, x):
        for layer in self:
            x = torch.cat([x, layer(x)], dim=1)
        return x


class TransitLayer(torch.nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.nonlinear = nonlinear(c_in)
        self.linear = torch.nn.Conv1d(c_in, c_out, 1, bias=False)

    def forward(self, x):
        return self.linear(self.nonlinear(x))


class DenseLayer(torch.nn.Module):
    def __init__(self, c_in, c_out):
        super().__init__()
        self.linear = torch.nn.Conv1d(c_in, c_out, 1, bias=False)
        self.nonlinear = nonlinear(c_out, affine=False, relu=False)

    def forward(self, x):      # [1][c_in]
        return self.nonlinear(self.linear(x.unsqueeze(-1)).squeeze(-1))


class CAMPPlusModules(torch.nn.Module):
    def __init__(self, dim=EMBED_DIM):
        super().__init__()
        self.head = FCM()
        xv = OrderedDict(tdnn=TDNNLayer())
        c = INIT_CH
        for i, (n_layers, dilation) in enumerate(BLOCKS):
            xv[f"block{i + 1}"] = CAMDenseTDNNBlock(n_layers, c, dilation)
            c += n_layers * GROWTH
            xv[f"transit{i + 1}"] = TransitLayer(c, c // 2)
            c //= 2
        xv["out_nonlinear"] = nonlinear(c)
        self.xvector = torch.nn.Sequential(xv)
        self.xvector.add_module("dense", DenseLayer(2 * c, dim))


def tensor_shapes(dim=EMBED_DIM) -> "OrderedDict[str, tuple]":
    """state-dict key -> shape of every float tensor, in state-dict order"""
    sd = CAMPPlusModules(dim).state_dict()
    return OrderedDict((k, tuple(v.shape)) for k, v in sd.items() if not k.endswith("num_batches_tracked"))


def make_weights(seed: int, dim: int = EMBED_DIM) -> dict:
    """Every tensor from numpy.random.default_rng(seed), in state-dict order: convolution weights uniform with bound
    sqrt(6 / fan_in), the gate's biases in +-0.1, BatchNorm weight in 0.8 ... 1.2, bias and running_mean in +-0.2, running_var
    in 0.5 ... 1.5 (with 1 / sqrt(fan) the activations collapse over 60 layers)."""
    rng = np.random.default_rng(seed)
    w = {}
    for key, shape in tensor_shapes(dim).items():
        if len(shape) >= 3:
            b = np.sqrt(6.0 / np.prod(shape[1:]))
            v = rng.uniform(-b, b, shape)
        elif key.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif key.endswith("running_mean"):
            v = rng.uniform(-0.2, 0.2, shape)
        elif "cam_layer" in key:      # the two biases of the gate
            v = rng.uniform(-0.1, 0.1, shape)
        elif key.endswith("weight"):
            v = rng.uniform(0.8, 1.2, shape)
        else:
            v = rng.uniform(-0.2, 0.2, shape)
        w[key] = v.astype(np.float32)
    return w


class CAMPPlus(CAMPPlusModules):
    def __init__(self, weights: dict, dtype=torch.float64):
        dim = int(np.asarray(weights["xvector.dense.linear.weight"]).shape[0])
        super().__init__(dim)
        self.to(dtype)
        sd = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dtype) for k, v in weights.items() if not k.endswith("num_batches_tracked")}
        missing, unexpected = self.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
        self.dtype, self.dim = dtype, dim
        self.eval()

    @torch.no_grad()
    def forward(self, feats_list):
        """list of [T][80] -> per chunk (embedding [dim], head [T][320], out_nonlinear [T2][512], statistics [1024]) as numpy"""
        out = []
        xv = self.xvector
        for feats in feats_list:
            x = torch.as_tensor(np.asarray(feats, np.float32)).to(self.dtype).t().unsqueeze(0)      # [1][80][T]
            head = self.head(x)
            y = xv.tdnn(head)
            for i in range(len(BLOCKS)):
                y = getattr(xv, f"transit{i + 1}")(getattr(xv, f"block{i + 1}")(y))
            y = xv.out_nonlinear(y)
            stats = torch.cat([y.mean(-1), torch.sqrt(y.var(-1, unbiased=True) + POOL_EPS)], dim=-1)
            emb = xv.dense(stats)
            out.append((emb[0].numpy(), head[0].t().contiguous().numpy(), y[0].t().contiguous().numpy(), stats[0].numpy()))
        return out

    def embed(self, feats):
        return self.forward([feats])[0][0]

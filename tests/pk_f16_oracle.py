"""Oracle of the Parakeet encoder's precision mode 1 (crispy_pk_set_precision, include/crispy_hip.h): tests/pk_oracle.py's network
with f16 operands in every product that the library's GEMM performs.

Definition.  In subsampling.linear, the four feed-forward linears, q_proj, k_proj, v_proj, relative_k_proj (on the position
table), o_proj, pointwise_conv1 and pointwise_conv2, both operands -- the weight and the input -- are rounded once to IEEE
binary16: round to nearest even, subnormals kept, overflow to infinity, exactly torch.Tensor.to(torch.float16).  The products
and sums are those of the oracle's own precision (float64: exact; float32: the yardstick for f32 sums).  Everything else is
pk_oracle's arithmetic untouched: the subsampling Conv2d layers, LayerNorm, the attention products and soft-max, the depthwise
convolution with its BatchNorm, the biases, SiLU, GLU and the residual stream.

The rounding is a weight replaced at construction and a forward pre-hook on the module's input; with `hooks` off the class is
pk_oracle.Encoder bit for bit.  tests/test_pk_f16_oracle.py pins this file."""
import numpy as np
import torch
from torch import nn

from tests import pk_oracle as PO


def round_f16(x: torch.Tensor) -> torch.Tensor:
    """x rounded once to binary16, in x's own dtype"""
    return x.to(torch.float16).to(x.dtype)


def is_gemm(m: nn.Module) -> bool:
    """the modules the library runs through its GEMM: every Linear and every Conv1d of kernel size 1"""
    return isinstance(m, nn.Linear) or (isinstance(m, nn.Conv1d) and tuple(m.kernel_size) == (1,))


def gemm_names(c: PO.Config):
    """the state-dict prefixes of the hooked modules, in module order"""
    return [name for name, m in PO.EncoderModules(c).named_modules() if is_gemm(m)]


class Encoder(PO.Encoder):
    """pk_oracle.Encoder with f16 operands in the GEMM modules; `hooks` False leaves it as pk_oracle.Encoder."""

    def __init__(self, c: PO.Config, weights: dict, dtype=torch.float64, hooks: bool = True):
        super().__init__(c, weights, dtype)
        self.hooked = []
        if not hooks:
            return
        for name, m in self.net.named_modules():
            if not is_gemm(m):
                continue
            with torch.no_grad():
                m.weight.copy_(round_f16(m.weight))
            m.register_forward_pre_hook(lambda _m, args: (round_f16(args[0]),) + tuple(args[1:]))
            self.hooked.append(name)


def linear_f16(x: np.ndarray, w: np.ndarray, b=None, dtype=np.float64) -> np.ndarray:
    """the definition written out for one Linear: x [M][K], w [N][K] (state-dict layout), b [N] -> [M][N] in `dtype`"""
    xr = x.astype(np.float32).astype(np.float16).astype(dtype)
    wr = w.astype(np.float32).astype(np.float16).astype(dtype)
    y = xr @ wr.T
    return y if b is None else y + b.astype(dtype)

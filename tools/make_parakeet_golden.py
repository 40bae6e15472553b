#!/usr/bin/env python3
"""Writes tests/golden/parakeet_enc_golden.npz: the float64 forward of transformers' ParakeetEncoder at tests/pk_oracle.py's TINY
config on the clips of GOLDEN_ROWS, each alone with no mask.  Outputs only: the weights regenerate from the seed
(pk_oracle.make_weights(TINY, GOLDEN_SEED)) and the clips from theirs (pk_oracle.clip(rows, 128, rows)).  Needs transformers with
transformers.models.parakeet; tests/test_pk_oracle.py asserts the file without it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pk_oracle as PO  # noqa: E402


def library_encoder(cfg, weights):
    from transformers.models.parakeet import ParakeetEncoder, ParakeetEncoderConfig
    hc = ParakeetEncoderConfig(hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, intermediate_size=cfg.ffn,
                               conv_kernel_size=cfg.conv_kernel, num_mel_bins=cfg.mel_bins, subsampling_conv_channels=cfg.sub_channels,
                               attention_bias=bool(cfg.attention_bias), convolution_bias=bool(cfg.convolution_bias),
                               scale_input=bool(cfg.scale_input))
    net = ParakeetEncoder(hc).double().eval()
    missing = net.load_state_dict({k: torch.from_numpy(v).double() for k, v in weights.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    assert [k for k in net.state_dict() if not k.endswith("num_batches_tracked")] == list(weights)
    return net


def library_forward(net, x):
    with torch.no_grad():
        return net(torch.from_numpy(x).double()[None]).last_hidden_state[0].numpy()


def main():
    net = library_encoder(PO.TINY, PO.make_weights(PO.TINY, PO.GOLDEN_SEED))
    out = {f"rows{r}": library_forward(net, PO.clip(r, PO.TINY.mel_bins, r)) for r in PO.GOLDEN_ROWS}
    path = os.path.join(ROOT, "tests", "golden", "parakeet_enc_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

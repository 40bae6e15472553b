#!/usr/bin/env python3
"""Writes tests/golden/parakeet_tdt_golden.npz: transformers' ParakeetForTDT in float64 at tests/pk_tdt_oracle.py's TINY_TDT config
on the clips of GOLDEN_FRAMES -- frames in, and out the greedy path (token, frame, duration per step) with the logits of its first
and last steps.  The path is driven step by step through ParakeetForTDT.forward with a ParakeetRNNTDecoderCache and the update
rule of ParakeetTDTGenerationMixin, so that the frames go in as they are.  The weights regenerate from their seed
(pk_tdt_oracle.make_tdt_weights(TINY_TDT, GOLDEN_SEED, **MIX)).  Needs transformers with transformers.models.parakeet;
tests/test_pk_tdt_oracle.py asserts the file without it.

`--search` looks for the weight seeds of the tests' fixture: the lowest seeds whose float64 paths have the coverage and the
top-two gaps the tests assert (tests/pk_tdt_oracle.py: FIXTURE), with a margin of four on the gaps; `--search-catalog` does the same
for the catalog-width test's seed."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pk_oracle as PO  # noqa: E402
from tests import pk_tdt_oracle as TO  # noqa: E402

LOGIT_ROWS = 3      # of each end of a path


def library_model(cfg, weights, dtype=torch.float64, encoder_cfg=PO.TINY, encoder_weights=None, duration_shift=0.0):
    """ParakeetForTDT with `weights` (and a seeded encoder); duration_shift is subtracted from the duration biases, which changes no
    decision of the loop and keeps generate()'s own arg-max over all V + n_d logits inside the vocabulary"""
    from transformers.models.parakeet import ParakeetEncoderConfig, ParakeetForTDT, ParakeetTDTConfig
    ec = ParakeetEncoderConfig(hidden_size=encoder_cfg.hidden, num_hidden_layers=encoder_cfg.layers, num_attention_heads=encoder_cfg.heads,
                               intermediate_size=encoder_cfg.ffn, conv_kernel_size=encoder_cfg.conv_kernel, num_mel_bins=encoder_cfg.mel_bins,
                               subsampling_conv_channels=encoder_cfg.sub_channels, attention_bias=bool(encoder_cfg.attention_bias),
                               convolution_bias=bool(encoder_cfg.convolution_bias), scale_input=bool(encoder_cfg.scale_input))
    hc = ParakeetTDTConfig(vocab_size=cfg.vocab, decoder_hidden_size=cfg.decoder_hidden, num_decoder_layers=cfg.decoder_layers,
                           max_symbols_per_step=cfg.max_symbols_per_step, encoder_config=ec, pad_token_id=0, blank_token_id=cfg.blank,
                           durations=list(cfg.durations))
    net = ParakeetForTDT(hc).to(dtype).eval()
    sd = {k: torch.from_numpy(np.array(v, np.float32)).to(dtype) for k, v in weights.items()}
    sd["joint.head.bias"][cfg.vocab:] -= duration_shift
    if encoder_weights is None:
        encoder_weights = PO.make_weights(encoder_cfg, 1)
    sd.update({"encoder." + k: torch.from_numpy(v).to(dtype) for k, v in encoder_weights.items()})
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    mine = [k for k in net.state_dict() if k.startswith(("encoder_projector.", "decoder.", "joint."))]
    assert mine == list(weights), (mine, list(weights))      # the keys and their order
    net.generation_config.decoder_start_token_id = cfg.blank
    return net


@torch.no_grad()
def library_path(net, cfg, frames):
    """(steps int32 [n][3], logits [n][V + n_d]) of the library's modules on frames [T'][H], one forward per step"""
    from transformers.models.parakeet.generation_parakeet import ParakeetRNNTDecoderCache
    from transformers.models.parakeet.modeling_parakeet import ParakeetEncoderModelOutput
    dtype = next(net.parameters()).dtype
    n_frames = frames.shape[0]
    steps, rows = [], []
    if n_frames == 0:
        return np.zeros((0, 3), np.int32), np.zeros((0, cfg.width))
    p = net.encoder_projector(torch.from_numpy(frames).to(dtype))
    cache = ParakeetRNNTDecoderCache(net.config)
    token, t = cfg.blank, 0
    for _ in range(TO.max_steps(cfg, n_frames)):
        out = net(encoder_outputs=ParakeetEncoderModelOutput(pooler_output=p[None, t, None]), decoder_input_ids=torch.tensor([[token]]),
                  decoder_cache=cache)
        logits = out.logits[0, -1]
        token = int(logits[:cfg.vocab].argmax())
        d = int(cfg.durations[int(logits[cfg.vocab:].argmax())])
        if token == cfg.blank and d == 0:
            d = 1
        steps.append((token, t, d))
        rows.append(logits.numpy().copy())
        t += d
        if t >= n_frames:
            break
    return np.asarray(steps, np.int32).reshape(-1, 3), np.asarray(rows)


def fixture_report(seeds=None):
    """coverage and the smallest (gap / float32 error) over the fixture's clips, per weight set"""
    cover, ratio = [], {}
    for name, (kw, seed) in TO.FIXTURE_SETS.items():
        seed = seeds.get(name, seed) if seeds else seed
        w = TO.make_tdt_weights(TO.TINY_TDT, seed, **kw)
        o64, o32 = TO.Tdt(TO.TINY_TDT, w, torch.float64), TO.Tdt(TO.TINY_TDT, w, torch.float32)
        worst = float("inf")
        for which, n_frames, fseed in TO.FIXTURE_CLIPS:
            if which != name:
                continue
            e = TO.frames(n_frames, TO.TINY_TDT.hidden, fseed)
            steps, logits = o64.decode(e, with_logits=True)
            cover.append((n_frames, steps, logits))
            if len(steps):
                err = float(np.abs(o32.logits_along(e, steps) - logits).max())
                worst = min(worst, min(TO.top_two_gaps(logits, TO.TINY_TDT.vocab)) / err)
        ratio[name] = worst
    return TO.coverage(TO.TINY_TDT, cover), ratio, max(len(s) for _t, s, _l in cover)


def search():
    chosen = {}
    for name in TO.FIXTURE_SETS:
        for seed in range(1, 200):
            cov, ratio, longest = fixture_report(dict(chosen, **{name: seed}))
            ok = ratio[name] >= 4 * TO.GAP_FACTOR
            if name == "mix":      # the set that carries the variety; the others are what their names say at any seed
                ok = ok and cov["durations"] >= set(TO.TINY_TDT.durations) and cov["forced_blanks"] >= 1 and cov["overshoot"] >= 2 and longest <= 700
            if ok:
                chosen[name] = seed
                print(name, "seed", seed, "gap / float32 error", f"{ratio[name]:.1f}")
                break
    print(chosen, fixture_report(chosen))


def search_catalog():
    cfg = TO.CATALOG_TDT
    for seed in range(1, 50):
        w = TO.make_tdt_weights(cfg, seed, **TO.MIX)
        o64, o32 = TO.Tdt(cfg, w, torch.float64), TO.Tdt(cfg, w, torch.float32)
        worst, lengths = float("inf"), []
        for t in TO.CATALOG_FRAMES:
            e = TO.frames(t, cfg.hidden, 700 + t)
            steps, logits = o64.decode(e, with_logits=True)
            err = float(np.abs(o32.logits_along(e, steps) - logits).max())
            worst = min(worst, min(TO.top_two_gaps(logits, cfg.vocab)) / err)
            lengths.append(len(steps))
        print("catalog seed", seed, "gap / float32 error", f"{worst:.1f}", "steps", lengths)
        if worst >= 4 * TO.GAP_FACTOR and max(lengths) <= 200:
            return seed


def main():
    if "--search" in sys.argv:
        return search()
    if "--search-catalog" in sys.argv:
        return search_catalog()
    cfg = TO.TINY_TDT
    net = library_model(cfg, TO.make_tdt_weights(cfg, TO.GOLDEN_SEED, **TO.MIX))
    out = {}
    for t in TO.GOLDEN_FRAMES:
        e = TO.frames(t, cfg.hidden, t)
        steps, logits = library_path(net, cfg, e)
        out[f"frames{t}"] = e
        out[f"steps{t}"] = steps
        out[f"first{t}"] = logits[:LOGIT_ROWS].astype(np.float64)
        out[f"last{t}"] = logits[-LOGIT_ROWS:].astype(np.float64)
    path = os.path.join(ROOT, "tests", "golden", "parakeet_tdt_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

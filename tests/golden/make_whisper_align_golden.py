"""Generates tests/golden/whisper_tiny_align_golden.npz: the word-alignment matrix as HuggingFace transformers computes it
(`WhisperForConditionalGeneration(output_attentions=True)`, teacher-forced, then the steps of its
`_extract_token_timestamps`: soft-maxed cross-attention of the alignment heads cropped to num_frames // 2, population
std / mean over the tokens, `_median_filter` of width 7, the mean over the heads, `_dynamic_time_warping` on minus the
rows of <|notimestamps|> and the text) on the seeded synthetic Whisper-tiny weights -- the reference for
tests/test_gpu_align_shapes.py that does not come from tests/align_oracle.py.  Two full 30 s clips (the crop is then
the whole 1500 keys, where HF's crop-after-soft-max and openai's crop-before agree), 40 text tokens each.

    python tests/golden/make_whisper_align_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from transformers import WhisperConfig, WhisperFeatureExtractor, WhisperForConditionalGeneration  # noqa: E402
from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter  # noqa: E402

from crispy_amd import synth_audio  # noqa: E402
from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights  # noqa: E402
from hf_names import hf_name  # noqa: E402

HEADS = [(2, 2), (3, 0), (3, 2), (3, 3), (3, 4), (3, 5)]
hp = HParams.tiny()
W = synthetic_whisper_weights(hp, 0)
cfg = WhisperConfig()
cfg._attn_implementation = "eager"                   # the attention probabilities are returned by the eager form only
model = WhisperForConditionalGeneration(cfg).eval()
sd = model.state_dict()
for n, v in W.items():
    sd[hf_name(n)].copy_(torch.from_numpy(v))
sd["proj_out.weight"].copy_(torch.from_numpy(W["decoder.token_embedding.weight"]))
model.load_state_dict(sd)

sot = [50258, 50259, 50359]                          # sot, <|en|>, <|transcribe|>
out = {}
for ci, seed in enumerate((11, 12)):
    x = synth_audio.clip16k_np(seed, 480000)
    mel = WhisperFeatureExtractor()(x, sampling_rate=16000, return_tensors="pt")["input_features"]
    text = np.random.default_rng(seed).integers(0, 50257, 40).tolist()
    toks = sot + [50363] + text + [50257]
    with torch.no_grad():
        enc = model.model.encoder(mel).last_hidden_state
        o = model(encoder_outputs=(enc,), decoder_input_ids=torch.tensor([toks]), output_attentions=True)
    w = torch.stack([o.cross_attentions[l][0, h] for l, h in HEADS])          # [heads][rows][1500], soft-maxed
    w = w[..., : 3000 // 2]
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    m = _median_filter((w - mean) / std, 7).mean(0)
    mx = m[len(sot):-1].double().numpy()
    ti, tj = _dynamic_time_warping(-mx)
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    out[f"c{ci}_clip"] = np.array([seed, 480000])
    out[f"c{ci}_tokens"] = np.array(toks, np.int32)
    out[f"c{ci}_probs"] = w[:, :, ::50].numpy().astype(np.float32)          # every 50th frame: [heads][rows][30]
    out[f"c{ci}_jump_idx"] = tj[jumps].astype(np.int32)
    out[f"c{ci}_path"] = np.stack([ti, tj]).astype(np.int16)
    if ci == 0:
        out["c0_matrix"] = mx.astype(np.float32)                            # the rows the DTW takes, [41][1500]
    print(ci, "probs max", float(w.max()), "matrix range", float(m.min()), float(m.max()), "jumps", tj[jumps][:10])
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "whisper_tiny_align_golden.npz"), heads=np.array(HEADS), **out)

"""Oracle of the audio context (crispy_asr_set_audio_ctx; whisper.cpp's whisper_full_params.audio_ctx [UPSTREAM-RECALL]):
the three encoders of oracle/whisper_oracle.py -- exact, f16 operands (precision mode 1), f16 operands + ggml's rounding
points inside the attention (mode 2) -- restated with the context n as a parameter.

With audio_ctx = n the encoder's input is mel frames [0, 2 n) of the window; conv1 (k3, p1) sees its own ZERO padding at
frame 2 n, not the frame that follows in the 3000-frame buffer; conv2 (k3, s2, p1) yields n rows, rows 0 .. n - 1 of the
positional embedding are added, every layer and ln_post run over n rows.  The decoder side needs nothing new:
WO.decoder_logits, WO.DecoderCache, WO.whisper_full and tests/confidence_oracle.token_logprobs take whatever encoder rows
they are given.

Every operation below is the one of WO.encoder_forward / WO.encoder_forward_f16 on the same shapes at n = 1500, so the
restatement equals them exactly there (tests/test_audio_ctx_oracle.py)."""
import numpy as np

from oracle import whisper_oracle as WO


def encoder_forward_ctx(weights, hp, mel, n, f16=False, attn16=False, noise=None):
    """mel [n_mels, >= 2 n] (the window's log-mel; frames from 2 n on are never read) -> [n, d] float64.
    noise (f16 only; `accumulation_noise_floor`): a function applied to every COMPUTED value in front of its f16 rounding --
    the activations and the argument of ggml's GELU table; weights and the log-mel are rounded as they are."""
    n = int(n)
    if not 1 <= n <= hp.n_audio_ctx:
        raise ValueError(f"audio context {n} outside 1 ... {hp.n_audio_ctx}")
    if attn16 and not f16:
        raise ValueError("attn16 is a variant of the f16-operand encoder")
    W = WO._f64(weights)
    hw, gelu = (WO._h, WO._gelu_ggml) if f16 else ((lambda a: a), WO._gelu)      # hw: a stored value (weight, log-mel) rounded
    h = hw                                                                        # h: a computed value rounded
    if noise is not None:
        if not f16:
            raise ValueError("noise goes in front of the f16 roundings")
        h = lambda a: WO._h(noise(a))
        gelu = lambda a: WO._gelu_ggml(noise(a))
    M = 2 * n
    x = hw(mel[:, :M]) if f16 else mel[:, :M].astype(np.float64)
    xp = np.pad(x, ((0, 0), (1, 1)))                      # the convolution's own padding: a zero at frame 2 n
    w1 = hw(W["encoder.conv1.weight"])
    h1 = sum(w1[:, :, k] @ xp[:, k:k + M] for k in range(3)) + W["encoder.conv1.bias"][:, None]
    h1 = h(gelu(h1))
    hp1 = np.pad(h1, ((0, 0), (1, 1)))
    w2 = hw(W["encoder.conv2.weight"])
    h2 = sum(w2[:, :, k] @ hp1[:, k:k + M:2][:, :n] for k in range(3)) + W["encoder.conv2.bias"][:, None]
    x = gelu(h2).T + W["encoder.positional_embedding"][:n]
    H = hp.n_audio_head
    for i in range(hp.n_audio_layer):
        p = f"encoder.blocks.{i}"
        if not f16:
            xn = WO._ln(x, W[p + ".attn_ln.weight"], W[p + ".attn_ln.bias"])
            x = x + WO._mha(xn, xn, W, p + ".attn", H)
            xn = WO._ln(x, W[p + ".mlp_ln.weight"], W[p + ".mlp_ln.bias"])
            x = x + WO._gelu(xn @ W[p + ".mlp.0.weight"].T + W[p + ".mlp.0.bias"]) @ W[p + ".mlp.2.weight"].T + W[p + ".mlp.2.bias"]
            continue
        # the rounding points of WO.encoder_forward_f16, in its order
        xn = h(WO._ln(x, W[p + ".attn_ln.weight"], W[p + ".attn_ln.bias"]))
        q = h(xn @ hw(W[p + ".attn.query.weight"]).T + W[p + ".attn.query.bias"])
        k = h(xn @ hw(W[p + ".attn.key.weight"]).T)
        v = h(xn @ hw(W[p + ".attn.value.weight"]).T + W[p + ".attn.value.bias"])
        att = np.empty_like(q)
        dh = q.shape[1] // H
        for hh in range(H):
            sl = slice(hh * dh, (hh + 1) * dh)
            t = (q[:, sl] @ k[:, sl].T) / np.sqrt(dh) * np.log2(np.e)
            if attn16:
                pe = np.exp2(t - t.max(-1, keepdims=True))
                att[:, sl] = h(pe / pe.sum(-1, keepdims=True)) @ v[:, sl]
                continue
            pe = np.exp2(t - np.ceil(t.max(-1, keepdims=True)))
            att[:, sl] = (h(pe) @ v[:, sl]) / pe.sum(-1, keepdims=True)
        x = x + h(att) @ hw(W[p + ".attn.out.weight"]).T + W[p + ".attn.out.bias"]
        xn = h(WO._ln(x, W[p + ".mlp_ln.weight"], W[p + ".mlp_ln.bias"]))
        hid = h(gelu(xn @ hw(W[p + ".mlp.0.weight"]).T + W[p + ".mlp.0.bias"]))
        x = x + hid @ hw(W[p + ".mlp.2.weight"]).T + W[p + ".mlp.2.bias"]
    return WO._ln(x, W["encoder.ln_post.weight"], W["encoder.ln_post.bias"])


def accumulation_noise_floor(weights, hp, mel, n, attn16=False, rel=3e-7, seeds=5):
    """What agreement with encoder_forward_ctx(f16=True) an f32 pipeline can reach at context n -- the simulation
    tests/test_gpu_whisper.py::test_f16_operand_mode_matches_the_f16_operand_oracle describes, on the oracle itself:
    `rel` relative noise (f32 accumulation in another order) in front of every f16 rounding of a computed value moves a
    few values per thousand across an f16 boundary, a full 2^-11 step each.  Returns (max, rms) of the deviation from the
    noise-free oracle as shares of its peak, the worst of `seeds` noise seeds each."""
    ref = encoder_forward_ctx(weights, hp, mel, n, f16=True, attn16=attn16)
    peak = np.abs(ref).max()
    worst_max = worst_rms = 0.0
    for seed in range(seeds):
        rng = np.random.default_rng(seed)
        got = encoder_forward_ctx(weights, hp, mel, n, f16=True, attn16=attn16,
                                  noise=lambda a: a * (1.0 + rel * rng.standard_normal(np.shape(a))))
        worst_max = max(worst_max, float(np.abs(got - ref).max() / peak))
        worst_rms = max(worst_rms, float(np.sqrt(np.mean((got - ref) ** 2)) / peak))
    return worst_max, worst_rms

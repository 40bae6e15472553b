"""The audio-context oracle (tests/audio_ctx_oracle.py) against oracle/whisper_oracle.py, and the two new entry points on
the host side (no GPU): at the full context the restatement IS the three encoders; below it, it is not a slice of them;
the zero at frame 2 n is the convolution's own padding; header, Python binding and Rust crate agree on the two names."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "crispy_hip.h")
NAMES = ("crispy_asr_set_audio_ctx", "crispy_asr_audio_ctx")


@pytest.fixture(scope="module")
def case():
    """Random-init tiny, a log-mel-like window (values in [-1, 1.5] as whisper's normalisation leaves them), and the exact
    full-context encoder -- computed once, shared, never written to."""
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    from oracle import whisper_oracle as WO
    hp = HParams.tiny()
    W = synthetic_whisper_weights(hp, 0)
    rng = np.random.default_rng(11)
    mel = (rng.random((hp.n_mels, 3000)) * 2.5 - 1.0).astype(np.float32)
    full = WO.encoder_forward(W, hp, mel)
    full.setflags(write=False)
    return hp, W, mel, full


def test_at_the_full_context_the_restatement_is_the_exact_encoder(case):
    from tests.audio_ctx_oracle import encoder_forward_ctx
    hp, W, mel, full = case
    assert np.array_equal(encoder_forward_ctx(W, hp, mel, hp.n_audio_ctx), full)


@pytest.mark.parametrize("attn16", [False, True])
def test_at_the_full_context_the_restatement_is_the_f16_operand_encoder(case, attn16):
    from oracle import whisper_oracle as WO
    from tests.audio_ctx_oracle import encoder_forward_ctx
    hp, W, mel, _ = case
    assert np.array_equal(encoder_forward_ctx(W, hp, mel, hp.n_audio_ctx, f16=True, attn16=attn16),
                          WO.encoder_forward_f16(W, hp, mel, attn16=attn16))


def test_a_reduced_context_is_not_a_slice_of_the_full_one(case):
    """n = 30 against rows 0 .. 29 of the full encoder: the difference is orders above every GPU bar of
    tests/test_gpu_audio_ctx.py (1e-4 / 4e-4 of the peak), so a library that sliced would fail there."""
    from tests.audio_ctx_oracle import encoder_forward_ctx
    hp, W, mel, full = case
    got = encoder_forward_ctx(W, hp, mel, 30)
    assert got.shape == (30, hp.n_audio_state)
    gap = np.abs(got - full[:30]).max() / np.abs(got).max()
    assert gap > 100 * 4e-4, gap
    got16 = encoder_forward_ctx(W, hp, mel, 30, f16=True)
    assert np.abs(got16 - got).max() / np.abs(got).max() < 0.01 * gap      # the modes differ far less than the contexts


@pytest.mark.parametrize("n", [1, 30, 129])
def test_frame_2n_is_the_convolutions_own_zero(case, n):
    """Mel frame 2 n reaches row n - 1 of the full-context stem (conv1 at frame 2 n - 1 reads it, conv2's row n - 1 reads
    that); with audio_ctx = n it is never read."""
    from oracle import whisper_oracle as WO
    from tests.audio_ctx_oracle import encoder_forward_ctx
    hp, W, mel, _ = case
    mel2 = mel.copy()
    mel2[:, 2 * n] += 1.0
    stem, stem2 = (WO.encoder_forward(W, hp, m, upto_layer=0) for m in (mel, mel2))
    assert np.abs(stem2[n - 1] - stem[n - 1]).max() > 1e-3
    assert np.array_equal(stem2[:n - 1], stem[:n - 1])                      # ... and no row before it
    a, b = encoder_forward_ctx(W, hp, mel, n), encoder_forward_ctx(W, hp, mel2, n)
    assert np.array_equal(a, b)
    # and the stem of the restatement is the full stem everywhere but in that last row
    import dataclasses
    hp0 = dataclasses.replace(hp, n_audio_layer=0)
    s = encoder_forward_ctx(W, hp0, mel, n)
    ref = WO._ln(stem[:n], W["encoder.ln_post.weight"].astype(np.float64), W["encoder.ln_post.bias"].astype(np.float64))
    assert np.allclose(s[:n - 1], ref[:n - 1], rtol=0, atol=1e-12) and np.abs(s[n - 1] - ref[n - 1]).max() > 1e-3


def test_argument_range(case):
    from tests.audio_ctx_oracle import encoder_forward_ctx
    hp, W, mel, _ = case
    for n in (0, -1, hp.n_audio_ctx + 1):
        with pytest.raises(ValueError):
            encoder_forward_ctx(W, hp, mel, n)


def test_the_two_names_are_declared_bound_and_mirrored():
    from crispy_amd import _native as N
    L = N.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in N.ALL_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
        assert re.search(r"pub fn %s\(" % name, rs), name
    assert re.search(r"int crispy_asr_set_audio_ctx\s*\(\s*crispy_asr \*h,\s*int n\s*\)", hdr)
    assert re.search(r"int crispy_asr_audio_ctx\s*\(\s*const crispy_asr \*h,\s*int \*n\s*\)", hdr)
    assert L.crispy_abi_version() == 6                                       # new entry points only
    assert re.search(r"#define CRISPY_ABI_VERSION 6\b", open(HEADER).read())
    assert re.search(r"pub const CRISPY_ABI_VERSION: c_int = 6;", rs)


def test_null_arguments_are_refused_without_a_device():
    import ctypes as C
    from crispy_amd import _native as N
    L = N.lib()
    bad = int(re.search(r"CRISPY_ERR_INVALID_ARG = (-?\d+)", open(HEADER).read()).group(1))
    n = C.c_int(-7)
    assert L.crispy_asr_set_audio_ctx(None, 30) == bad and L.crispy_last_error().decode().startswith("crispy_asr_set_audio_ctx:")
    assert L.crispy_asr_audio_ctx(None, C.byref(n)) == bad and L.crispy_last_error().decode().startswith("crispy_asr_audio_ctx:")
    assert n.value == -7

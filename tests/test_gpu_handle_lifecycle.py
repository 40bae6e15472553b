"""The Whisper handle owns every device buffer through its members (crispy_amd/csrc/api_util.h: DevBuf): what it computes must
not depend on what it allocated, regrew or let go before.  One-layer model at width 384 (the synthetic weights of
tests/test_host_sanitizers.py), seeded 1 s clips; a dense handle in precision modes 0 and 1 and a resident q5_0 handle.  The
encoder output and the greedy tokens of clip 0 are compared BIT FOR BIT between runs of the library itself -- at batch 1, at
batch 3 (the workspaces regrow) and at batch 1 again; after the precision modes 1 -> 2 -> 0 -> 1 on the same handle (the f16
and packed copies are made, the captured steps dropped); on a second handle loaded after the first was freed.  Parity with the
oracle is tests/test_gpu_whisper.py's and tests/test_gpu_resident.py's business; free device memory is not looked at (the cards
are shared)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROMPT = [50258, 50259, 50359, 50363]
N_NEW = 8


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from crispy_amd import synth_audio
    from crispy_amd.ggml_io import synthetic_vocab, write_ggml_quantized
    from crispy_amd.mel_filters import whisper_mel_filters
    from crispy_amd.whisper_weights import HParams, synthetic_whisper_weights
    hp = HParams(n_audio_layer=1, n_text_layer=1)
    W = synthetic_whisper_weights(hp, 2)
    path = str(tmp_path_factory.mktemp("lifecycle") / "one-layer-q5_0.bin")
    write_ggml_quantized(path, hp, W, whisper_mel_filters(80), synthetic_vocab(hp.n_vocab), "q5_0", keep=False)
    clips = [synth_audio.clip16k_np(900 + i, 16000) for i in range(3)]
    return hp, W, path, clips


def _load(model, kind):
    from crispy_amd.asr import WhisperEngine, WhisperModel
    hp, W, path, _ = model
    if kind == "resident":
        return WhisperEngine(path, resident=True)
    m = WhisperModel(hp, W)
    m.set_precision(int(kind))
    return m


def _clip0(m, clips):
    """Encoder output and greedy tokens of the first clip of a batch, as bytes / ids."""
    enc = m.encode(clips)
    toks, n = m.transcribe_tokens(clips, PROMPT, N_NEW)
    return enc[0].tobytes(), toks[0, :n[0]].tolist()


@pytest.mark.parametrize("kind", ["0", "1", "resident"])
def test_results_do_not_depend_on_the_handles_allocation_history(model, kind):
    from crispy_amd import _native as N
    clips = model[3]
    m = _load(model, kind)
    base = _clip0(m, clips[:1])
    assert len(base[1]) >= 1
    # (a) batch 1 -> 3 -> 1: the encoder and decoder workspaces regrow in between
    assert _clip0(m, clips) == base, "batch 3"
    assert _clip0(m, clips[:1]) == base, "batch 1 after batch 3"
    # (b) the precision modes in turn on the same handle, then the mode of this case again
    for mode in (1, 2, 0, 1):
        if kind == "resident" and mode != 1:          # a resident model runs in mode 1 only: refused, nothing changes
            with pytest.raises(N.CrispyError) as e:
                m.set_precision(mode)
            assert e.value.code == -6
        else:
            m.set_precision(mode)
    if kind != "resident":
        m.set_precision(int(kind))
    assert _clip0(m, clips[:1]) == base, "after precision modes 1, 2, 0, 1"
    # (c) a second handle, loaded after the first was freed
    m.close()
    m2 = _load(model, kind)
    assert _clip0(m2, clips[:1]) == base, "second handle"
    m2.close()

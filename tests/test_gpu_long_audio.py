"""Audio of any length through one call: the log-mel of clips longer than 30 s (`crispy_mel_compute_long_device` +
`crispy_mel_window_device`) and whisper_full's seek loop over them (`crispy_asr_transcribe{,_batch,_hooks}`), against the
float64 numpy log-mel for any length (tests/long_logmel_oracle.py, pinned to the C oracle by tests/test_long_logmel_oracle.py)
and the oracle's whisper_full (oracle/whisper_oracle.py), which takes any n_samples."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# GPU against the C oracle is held to 1e-4 (tests/test_gpu_whisper.py::test_mel_windows_match_oracle); the numpy form used
# here is within 2e-5 of the C oracle (tests/test_long_logmel_oracle.py)
MEL_BAR = 1e-4 + 2e-5


def _windows(lm, clip_idx, seeks, n_mel=80):
    """Both layouts of the windows (clip_idx[k], seeks[k]), one call each (a call takes at most as many windows as clips)."""
    import torch
    d_out = torch.empty(len(seeks), n_mel, 3000, device="cuda")
    d_out_t = torch.full((len(seeks), 3002, n_mel), 7.0, device="cuda")
    d_out_t[:, 0] = 0.0             # the padding frames are the encoder workspace's, written once when it is made
    d_out_t[:, -1] = 0.0
    torch.cuda.synchronize()
    for k, (ci, sk) in enumerate(zip(clip_idx, seeks)):
        lm.window_device([ci], [sk], d_out=d_out[k].data_ptr(), d_out_t=d_out_t[k].data_ptr())
    lm.synchronize()
    return d_out.cpu().numpy(), d_out_t.cpu().numpy()


def _check_windows(got, got_t, raws, clip_idx, seeks, what):
    from tests import long_logmel_oracle as LO
    for k, (ci, sk) in enumerate(zip(clip_idx, seeks)):
        ref = LO.window(raws[ci], sk)
        d, dt = np.abs(got[k] - ref).max(), np.abs(got_t[k] - LO.window_t(raws[ci], sk)).max()
        print(f"{what}: clip {ci} seek {sk}: max difference {d:.2e} / frame-major {dt:.2e}")
        assert d < MEL_BAR and dt < MEL_BAR, (what, ci, sk, d, dt)


def test_mel_windows_of_long_clips(oracle):
    """One batch of 70.2 s (no multiple of 160 samples, nor of a 64-frame tile), 480001 samples (the first length that was
    illegal) and 100000 samples, stride = the longest.  Windows at every kind of seek against the numpy form, both layouts;
    the short clip's windows are bit for bit what the 30 s path gives; the zero padding is the same float in both paths;
    10 minutes for the index arithmetic; the refusals."""
    import torch
    from crispy_amd import synth_audio
    from crispy_amd.asr import MAX_SAMPLES, LogMel
    from tests import long_logmel_oracle as LO
    from tests.long_audio_cases import N_LONG
    lens = [N_LONG, 480001, 100000]
    clips = [synth_audio.clip16k_np(40 + i, n) for i, n in enumerate(lens)]
    pcm = np.zeros((3, N_LONG), np.float32)
    for i, c in enumerate(clips):
        pcm[i, :c.size] = c
    raws = [LO.raw(c) for c in clips]
    lm = LogMel(80)
    d_pcm = torch.from_numpy(pcm).cuda()
    torch.cuda.synchronize()
    lm.compute_long_device(d_pcm.data_ptr(), N_LONG, np.array(lens, np.int32))
    last = LO.n_len_org(N_LONG)
    assert last == 7021
    seeks0 = [0, 2999, 3000, 3001, 3008, 4032, 6600, last - 1]
    ci = [0] * len(seeks0) + [1, 1, 1, 2, 2]
    sk = seeks0 + [0, 1500, LO.n_len_org(480001), 0, 200]
    got, got_t = _windows(lm, ci, sk)
    _check_windows(got, got_t, raws, ci, sk, "batch of three")
    # three windows in ONE call, clips in another order
    d3 = torch.empty(3, 80, 3000, device="cuda")
    lm.window_device([2, 0, 1], [200, 4032, 1500], d_out=d3.data_ptr())
    lm.synchronize()
    g3 = d3.cpu().numpy()
    assert np.array_equal(g3[0], got[sk.index(200, len(seeks0))]) and np.array_equal(g3[1], got[seeks0.index(4032)]) and np.array_equal(g3[2], got[len(seeks0) + 1])
    # the window at 6600 runs out of audio at frame 7021 - 6600: what follows is the clip's clamp floor, everywhere the same
    tail = got[seeks0.index(6600)][:, last - 6600 + 2:]
    assert tail.size > 0 and np.all(tail == tail[0, 0])
    # refusals: a seek above n_len_org of ITS clip, a clip outside the batch
    for bad_ci, bad_sk in ((0, last + 1), (2, LO.n_len_org(100000) + 1), (3, 0), (0, -1)):
        with pytest.raises(Exception):
            lm.window_device([bad_ci], [bad_sk], d_out=d3.data_ptr())
    long_bits = {s: got[len(seeks0) + 3 + j].copy() for j, s in enumerate((0, 200))}

    # the short clip alone through the 30 s path: the same bits (and that path's limits are back: seek <= 3000)
    d_short = torch.from_numpy(clips[2]).cuda()
    d1 = torch.empty(1, 80, 3000, device="cuda")
    torch.cuda.synchronize()
    lm.compute_device(d_short.data_ptr(), 100000, np.array([100000], np.int32), d_out=d1.data_ptr())
    lm.synchronize()
    assert np.array_equal(d1.cpu().numpy()[0], long_bits[0])
    lm.window_device([0], [200], d_out=d1.data_ptr())
    lm.synchronize()
    assert np.array_equal(d1.cpu().numpy()[0], long_bits[200])
    with pytest.raises(Exception):
        lm.window_device([0], [3001], d_out=d1.data_ptr())

    # The zero padding.  The 30 s path runs the frame kernel over it, the long path substitutes the float that kernel gives for
    # an all-zero frame.  On a quiet clip (maximum - 8 below log10(1e-10)) nothing clamps and the padding shows as it is stored.
    quiet_short = (clips[2] * np.float32(1e-3)).astype(np.float32)
    quiet_long = (synth_audio.clip16k_np(44, 500001) * np.float32(1e-3)).astype(np.float32)
    d_q = torch.from_numpy(quiet_short).cuda()
    torch.cuda.synchronize()
    lm.compute_device(d_q.data_ptr(), 100000, np.array([100000], np.int32), d_out=d1.data_ptr())
    lm.synchronize()
    pad_short = d1.cpu().numpy()[0][:, 700:]                     # frames past the audio (625 + 2) of the 30 s path
    d_q = torch.from_numpy(quiet_long).cuda()
    torch.cuda.synchronize()
    lm.compute_long_device(d_q.data_ptr(), 500001, np.array([500001], np.int32))
    lm.window_device([0], [3000], d_out=d1.data_ptr())
    lm.synchronize()
    w = d1.cpu().numpy()[0]
    pad_long = w[:, 3130 - 3000:]                                # frames past the audio (3125 + 2): the rest of the last stored tile, then past it (3136)
    assert np.all(pad_short == np.float32(-1.5)) and np.all(pad_long == np.float32(-1.5)), (pad_short.min(), pad_long.max())
    assert np.abs(w - LO.window(LO.raw(quiet_long), 3000)).max() < MEL_BAR
    # digital silence: the clip maximum is the padding's floor, not "below anything"
    d_z = torch.zeros(500001, device="cuda")
    torch.cuda.synchronize()
    lm.compute_long_device(d_z.data_ptr(), 500001, np.array([500001], np.int32))
    lm.window_device([0], [1000], d_out=d1.data_ptr())
    lm.synchronize()
    assert np.all(d1.cpu().numpy() == np.float32(-1.5))

    # 10 minutes: index arithmetic at scale (the sample index of the last frame is 9.6e6, the row offset 80 x 60032)
    n10 = 9600037
    x10 = synth_audio.clip16k_np(45, n10)
    r10 = LO.raw(x10)
    d_10 = torch.from_numpy(x10).cuda()
    torch.cuda.synchronize()
    lm.compute_long_device(d_10.data_ptr(), n10, np.array([n10], np.int32))
    sk10 = [0, 30000, 57000]
    got, got_t = _windows(lm, [0, 0, 0], sk10)
    _check_windows(got, got_t, [r10], [0, 0, 0], sk10, "10 min")

    # one sample above the cap is refused (before anything is read), and the handle goes on working
    with pytest.raises(Exception) as ei:
        lm.compute_long_device(d_10.data_ptr(), MAX_SAMPLES + 1, np.array([MAX_SAMPLES + 1], np.int32))
    assert str(MAX_SAMPLES) in str(ei.value)
    lm.compute_long_device(d_short.data_ptr(), 100000, np.array([100000], np.int32))
    lm.window_device([0], [200], d_out=d1.data_ptr())
    lm.synchronize()
    assert np.array_equal(d1.cpu().numpy()[0], long_bits[200])
    lm.close()


def _engine(tmp_path_factory, hp, W, tag, mode):
    from crispy_amd.asr import WhisperEngine
    from crispy_amd.ggml_io import synthetic_vocab, write_ggml
    from crispy_amd.mel_filters import whisper_mel_filters
    path = tmp_path_factory.mktemp("ggml_long") / f"ggml-{tag}.bin"
    write_ggml(str(path), hp, W, whisper_mel_filters(hp.n_mels), synthetic_vocab(hp.n_vocab), f16=False)
    eng = WhisperEngine(str(path))
    eng.set_precision(mode)
    return eng


def _same_windows(got, ref, tol_lp, what):
    """The bars of tests/test_gpu_decision.py::_same_windows, restated."""
    assert len(got) == len(ref), (what, got, [(w["seek"], w["temperature"]) for w in ref])
    for g, w in zip(got, ref):
        assert g["seek"] == w["seek"] and g["seek_advance"] == w["seek_advance"], (what, g, w["seek"], w["seek_advance"])
        assert abs(g["temperature"] - w["temperature"]) < 1e-6 and g["decoder"] == w["decoder"], (what, g, w["temperature"], w["decoder"])
        assert g["failed"] == int(w["failed"]) and g["no_speech"] == int(w["is_no_speech"]), (what, g, w["failed"], w["is_no_speech"])
        assert g["n_tokens"] == (0 if w["is_no_speech"] else len(w["tokens"])), (what, g, w["tokens"])
        assert abs(g["no_speech_prob"] - w["no_speech_prob"]) <= 5e-3 * w["no_speech_prob"] + 1e-7, (what, g, w["no_speech_prob"])
        if np.isfinite(w["avg_logprob"]):
            assert abs(g["avg_logprob"] - w["avg_logprob"]) <= tol_lp, (what, g, w["avg_logprob"])
        else:
            assert g["avg_logprob"] == w["avg_logprob"]
        assert abs(g["entropy"] - w["entropy"]) <= 1e-5, (what, g, w["entropy"])


def _same_segments(segs, rsegs):
    assert [(round(a * 100), round(b * 100), s) for a, b, s in segs] == [(a, b, s.decode()) for a, b, s in rsegs]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("script", ["bare", "past"])
def test_seek_loop_past_30_s_on_scripted_models(oracle, tmp_path_factory, script, mode):
    """70.2 s through `crispy_asr_transcribe` on a model whose decoder follows a script by position and ignores the audio.
    bare: every window says "<|0.00|> w1 w2 <|22.00|><|22.00|>" on the bare prompt (prev_text off): windows at 0 / 2200 /
    4400 / 6600.  past: the same picks after the text so far -- prompts of 3, 9, 14 tokens across the 30 s mark, and 3 again
    for the last window, which has under 5 s left and drops the past.  The shapes are asserted on the oracle's result first;
    then product == oracle."""
    from crispy_amd import synth_audio
    from crispy_amd.whisper_weights import HParams
    from tests import long_audio_cases as LC, oracle_cases as OC
    hp = HParams.tiny()
    sp, _, _ = OC.wcpp_masks(hp)
    EOT = sp["eot"]
    W = (LC.bare_script if script == "bare" else LC.past_script)(hp)
    kw = dict(prev_text=False) if script == "bare" else {}
    rsegs, rkept, rwins = OC.scripted_whisper_full(W, hp, LC.N_LONG, mode, **kw)
    assert [w["seek"] for w in rwins] == [0, 2200, 4400, 6600] and [w["seek_advance"] for w in rwins] == [2200, 2200, 2200, 421]
    assert [len(w["prompt"]) for w in rwins] == ([3, 3, 3, 3] if script == "bare" else [3, 9, 14, 3])
    assert all(w["prompt"][0] == sp["prev"] for w in rwins if len(w["prompt"]) > 3)
    assert all(w["temperature"] == 0.0 and not w["failed"] and not w["is_no_speech"] for w in rwins)
    eng = _engine(tmp_path_factory, hp, W, f"{script}{mode}", mode)
    x = synth_audio.clip16k_np(80, LC.N_LONG)
    text, segs, toks = eng.transcribe_segments(x, language_token=sp["lang0"], **kw)
    assert toks == [t for t in rkept if t != EOT], (toks, rkept)
    _same_segments(segs, rsegs)
    assert text == "".join(s for _, _, s in segs)
    _same_windows(eng.last_windows, rwins, 1e-4 if mode == 0 else 5e-3, f"{script} mode {mode}")
    eng.close()


def test_long_clips_in_a_batch_word_times_cancel_and_plain_greedy(oracle, tmp_path_factory):
    """On the conditioned script, mode 1: the long clip between a 7 s clip and a second long clip of another length equals
    its solo result in every field, and so do its neighbours; with dtw=True tokens and segments are unchanged, word times
    do not go back and lie in their window; a cancel flag set from the progress of window 2 ends the call; plain greedy
    (one window by definition) refuses the long clip and says so; one sample above the cap is refused with the cap."""
    from crispy_amd import synth_audio
    from crispy_amd.asr import MAX_SAMPLES, Cancelled, transcribe_batch
    from crispy_amd.whisper_weights import HParams
    from tests import long_audio_cases as LC, oracle_cases as OC
    hp = HParams.tiny()
    sp, _, _ = OC.wcpp_masks(hp)
    eng = _engine(tmp_path_factory, hp, LC.past_script(hp), "past-batch", 1)
    x = synth_audio.clip16k_np(80, LC.N_LONG)
    clips = [x[:16000 * 7], x, synth_audio.clip16k_np(81, 777777)]
    solo = []
    for c in clips:
        text, segs, toks = eng.transcribe_segments(c, language_token=sp["lang0"])
        solo.append((text, toks, sp["lang0"], segs, eng.last_windows))
    assert [w["seek"] for w in solo[1][4]] == [0, 2200, 4400, 6600] and len(solo[2][4]) == 3 and len(solo[0][4]) == 1
    got = transcribe_batch(eng, clips, language_token=sp["lang0"], timestamps=True, with_segments=True)
    for i in range(3):
        assert got[i] == solo[i], i
    # word-level timestamps over the long clip
    text, segs, toks = eng.transcribe_segments(x, language_token=sp["lang0"], dtw=True)
    assert (text, toks, segs) == (solo[1][0], solo[1][1], solo[1][3])
    words, wins = eng.last_words, eng.last_windows
    assert len(words) >= 2 * len(wins) and len(eng.last_token_times) == len(toks)
    t0s = [w[0] for w in words]
    assert all(b >= a for a, b in zip(t0s, t0s[1:])), t0s
    per_window = len(words) // len(wins)                          # every window says the same two words
    for i, (t0, t1, _word, _first, _n) in enumerate(words):
        lo = wins[min(i // per_window, len(wins) - 1)]["seek"] * 0.01
        assert lo - 1e-3 <= t0 <= t1 <= lo + 30.0 + 1e-3, (i, t0, t1, lo)
    assert t0s[-1] >= 66.0
    # cancel from the progress of window 2
    flag, seen = C.c_int(0), []

    def progress(done, total):
        seen.append((done, total))
        if len(seen) == 2:
            flag.value = 1

    with pytest.raises(Cancelled):
        eng.transcribe(x, language_token=sp["lang0"], timestamps=True, cancel=flag, progress=progress)
    assert seen == [(2200 * 160, x.size), (4400 * 160, x.size)], seen
    # ... and without the flag the hooks change nothing; the last progress is the whole clip
    seen.clear()
    flag.value = 0
    text2, toks2 = eng.transcribe(x, language_token=sp["lang0"], timestamps=True, cancel=flag, progress=lambda d, t: seen.append((d, t)))
    assert (text2, toks2, eng.last_segments, eng.last_windows) == (solo[1][0], solo[1][1], solo[1][3], solo[1][4])
    assert len(seen) == 4 and seen[-1] == (x.size, x.size)
    # plain greedy decodes one window
    with pytest.raises(Exception) as ei:
        eng.transcribe(x[:480001], language_token=sp["lang0"], timestamps=False)
    assert "no_timestamps" in str(ei.value) and "480000" in str(ei.value)
    eng.transcribe(x[:480000], language_token=sp["lang0"], timestamps=False, max_new_tokens=4)
    # the cap (the length check comes before anything is read: the array only has to be addressable)
    from crispy_amd import _native as N
    res = C.c_void_p()
    rc = N.lib().crispy_asr_transcribe(eng._h, x.ctypes.data, MAX_SAMPLES + 1, None, C.byref(res))
    assert rc == -1
    with pytest.raises(Exception) as ei:
        N.check(rc, N.lib())
    assert str(MAX_SAMPLES) in str(ei.value)
    eng.close()


def test_seek_loop_past_30_s_where_the_audio_matters(oracle, tmp_path_factory):
    """Random-init tiny on 43.75 s: four windows, the last one past frame 3000, each conditioned on the text so far.  The
    oracle (committed: tests/long_audio_cases.py) is whisper_full over the numpy log-mel of the whole clip and the float64
    encoder.  The clip is chosen so that the test would notice a wrong window: see the three assertions."""
    from tests import long_audio_cases as LC, oracle_cases as OC
    hp, W, x = LC.real_inputs()
    sp, _, _ = OC.wcpp_masks(hp)
    ref = LC.real_ref()
    bar = 1e-4
    past_30, margin, moved = LC.conditions(ref, bar)
    assert past_30, "no window at seek > 3000; choose another seed"
    assert margin > 1e-3, "test clip has an f32-unresolvable pick; choose another seed"
    assert moved > 10, "the last window's avg_logprob does not depend on its mel by 10 bars; choose another seed"
    rwins = ref["wins"]
    assert len(rwins) >= 3 and max(len(w["prompt"]) for w in rwins) > 3
    eng = _engine(tmp_path_factory, hp, W, "real", 0)
    text, segs, toks = eng.transcribe_segments(x, max_new_tokens=LC.REAL_MAX_NEW, language_token=sp["lang0"], fallback=False)
    assert toks == [t for t in ref["kept"] if t != sp["eot"]], (toks, ref["kept"])
    _same_segments(segs, [tuple(s) for s in ref["segs"]])
    _same_windows(eng.last_windows, rwins, bar, "real clip")
    eng.close()

"""The decode step of the catalog widths (tests/test_gpu_gemv_decode.py) beyond its first 14 positions: `whisper_dec_gemv.hip`
plus `attn_decoder_kv16` in every key class of the pass (1 / 2 / 4 key slots per wave of attn_dec_x16_kernel for up to 128 /
256 / 512 positions -- also the classes the captured steps are cached under), up to the last row of the positional embedding,
and with rows whose prompts differ in length (left-padded: `DecodePass::row_off`, `AttnRows::key_off`, `embed_*`'s `row_off`).

 * A: every key class against the oracle of precision mode 1 (DecoderCache(f16=True), teacher-forced on the GPU's picks) at
      the mode's bar, dense f16 at 768 / 1024 / 1280, and the skinny kernels (developer build, CRISPY_ASR_GEMV=0) at the same bar;
 * B: three rows with prompts of 3, 13 and 224 tokens in one pass of 264 keys == the rows alone, bytes, and == the oracle;
 * C: resident q4_1 / q5_0 blocks == the inflated file at 257 keys and with row offsets, bytes;
 * D: a row behind a 228-token prompt decodes to the same bits alone, in a batch of 6 and in one of 37.

The oracle runs on the CPU at ~13 ms per position: the rows of a width share one encoder output per row and one stem of
prompt ids, so a row's oracle walks its prompt once (`_Width.oracle_after`) and every case forks from where its prompt ends."""
import numpy as np
import pytest

from tests.native_variant import library_variant

pytestmark = pytest.mark.gpu

PREV, SOT, LANG0, TRANSCRIBE = 50361, 50258, 50259, 50359
WEIGHT_SEED = 5                 # synthetic_whisper_weights(hp, 5): plain fan-in-scaled weights, as in test_gpu_gemv_decode.py
ENC_SEED = 1000                 # + width: encoder outputs of the oracle cases
IDS = np.random.default_rng(228).integers(0, 50000, 224).tolist()        # the stem of every long prompt

# case -> (prompt tokens, new tokens); max_keys of the pass = their sum
CASES = {"edge0": (116, 12),    # 128: the 1-slot form, full
         "edge1": (117, 12),    # 129: the 2-slot form; its first generated step has 118 keys
         "edge2": (228, 28),    # 256: the 2-slot form, full
         "edge3": (228, 29),    # 257: the 4-slot form
         "end": (228, 220)}     # 448: the 4-slot form up to the last position of the context


def _hp(d, layers=2):
    from crispy_amd.whisper_weights import HParams
    return HParams(n_audio_state=d, n_audio_head=d // 64, n_audio_layer=1, n_text_state=d, n_text_head=d // 64, n_text_layer=layers)


def _prompt(n):
    """The conditioned prompt of tests/test_gpu_prefill.py: <|startofprev|> + text ids + the usual three."""
    return [PREV] + IDS[:n - 4] + [SOT, LANG0, TRANSCRIBE]


class _Width:
    """What the oracle cases of one width share: weights, three encoder outputs, the model on the GPU, and per encoder row the
    oracle's decoder after <|startofprev|> + IDS[:n] for every n asked for so far (never stepped again: callers get forks)."""

    def __init__(self, d):
        from crispy_amd.whisper_weights import synthetic_whisper_weights
        self.d, self.hp = d, _hp(d)
        self.W = synthetic_whisper_weights(self.hp, WEIGHT_SEED)
        rng = np.random.default_rng(ENC_SEED + d)
        self.enc = (rng.standard_normal((3, 1500, d)) * 0.8).astype(np.float32)
        self._stem = {}                 # (row, ids fed) -> DecoderCache; ids fed = -1: nothing fed, not even <|startofprev|>
        self._model = None

    def model(self):
        from crispy_amd.asr import WhisperModel
        if self._model is None:
            self._model = WhisperModel(self.hp, self.W)
            self._model.set_precision(1)
        return self._model

    def close(self):
        if self._model is not None:
            self._model.close()
            self._model = None

    def oracle_after(self, row, n_ids):
        from oracle import whisper_oracle as WO
        have = [k for (r, k) in self._stem if r == row and k <= n_ids]
        if have:
            at = max(have)
            dc = self._stem[(row, at)].fork()
        else:
            at = -1
            dc = WO.DecoderCache(self.W, self.hp, self.enc[row], f16=True)
            self._stem[(row, -1)] = dc.fork()
        while at < n_ids:
            dc.step(PREV if at < 0 else IDS[at])
            at += 1
        self._stem[(row, n_ids)] = dc
        return dc.fork()


@pytest.fixture(scope="module")
def width():
    """One width's shared state at a time (a width's oracle decoders hold float64 copies of its token embedding)."""
    held = {}

    def get(d):
        if d not in held:
            for w in held.values():
                w.close()
            held.clear()
            held[d] = _Width(d)
        return held[d]
    yield get
    for w in held.values():
        w.close()


def _teacher_forced(dc, last, picks):
    """The oracle's logit of every pick, its own arg-max and its top-2 margin, fed the picks."""
    n = len(picks)
    best = np.zeros(n); margin = np.zeros(n); ids = np.zeros(n, np.int64)
    tok = last
    for i in range(n):
        l = dc.step(tok)
        tok = int(picks[i])
        best[i] = l[tok]
        top = np.partition(l, -2)[-2:]
        margin[i] = top[1] - top[0]
        ids[i] = int(np.argmax(l))
    return best, margin, ids


A_CASES = [(768, c) for c in CASES] + [(1280, "edge1"), (1280, "edge3"), (1280, "end"), (1024, "edge3")]


@pytest.mark.parametrize("d,case", A_CASES)
def test_every_key_class_against_the_oracle(width, d, case):
    """Two rows behind one long prompt.  Measured on the MI355X (NOTEBOOK 17): rms 5.6e-5 .. 9.7e-5 and worst 1.3e-4 .. 2.7e-4 of
    scale over the cases, every pick resolved, no drift over the 64-position blocks of `end`.  `edge1` and `edge3` pin the class
    choice (their key count stays one short of the bound); `edge2` and `end` are the ones that fill the 2 and 4 slots."""
    import torch
    from crispy_amd.asr import WhisperModel
    w = width(d)
    hp, W = w.hp, w.W
    n_prompt, n_new = CASES[case]
    prompt = _prompt(n_prompt)
    assert len(prompt) == n_prompt
    B = 2
    enc = w.enc[:B]
    d_enc = torch.from_numpy(enc).to("cuda:0")
    torch.cuda.synchronize()
    m = w.model()
    tg, _, lg = m.decode_greedy_device(d_enc.data_ptr(), B, prompt, n_new)
    tg2, _, lg2 = m.decode_greedy_device(d_enc.data_ptr(), B, prompt, n_new)
    solo, _, lsolo = m.decode_greedy_device(d_enc[1:2].contiguous().data_ptr(), 1, prompt, n_new)
    assert np.array_equal(tg, tg2) and lg.tobytes() == lg2.tobytes()                  # deterministic
    assert np.array_equal(solo[0], tg[1]) and lsolo[0].tobytes() == lg[1].tobytes()    # alone = in the step, bit for bit
    skinny = d == 768 and case in ("edge1", "edge3")
    if skinny:
        with library_variant("dev", {"CRISPY_ASR_GEMV": "0"}):
            ms = WhisperModel(hp, W)
            try:
                ms.set_precision(1)
                ts, _, ls = ms.decode_greedy_device(d_enc.data_ptr(), B, prompt, n_new)
            finally:
                ms.close()
    rows = [0] if (case == "end" or d != 768) else [0, 1]
    best = np.zeros((len(rows), n_new)); margin = np.zeros((len(rows), n_new)); ids = np.zeros((len(rows), n_new), np.int64)
    for k, b in enumerate(rows):
        dc = w.oracle_after(b, n_prompt - 4)
        for t in prompt[-3:-1]:
            dc.step(t)
        best[k], margin[k], ids[k] = _teacher_forced(dc, prompt[-1], tg[b])
    scale = np.abs(best).max()
    eg = (lg[rows] - best) / scale
    resolved = margin > 1e-3 * scale
    print(f"d {d} {case} ({n_prompt} + {n_new}): gemv rms {np.sqrt(np.mean(eg ** 2)):.2e} worst {np.abs(eg).max():.2e}; "
          f"{int(resolved.sum())} of {resolved.size} picks resolved; scale {scale:.3f}")
    if case == "end":
        for lo in range(0, n_new, 64):
            e = eg[:, lo:lo + 64]
            print(f"    positions {n_prompt + lo} .. {n_prompt + lo + e.shape[1] - 1}: rms {np.sqrt(np.mean(e ** 2)):.2e} worst {np.abs(e).max():.2e}")
    assert np.sqrt(np.mean(eg ** 2)) < 1.6e-4 and np.abs(eg).max() < 5e-4
    assert resolved.sum() * 2 >= resolved.size, (int(resolved.sum()), resolved.size)
    assert np.array_equal(tg[rows][resolved], ids[resolved])
    if skinny:
        same = tg[rows] == ts[rows]
        es = (ls[rows] - best)[same] / scale
        print(f"    skinny rms {np.sqrt(np.mean(es ** 2)):.2e} worst {np.abs(es).max():.2e}; forms agree on {int(same.sum())} of {same.size} picks")
        assert np.sqrt(np.mean(es ** 2)) < 1.6e-4 and np.abs(es).max() < 5e-4
        assert np.array_equal(ts[rows][resolved], ids[resolved])


def _window_prompts(n_long):
    """Bare; <|startofprev|> + 9 ids; <|startofprev|> + n_long ids and another language token."""
    init = [SOT, LANG0, TRANSCRIBE]
    return [init, [PREV] + IDS[:9] + init, [PREV] + IDS[:n_long] + [SOT, LANG0 + 3, TRANSCRIBE]]


def _window_rows_equal_their_solo_runs(m, d_enc, prompts, n_new, seek_end):
    rows = len(prompts)
    got = m.decode_window_device(d_enc.data_ptr(), prompts, n_new, seek=[0] * rows, seek_end=[seek_end] * rows)
    toks, tids, plog, nosp, n = got
    for b in range(rows):
        t1, i1, p1, s1, n1 = m.decode_window_device(d_enc[b:b + 1].contiguous().data_ptr(), [prompts[b]], n_new, seek=[0], seek_end=[seek_end])
        assert np.array_equal(t1[0], toks[b]) and np.array_equal(i1[0], tids[b]) and n1[0] == n[b], (b, t1[0], toks[b])
        assert p1[0].tobytes() == plog[b].tobytes() and s1[0].tobytes() == nosp[b].tobytes(), (b, p1[0], plog[b], s1[0], nosp[b])
    return got


WINDOW_NEW = 40


def test_rows_with_unequal_prompts_at_a_catalog_width(width):
    """tests/test_gpu_decision.py::test_window_pass_statistics_and_rows_with_different_prompts at width 768 and 264 keys: prompts
    of 3, 13 and 224 tokens (the most whisper_full carries) -- the 4-slot attention with key_off = 221 / 211 / 0, the gemv
    q | k | v epilogue writing cache rows at the pass's position, the shortest row attending over 3 .. 43 keys of its own.
    Rows 0 and 2 against the oracle (row 2 shares its encoder output and its stem with the cases above)."""
    import torch
    from oracle import whisper_oracle as WO
    from tests.oracle_cases import wcpp_masks
    w = width(768)
    hp = w.hp
    sp, sup, sup_first = wcpp_masks(hp)
    assert (sp["prev"], sp["sot"], sp["lang0"], sp["transcribe"]) == (PREV, SOT, LANG0, TRANSCRIBE)
    prompts = _window_prompts(220)
    assert [len(p) for p in prompts] == [3, 13, 224]
    order = [1, 2, 0]                            # row 2 decodes encoder output 0
    d_enc = torch.from_numpy(np.ascontiguousarray(w.enc[order])).to("cuda:0")
    torch.cuda.synchronize()
    m = w.model()
    n_new, seek_end = WINDOW_NEW, WO.n_len_org(480000)
    toks, tids, plog, nosp, n = _window_rows_equal_their_solo_runs(m, d_enc, prompts, n_new, seek_end)
    rel = 4 * 4e-4
    compared = picks = 0
    for b in (0, 2):
        dc = w.oracle_after(order[b], len(prompts[b]) - 4)
        lg = None
        for t in prompts[b][-3:]:
            lg = dc.step(t)
        ref_nosp = float(np.exp(WO._log_softmax(np.asarray(lg, np.float64))[sp["nosp"]]))
        tol_p = 3.0 * rel * float(np.abs(lg).max())
        assert abs(nosp[b] - ref_nosp) <= tol_p * ref_nosp + 1e-9, (b, nosp[b], ref_nosp, tol_p)
        seq = []
        for i in range(int(n[b])):
            g = int(toks[b, i])
            ml, lp, tid = WO.process_logits(lg, seq, sp, WO.RULES_WCPP, sup, sup_first)
            fin = ml[np.isfinite(ml)]
            thr = rel * float(np.abs(lg).max())
            assert np.isfinite(ml[g]) and ml.max() - ml[g] <= thr, (b, i, g, int(np.argmax(ml)), float(ml.max() - ml[g]), thr)
            top2 = np.partition(fin, -2)[-2:] if fin.size > 1 else np.array([-np.inf, fin[0]])
            if top2[1] - top2[0] > thr:
                assert g == int(np.argmax(ml)), (b, i)
                assert abs(plog[b, i] - lp[g]) <= 2 * thr, (b, i, plog[b, i], lp[g], thr)
                assert int(tids[b, i]) == (g if g >= sp["beg"] else tid), (b, i, tids[b, i], tid)
                compared += 1
            picks += 1
            seq.append(g)
            if i + 1 < int(n[b]):
                lg = dc.step(g)
    print(f"unequal prompts at 768: {compared} of {picks} picks of rows 0 and 2 resolvable; picks per row {n.tolist()}; no_speech_prob {nosp.tolist()}")
    assert compared * 2 >= picks, (compared, picks)


def test_rows_with_unequal_prompts_in_the_two_slot_class(width):
    """129 keys: prompts of 3, 13 and 89 tokens + 40 picks -- attn_dec_x16_kernel<2> with key offsets 86 / 76 / 0.  Rows == solo rows."""
    import torch
    from oracle import whisper_oracle as WO
    w = width(768)
    prompts = _window_prompts(85)
    assert max(len(p) for p in prompts) + WINDOW_NEW == 129
    d_enc = torch.from_numpy(w.enc).to("cuda:0")
    torch.cuda.synchronize()
    toks = _window_rows_equal_their_solo_runs(w.model(), d_enc, prompts, WINDOW_NEW, WO.n_len_org(480000))[0]
    assert len({tuple(t) for t in toks.tolist()}) == 3, toks


@pytest.fixture(scope="module")
def quantised(tmp_path_factory):
    """The ggml files of the resident cases, written once: (width, kind) -> (path, three encoder outputs)."""
    from crispy_amd.ggml_io import synthetic_vocab, write_ggml_quantized
    from crispy_amd.mel_filters import whisper_mel_filters
    from crispy_amd.whisper_weights import synthetic_whisper_weights
    made = {}

    def get(d, kind):
        if kind not in made:
            hp = _hp(d)
            W = synthetic_whisper_weights(hp, 7, sensitive=True)
            path = str(tmp_path_factory.mktemp("ggml_long") / f"w{d}-{kind}.bin")
            write_ggml_quantized(path, hp, W, whisper_mel_filters(80), synthetic_vocab(hp.n_vocab), kind)
            rng = np.random.default_rng(d + len(kind))
            made[kind] = (path, (rng.standard_normal((3, 1500, d)) * 0.8).astype(np.float32))
        return made[kind]
    return get


@pytest.mark.parametrize("d,kind", [(1024, "q4_1"), (1280, "q5_0")])
def test_resident_blocks_equal_the_inflated_file_in_the_four_slot_class(quantised, d, kind):
    """medium's and large-v3's types behind a 228-token prompt, 257 keys: resident == inflated, ids and picked-logit bytes."""
    import torch
    from crispy_amd.asr import WhisperEngine
    path, enc = quantised(d, kind)
    n_prompt, n_new = CASES["edge3"]
    prompt = _prompt(n_prompt)
    B = 2
    d_enc = torch.from_numpy(enc[:B]).to("cuda:0")
    torch.cuda.synchronize()
    res = WhisperEngine(path, resident=True)
    inf = WhisperEngine(path)
    try:
        inf.set_precision(1)
        tr, _, lr = res.decode_greedy_device(d_enc.data_ptr(), B, prompt, n_new)
        ti, _, li = inf.decode_greedy_device(d_enc.data_ptr(), B, prompt, n_new)
        t1, _, l1 = res.decode_greedy_device(d_enc[1:2].contiguous().data_ptr(), 1, prompt, n_new)
    finally:
        res.close(); inf.close()
    assert np.array_equal(tr, ti) and lr.tobytes() == li.tobytes(), (tr, ti)
    assert np.array_equal(t1[0], tr[1]) and l1[0].tobytes() == lr[1].tobytes()
    assert len({tuple(t) for t in tr.tolist()}) == B


def test_resident_blocks_with_unequal_prompts(quantised):
    """The three rows of 3, 13 and 224 prompt tokens on the q4_1 file of width 1024: embed_q_kernel's row_off arm (a resident
    model embeds from the quantised token embedding), resident == inflated for all five outputs, every resident row == its solo run."""
    import torch
    from crispy_amd.asr import WhisperEngine
    from oracle import whisper_oracle as WO
    path, enc = quantised(1024, "q4_1")
    prompts = _window_prompts(220)
    d_enc = torch.from_numpy(enc).to("cuda:0")
    torch.cuda.synchronize()
    seek_end = WO.n_len_org(480000)
    res = WhisperEngine(path, resident=True)
    inf = WhisperEngine(path)
    try:
        inf.set_precision(1)
        r = _window_rows_equal_their_solo_runs(res, d_enc, prompts, WINDOW_NEW, seek_end)
        i = inf.decode_window_device(d_enc.data_ptr(), prompts, WINDOW_NEW, seek=[0] * 3, seek_end=[seek_end] * 3)
    finally:
        res.close(); inf.close()
    for a, b, what in zip(r, i, ("tokens", "timestamp ids", "log-probabilities", "no_speech_prob", "picks")):
        assert a.tobytes() == b.tobytes(), (what, a, b)
    assert len({tuple(t) for t in r[0].tolist()}) == 3, r[0]


def test_a_row_behind_a_long_prompt_decodes_to_the_same_bits_in_any_batch():
    """test_a_row_of_a_catalog_width_decodes_to_the_same_bits_in_any_batch in the 4-slot class: six clips behind the 228-token prompt,
    alone, as 6 rows and as 37 (LayerNorm as a launch of its own, the rows four at a time in several gridDim.y chunks)."""
    import torch
    from crispy_amd.asr import WhisperModel
    from crispy_amd.whisper_weights import synthetic_whisper_weights
    d = 768
    hp = _hp(d)
    m = WhisperModel(hp, synthetic_whisper_weights(hp, 11, sensitive=True))
    rng = np.random.default_rng(d + 228)
    base = (rng.standard_normal((6, 1500, d)) * 0.8).astype(np.float32)
    prompt, n_new = _prompt(228), 12
    try:
        m.set_precision(1)
        ref = {}
        for B in (1, 6, 37):
            d_enc = torch.from_numpy(np.ascontiguousarray(base[np.arange(B) % 6])).to("cuda:0")
            torch.cuda.synchronize()
            t, _, l = m.decode_greedy_device(d_enc.data_ptr(), B, prompt, n_new)
            for r in range(B):
                key = r % 6
                if key not in ref:
                    ref[key] = (t[r].copy(), l[r].tobytes())
                assert np.array_equal(t[r], ref[key][0]) and l[r].tobytes() == ref[key][1], (B, r)
            del d_enc
        assert len({tuple(v[0].tolist()) for v in ref.values()}) >= 3      # the six clips do not all decode alike
    finally:
        m.close()

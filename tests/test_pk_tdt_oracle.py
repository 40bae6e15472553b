"""Host side of Parakeet's TDT decoder (crispy_pk_tdt_*, include/crispy_hip.h), no GPU: the oracle (tests/pk_tdt_oracle.py) pinned on
transformers' ParakeetForTDT -- single steps through forward with a ParakeetRNNTDecoderCache, whole clips through generate() -- and on
the committed outputs of it; what the fixture's float64 paths cover; the step budget; the tensor table against the oracle's state
dict; the new symbols on every layer; the word grouping; and what the load and the decode refuse before a device is touched."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from tests import pk_oracle as PO
from tests import pk_tdt_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "parakeet_tdt_golden.npz")
NEW = ("crispy_pk_tdt_create", "crispy_pk_tdt_destroy", "crispy_pk_tdt_tensor_spec", "crispy_pk_tdt_load", "crispy_pk_tdt_loaded",
       "crispy_pk_tdt_config_of", "crispy_pk_tdt_max_steps", "crispy_pk_tdt_decode_device", "crispy_pk_tdt_decode", "crispy_pk_tdt_words")
# The float64 oracle and the float64 library run the same operations on the same numbers; what separates them is the order of
# float64 sums inside two BLAS calls, 1e-15 of logits that are about 10 large.  1e-11 is a thousand times that.
LIBRARY_BOUND = 1e-11
CFG = TO.TINY_TDT


def _lib():
    from crispy_amd import _native as N
    return N, N.lib()


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_parakeet_tdt_golden as G
    finally:
        sys.path.pop(0)
    return G


@pytest.fixture(scope="module")
def weights():
    return TO.make_tdt_weights(CFG, TO.GOLDEN_SEED, **TO.MIX)


@pytest.fixture(scope="module")
def oracle64(weights):
    import torch
    return TO.Tdt(CFG, weights, torch.float64)


def test_oracle_steps_against_the_transformers_modules(weights, oracle64):
    """single-step logits through ParakeetForTDT.forward with a ParakeetRNNTDecoderCache, float64"""
    pytest.importorskip("transformers.models.parakeet")
    G = _tool()
    net = G.library_model(CFG, weights)      # asserts the state-dict keys and their order
    for t in TO.GOLDEN_FRAMES + (12,):
        e = TO.frames(t, CFG.hidden, t)
        steps, logits = G.library_path(net, CFG, e)
        mine, mine_logits = oracle64.decode(e, with_logits=True)
        assert np.array_equal(steps, mine), t
        err = float(np.abs(logits - mine_logits).max())
        print(f"pk tdt oracle T' {t}: {len(steps)} steps, {err:.3e} from transformers' ParakeetForTDT in float64")
        assert err <= LIBRARY_BOUND
        assert float(np.abs(oracle64.logits_along(e, steps) - logits).max()) <= LIBRARY_BOUND


def test_oracle_paths_against_generate(weights):
    """generate()'s sequences and durations on single clips, float32 both; the duration biases are lowered by a constant, which
    changes no decision of the loop and keeps generate()'s own arg-max over all V + n_d logits inside the vocabulary"""
    pytest.importorskip("transformers.models.parakeet")
    import torch
    G = _tool()
    net = G.library_model(CFG, weights, dtype=torch.float32, duration_shift=1000.0)
    mine = TO.Tdt(CFG, weights, torch.float32)
    total = 0
    for rows in (9, 41, 200, 513):
        feats = torch.from_numpy(PO.clip(rows, PO.TINY.mel_bins, rows))[None]
        with torch.no_grad():
            e = net.encoder(feats).last_hidden_state[0].numpy()
            out = net.generate(input_features=feats)
        seq, dur = out.sequences[0].numpy(), out.durations[0].numpy()
        steps = mine.decode(e)
        assert seq[0] == CFG.blank and dur[0] == 0 and len(seq) == len(steps) + 1, (rows, len(seq), len(steps))
        assert np.array_equal(seq[1:], steps[:, 0]) and np.array_equal(dur[1:], steps[:, 2]), rows
        assert np.array_equal(np.cumsum(dur)[:-1], steps[:, 1])      # frames are the running sum of the durations
        assert len(steps) <= TO.max_steps(CFG, e.shape[0])
        total += len(steps)
    assert total > 20


def test_oracle_against_the_committed_library_outputs(oracle64):
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(f"{k}{t}" for t in TO.GOLDEN_FRAMES for k in ("frames", "steps", "first", "last"))
    for t in TO.GOLDEN_FRAMES:
        e = gold[f"frames{t}"]
        assert e.dtype == np.float32 and np.array_equal(e, TO.frames(t, CFG.hidden, t))
        steps, logits = oracle64.decode(e, with_logits=True)
        assert gold[f"steps{t}"].dtype == np.int32 and np.array_equal(steps, gold[f"steps{t}"]), t
        first, last = gold[f"first{t}"], gold[f"last{t}"]
        assert first.dtype == np.float64 and first.shape == (min(3, len(steps)), CFG.width)
        err = max(float(np.abs(logits[:3] - first).max()), float(np.abs(logits[-3:] - last).max()))
        print(f"pk tdt golden T' {t}: {len(steps)} steps, float64 oracle {err:.3e} from the file")
        assert err <= LIBRARY_BOUND


def test_fixture_paths_cover_what_the_gpu_tests_rest_on():
    """every duration, blanks forced from 0 to 1, runs at one frame, ends on the budget, an overshoot past T' by more than one frame,
    a clip of blanks only and one without any -- and the top-two gaps the path test needs, on every clip"""
    import torch
    paths, by_set = [], {}
    for name, (kw, seed) in TO.FIXTURE_SETS.items():
        w = TO.make_tdt_weights(CFG, seed, **kw)
        o64, o32 = TO.Tdt(CFG, w, torch.float64), TO.Tdt(CFG, w, torch.float32)
        for which, n_frames, fseed in TO.FIXTURE_CLIPS:
            if which != name:
                continue
            e = TO.frames(n_frames, CFG.hidden, fseed)
            steps, logits = o64.decode(e, with_logits=True)
            paths.append((n_frames, steps, logits))
            by_set.setdefault(name, []).append((n_frames, steps, logits))
            if len(steps):
                err = float(np.abs(o32.logits_along(e, steps) - logits).max())
                gaps = TO.top_two_gaps(logits, CFG.vocab)
                assert min(gaps) >= TO.GAP_FACTOR * err, (name, n_frames, gaps, err)
    cov = TO.coverage(CFG, paths)
    print("pk tdt fixture:", cov)
    assert cov["durations"] >= set(CFG.durations)
    assert cov["forced_blanks"] >= 1 and cov["longest_run"] >= 3 and cov["budget_ends"] >= 1 and cov["overshoot"] >= 2
    stall, blanks, tokens, mix = (TO.coverage(CFG, by_set[k]) for k in ("stall", "blanks", "tokens", "mix"))
    assert stall["budget_ends"] == 2 and stall["blanks"] == 0 and stall["longest_run"] == TO.max_steps(CFG, 3)
    assert blanks["tokens"] == 0 and blanks["blanks"] > 0 and tokens["blanks"] == 0 and tokens["tokens"] > 0
    assert mix["blanks"] > 0 and mix["tokens"] > 0      # the mask: some clips skip the prediction network while others run it
    assert [t for _n, t, _s in TO.FIXTURE_CLIPS[:len(TO.RAGGED_FRAMES)]] == list(TO.RAGGED_FRAMES) == [0, 1, 2, 5, 31, 32, 33, 65]


def test_max_steps_is_generates_budget():
    N, L = _lib()
    from crispy_amd.parakeet import make_tdt_config, pk_tdt_max_steps
    assert L.crispy_pk_tdt_max_steps.restype is C.c_long
    for cfg in (CFG, TO.CATALOG_TDT, TO.TdtConfig(256, 128, 1, 5, 0, (1, 3), 1)):
        for t in (-3, 0, 1, 2, 5, 375, 5000):
            assert pk_tdt_max_steps(cfg.as_dict(), t) == TO.max_steps(cfg, t) == (max(0, cfg.max_symbols_per_step * t - 1) if t > 0 else 0)
    c = make_tdt_config(CFG.as_dict())
    assert L.crispy_pk_tdt_max_steps(C.byref(c), 5001) == -1 and b"frames 5001" in L.crispy_last_error()
    assert L.crispy_pk_tdt_max_steps(None, 5) == -1 and b"cfg is NULL" in L.crispy_last_error()


def test_new_symbols_on_every_layer_and_abi_unchanged():
    N, L = _lib()
    assert N.PK_TDT_SYMBOLS == NEW and set(NEW) <= set(N.ALL_SYMBOLS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crispy_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(L, s).argtypes is not None, s
        assert re.search(r"pub fn %s\(" % s, rust), s
    assert L.crispy_abi_version() == 6 == N.ABI_VERSION and "#define CRISPY_ABI_VERSION 6" in hdr
    fields = re.search(r"typedef struct crispy_pk_tdt_config \{\s*int ([^;]*);", hdr).group(1)
    names = tuple(f.strip() for f in fields.split(","))
    assert names == ("hidden", "decoder_hidden", "decoder_layers", "vocab", "blank", "n_durations", "durations[8]", "max_symbols_per_step")
    assert tuple(n.split("[")[0] for n in names) == tuple(k for k, _t in N.PkTdtConfig._fields_)
    body = re.search(r"pub struct crispy_pk_tdt_config \{(.*?)\n\}", rust, flags=re.S).group(1)
    assert tuple(re.findall(r"pub (\w+): (?:c_int|\[c_int; 8\]),", body)) == tuple(k for k, _t in N.PkTdtConfig._fields_)
    assert "pub durations: [c_int; 8]," in body and C.sizeof(N.PkTdtConfig) == 15 * 4
    import crispy_amd
    from crispy_amd.parakeet import ParakeetTDT
    assert crispy_amd.ParakeetTDT is ParakeetTDT


@pytest.mark.parametrize("cfg", [CFG, TO.CATALOG_TDT, TO.TdtConfig(512, 256, 3, 100, 7, (0, 2, 5))], ids=["tiny", "catalog", "three layers"])
def test_tensor_spec_is_the_oracles_state_dict(cfg):
    from crispy_amd.parakeet import pk_tdt_tensor_spec
    assert pk_tdt_tensor_spec(cfg.as_dict()) == TO.tensor_list(cfg)


def test_config_limits_name_the_field():
    N, L = _lib()
    from crispy_amd.parakeet import make_tdt_config
    ok = make_tdt_config(CFG.as_dict())
    n = L.crispy_pk_tdt_tensor_spec(C.byref(ok), 0, None, None)
    assert n == len(TO.tensor_list(CFG)) == 15
    for i in (-1, n):
        assert L.crispy_pk_tdt_tensor_spec(C.byref(ok), i, None, None) == -1 and b"outside" in L.crispy_last_error()
    assert L.crispy_pk_tdt_tensor_spec(None, 0, None, None) == -1 and b"cfg is NULL" in L.crispy_last_error()
    bad = [("hidden", 250), ("hidden", 0), ("decoder_hidden", 64), ("decoder_hidden", 192), ("decoder_hidden", 2176), ("decoder_layers", 0),
           ("decoder_layers", 9), ("vocab", 1), ("vocab", 65537), ("blank", 33), ("blank", -1), ("n_durations", 0), ("n_durations", 9),
           ("max_symbols_per_step", 0), ("max_symbols_per_step", 65)]
    for field, value in bad:
        cfg = make_tdt_config(dict(CFG.as_dict(), **{field: value}))
        assert L.crispy_pk_tdt_tensor_spec(C.byref(cfg), 0, None, None) == -1, (field, value)
        assert field.encode() in L.crispy_last_error(), (field, L.crispy_last_error())
    for durations in ([0, 1, 1, 3, 4], [0, 2, 1, 3, 4], [-1, 0, 1, 2, 3], [4, 3, 2, 1, 0]):
        cfg = make_tdt_config(dict(CFG.as_dict(), durations=durations))
        assert L.crispy_pk_tdt_tensor_spec(C.byref(cfg), 0, None, None) == -1 and b"durations[" in L.crispy_last_error(), durations
    for good in (dict(vocab=65536, blank=65535), dict(decoder_hidden=2048), dict(n_durations=8, durations=[0, 1, 2, 3, 4, 5, 6, 7]),
                 dict(n_durations=1, durations=[1])):
        cfg = make_tdt_config(dict(CFG.as_dict(), **good))
        assert L.crispy_pk_tdt_tensor_spec(C.byref(cfg), 0, None, None) == 15, good


def _load(L, h, cfg, tensors, counts=None, null=None, extra=()):
    from crispy_amd.parakeet import make_tdt_config
    names = list(tensors) + list(extra)
    arrs = [np.ascontiguousarray(tensors[k], dtype=np.float32).reshape(-1) for k in names]
    cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
    cd = (C.c_void_p * len(names))(*[None if k == null else a.ctypes.data for k, a in zip(names, arrs)])
    cnt = np.array([a.size if counts is None or k not in counts else counts[k] for k, a in zip(names, arrs)], np.int64)
    c = make_tdt_config(cfg if isinstance(cfg, dict) else cfg.as_dict())
    rc = L.crispy_pk_tdt_load(h, C.byref(c), cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), len(names))
    return rc, L.crispy_last_error()


def test_load_validates_before_touching_a_device(weights):
    N, L = _lib()
    fake = C.c_void_p(1)      # never dereferenced: every case below fails before the handle is used
    rc, msg = _load(L, None, CFG, weights)
    assert rc == -1 and b"NULL handle" in msg
    assert L.crispy_pk_tdt_loaded(None) == 0
    for name in ("encoder_projector.weight", "decoder.embedding.weight", "decoder.lstm.bias_hh_l1", "decoder.decoder_projector.bias", "joint.head.weight"):
        rc, msg = _load(L, fake, CFG, {k: v for k, v in weights.items() if k != name})
        assert rc == -1 and name.encode() in msg and b"missing" in msg, (name, msg)
    rc, msg = _load(L, fake, CFG, weights, extra=["decoder.lstm.weight_ih_l0"])
    assert rc == -1 and b"decoder.lstm.weight_ih_l0" in msg and b"twice" in msg
    for name in ("decoder.lstm.weight_ih_l2", "encoder.layers.0.norm_out.bias", "joint.head.scale"):      # a third layer, an encoder tensor
        rc, msg = _load(L, fake, CFG, dict(weights, **{name: np.zeros(4, np.float32)}))
        assert rc == -1 and name.encode() in msg and b"unknown" in msg, (name, msg)
    for name, off in (("joint.head.weight", -128), ("joint.head.bias", 1), ("decoder.lstm.weight_hh_l0", 128), ("decoder.embedding.weight", -1)):
        rc, msg = _load(L, fake, CFG, weights, counts={name: int(np.asarray(weights[name]).size) + off})
        assert rc == -1 and name.encode() in msg and b"expected" in msg, (name, msg)
    rc, msg = _load(L, fake, CFG, weights, null="decoder.lstm.weight_hh_l1")
    assert rc == -1 and b"decoder.lstm.weight_hh_l1" in msg and b"NULL" in msg
    for name, bad in (("joint.head.bias", np.nan), ("decoder.lstm.weight_ih_l1", np.inf)):
        w = dict(weights)
        w[name] = np.array(weights[name], np.float32)
        w[name].reshape(-1)[-1] = bad
        rc, msg = _load(L, fake, CFG, w)
        assert rc == -1 and name.encode() in msg and b"non-finite" in msg, (name, msg)
    for field, bad in (("decoder_hidden", 200), ("blank", 40), ("vocab", 0), ("n_durations", 12)):
        rc, msg = _load(L, fake, dict(CFG.as_dict(), **{field: bad}), weights)
        assert rc == -1 and field.encode() in msg, (field, msg)
    c = N.PkTdtConfig()
    assert L.crispy_pk_tdt_load(fake, None, None, None, None, 15) == -1 and b"cfg is NULL" in L.crispy_last_error()
    from crispy_amd.parakeet import make_tdt_config
    c = make_tdt_config(CFG.as_dict())
    assert L.crispy_pk_tdt_load(fake, C.byref(c), None, None, None, 15) == -1 and b"NULL" in L.crispy_last_error()


def test_decode_validates_before_touching_a_device():
    N, L = _lib()
    fake, ptr = C.c_void_p(1), C.c_void_p(256)
    lp = C.POINTER(C.c_long)
    off = np.array([0, 5, 5], np.int64)
    for fn, tail in ((L.crispy_pk_tdt_decode_device, (None,)), (L.crispy_pk_tdt_decode, ())):
        assert fn(None, ptr, off.ctypes.data_as(lp), 2, ptr, ptr, None, None, *tail) == -1 and b"NULL handle" in L.crispy_last_error()
        for n in (0, -1, 4097):
            assert fn(fake, ptr, off.ctypes.data_as(lp), n, ptr, ptr, None, None, *tail) == -1
            assert b"n_clips %d" % n in L.crispy_last_error()
        assert fn(fake, ptr, None, 2, ptr, ptr, None, None, *tail) == -1 and b"frame_offset is NULL" in L.crispy_last_error()
        big = np.array([0, 5001], np.int64)
        assert fn(fake, ptr, big.ctypes.data_as(lp), 1, ptr, ptr, None, None, *tail) == -1 and b"5001 frames" in L.crispy_last_error()
        back = np.array([0, 5, 3], np.int64)
        assert fn(fake, ptr, back.ctypes.data_as(lp), 2, ptr, ptr, None, None, *tail) == -1 and b"clip 1 has -2 frames" in L.crispy_last_error()
        shifted = np.array([1, 9], np.int64)
        assert fn(fake, ptr, shifted.ctypes.data_as(lp), 1, ptr, ptr, None, None, *tail) == -1 and b"frame_offset[0]" in L.crispy_last_error()
    assert N.PK_TDT_MAX_FRAMES == 5000 == PO.frames(N.PK_MAX_ROWS)


def test_one_state_dict_loads_both_handles(weights):
    import torch
    from crispy_amd.parakeet import state_dict_items, tdt_state_dict_items
    enc = PO.make_weights(PO.TINY, 1)
    full = {"encoder." + k: torch.from_numpy(v) for k, v in enc.items()}
    full.update({k: torch.from_numpy(v) for k, v in weights.items()})
    assert [k for k, _a in state_dict_items(full)] == list(enc)
    items = tdt_state_dict_items(full)
    assert [k for k, _a in items] == list(weights)
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, weights[k].reshape(-1)) for k, a in items)


# ---- words ----------------------------------------------------------------------------------------------------------------
PIECES = ["▁he", "llo", "▁wor", "ld", "é", "▁日本", "語", "▁", "s", "<blank>"]
BLANK = 9


def _words(steps, frames, spf=0.08):
    from crispy_amd.parakeet import pk_tdt_words
    got = pk_tdt_words(steps, PIECES, frames, BLANK, spf)
    want = TO.words(steps, PIECES, frames, BLANK, spf)
    assert [(float(a), float(b), t) for a, b, t in got] == [(float(a), float(b), t) for a, b, t in want]
    assert all(a.dtype == np.float32 and b.dtype == np.float32 for a, b, _t in got)
    return got


def test_words_markers_multibyte_pieces_and_times():
    got = _words([[0, 0, 1], [1, 1, 2], [9, 3, 1], [2, 4, 0], [3, 4, 3], [9, 7, 4]], 20)
    assert [t for _a, _b, t in got] == ["hello", "world"]
    assert got[0][0] == np.float32(0.0) and got[0][1] == np.float32(3 * 0.08)      # first token's frame; last token's frame + duration
    assert got[1][0] == np.float32(4 * 0.08) and got[1][1] == np.float32(7 * 0.08)
    got = _words([[5, 2, 1], [6, 3, 2], [4, 5, 1]], 9)      # three-byte pieces behind a three-byte marker, then a two-byte piece
    assert [t for _a, _b, t in got] == ["日本語é"] and got[0][0] == np.float32(0.16) and got[0][1] == np.float32(0.48)
    got = _words([[4, 0, 2], [1, 2, 1], [0, 3, 1]], 9)      # a first piece without the marker still starts a word
    assert [t for _a, _b, t in got] == ["éllo", "he"]
    got = _words([[7, 0, 1], [8, 1, 1], [7, 2, 1]], 9)      # the marker alone: a word that begins empty
    assert [t for _a, _b, t in got] == ["s", ""]
    assert _words([[9, 0, 4], [9, 4, 4]], 8) == [] and _words(np.zeros((0, 3), np.int32), 0) == []      # blanks never appear
    got = _words([[0, 1, 2]], 10, spf=0.04)
    assert got[0][0] == np.float32(0.04) and got[0][1] == np.float32(0.12)


def test_words_end_is_clamped_at_the_clip():
    got = _words([[0, 5, 1], [1, 6, 4]], 8)      # 6 + 4 passes T' = 8 by two frames
    assert got[0][1] == np.float32(8 * 0.08)
    got = _words([[2, 7, 4]], 8)
    assert got[0][0] == np.float32(7 * 0.08) and got[0][1] == np.float32(8 * 0.08)


def test_words_buffer_sizes_and_refusals():
    N, L = _lib()
    steps = np.array([[0, 0, 1], [1, 1, 2], [2, 4, 0], [3, 4, 3], [5, 8, 1]], np.int32)
    raw = (C.c_char_p * len(PIECES))(*[p.encode() for p in PIECES])
    need = C.c_long(-1)
    args = (steps.ctypes.data, len(steps), 20, BLANK, raw, len(PIECES), 0.08)
    texts = b"hello\0world\0" + "日本".encode() + b"\0"
    assert L.crispy_pk_tdt_words(*args, None, None, None, 0, None, 0, C.byref(need)) == 3 and need.value == len(texts) == 19
    start, end, off = np.full(3, -1, np.float32), np.full(3, -1, np.float32), np.full(3, -1, np.int64)
    text = C.create_string_buffer(b"\xff" * 32, 32)
    for words_cap, text_cap in ((2, 32), (3, 18), (0, 0)):      # too few records, too few bytes: the sizes come back, nothing is written
        need.value = -1
        assert L.crispy_pk_tdt_words(*args, start.ctypes.data, end.ctypes.data, off.ctypes.data, words_cap, text, text_cap, C.byref(need)) == 3
        assert need.value == 19 and (start == -1).all() and (off == -1).all() and text.raw == b"\xff" * 32
    assert L.crispy_pk_tdt_words(*args, start.ctypes.data, end.ctypes.data, off.ctypes.data, 3, text, 19, None) == 3
    assert text.raw[:19] == texts and text.raw[19:] == b"\xff" * 13 and list(off) == [0, 6, 12]
    assert np.array_equal(end, np.array([3, 7, 9], np.float64).astype(np.float32) * 0 + (np.array([3, 7, 9]) * 0.08).astype(np.float32))
    for bad, word in (((steps.ctypes.data, -1, 20, BLANK, raw, len(PIECES), 0.08), b"n_steps"), ((None, 2, 20, BLANK, raw, len(PIECES), 0.08), b"steps is NULL"),
                      ((steps.ctypes.data, 5, 20, BLANK, None, len(PIECES), 0.08), b"pieces"), ((steps.ctypes.data, 5, -1, BLANK, raw, len(PIECES), 0.08), b"frames"),
                      ((steps.ctypes.data, 5, 20, BLANK, raw, len(PIECES), 0.0), b"seconds_per_frame"),
                      ((steps.ctypes.data, 5, 20, BLANK, raw, 5, 0.08), b"token 5")):
        assert L.crispy_pk_tdt_words(*bad, None, None, None, 0, None, 0, None) == -1 and word in L.crispy_last_error(), word

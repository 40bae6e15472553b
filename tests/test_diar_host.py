"""CPU tests of the host functions of the speaker clustering (crispy_diar_chunk_plan / _speaker_segments / _find_speaker /
_format_text / _format_result, include/crispy_hip.h) through ctypes on the built library: against the numpy restatement
(tests/nme_sc_oracle.py) and against hand-written strings.  The device entry points validate their arguments without
touching a device."""
import ctypes as C
import os
import re

import numpy as np

from crispy_amd import _native as N
from crispy_amd import diarize as D
from tests import nme_sc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_in_header_binding_and_rust():
    hdr = open(os.path.join(ROOT, "include", "crispy_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    L = N.lib()
    assert len(N.DIAR_SYMBOLS) == 14
    for name in N.DIAR_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and ("pub fn %s(" % name) in rs, name
        assert name in N.ALL_SYMBOLS and hasattr(L, name) and getattr(L, name).argtypes, name
    assert "CRISPY_ERR_INTERNAL = -8" in hdr and "pub const CRISPY_ERR_INTERNAL: c_int = -8;" in rs and N.ERR_INTERNAL == -8
    assert "#define CRISPY_ABI_VERSION 6" in hdr and L.crispy_abi_version() == 6
    # crispy_diar_info: the same scalar fields, in order, in the header, the ctypes mirror and the Rust struct
    fields = ["p_star", "k", "ratio", "gap", "p_max"]
    body = re.search(r"typedef struct crispy_diar_info \{(.*?)\} crispy_diar_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(?:int|float) (\w+);", body) == fields
    assert [f[0] for f in N.DiarInfo._fields_] == fields and C.sizeof(N.DiarInfo) == 20
    rbody = re.search(r"pub struct crispy_diar_info \{(.*?)\n\}", rs, re.S).group(1)
    assert re.findall(r"pub (\w+):", rbody) == fields


def test_device_entry_points_validate_before_any_device_work():
    L = N.lib()
    n = (C.c_int * 1)(3)
    emb = np.zeros((3, 4), np.float32)
    lab = np.zeros(3, np.int32)
    assert L.crispy_diar_create(0, None) == -1
    assert L.crispy_diar_cluster(None, emb.ctypes.data, n, 1, 4, 8, lab.ctypes.data, None) == -1
    assert b"NULL handle" in L.crispy_last_error()
    assert L.crispy_diar_cluster_device(None, None, n, 1, 4, 8, None, None, None) == -1
    assert L.crispy_diar_affinity_device(None, None, 3, 4, None) == -1
    assert L.crispy_diar_laplacian_device(None, None, 3, 1, None) == -1
    assert L.crispy_diar_eigh_device(None, None, 3, 1, None, None) == -1
    assert L.crispy_diar_decide_device(None, None, 3, 1, 8, None) == -1 and b"NULL handle" in L.crispy_last_error()
    assert L.crispy_diar_kmeans_device(None, None, 3, 2, None, None, None) == -1 and b"NULL handle" in L.crispy_last_error()
    L.crispy_diar_destroy(None)
    if L.crispy_device_count() == 0:
        h = C.c_void_p()
        assert L.crispy_diar_create(0, C.byref(h)) == -2 and not h      # no device: no CPU path


def test_chunk_plan_matches_the_oracle():
    segs = [(0.0, 3.0, 48000), (5.0, 9.0, 64000), (10.0, 14.5, 72000), (20.0, 33.3, 212801), (40.0, 40.0, 0),
            (50.0, 54.000001, 64001), (60.0, 69.0, 7)]
    got = D.chunk_plan(segs, 16000)
    want = O.chunk_plan(segs, 16000)
    assert got == want
    assert len(got) == 1 + 1 + 2 + 4 + 1 + 2 + 3
    assert got[2] == (10.0, 10.0 + 36000 / 16000, 2, 0, 36000) and got[3][3:] == (36000, 36000)
    assert got[7][3:] == (3 * 53200, 212801 - 3 * 53200)             # the last chunk takes the rest
    assert [g[4] for g in got[-3:]] == [2, 2, 3]                    # 7 samples in 3 chunks
    assert D.chunk_plan([]) == []
    L = N.lib()
    bad = (C.c_double * 1)(float("nan"))
    one = (C.c_double * 1)(1.0)
    ns = (C.c_long * 1)(5)
    assert L.crispy_diar_chunk_plan(bad, one, ns, 1, 16000, None, None, None, None, None, 0) == -1
    assert L.crispy_diar_chunk_plan(one, one, ns, 1, 0, None, None, None, None, None, 0) == -1


def test_speaker_segments_relabel_sort_and_merge():
    # labels in order of appearance: 2 -> Speaker 1, 0 -> Speaker 2, 1 -> Speaker 3
    starts = [0.0, 1.1, 2.5, 9.0, 4.0, 4.5]
    ends = [1.0, 2.0, 3.0, 9.5, 6.0, 5.0]
    labels = [2, 2, 0, 1, 0, 0]
    got = D.speaker_segments(starts, ends, labels, 0.5)
    assert got == O.speaker_segments(starts, ends, labels, 0.5)
    # 2.5-3.0 / 4.0-6.0 are 1.0 apart (> 0.5): not merged; 4.5-5.0 lies inside 4.0-6.0: the gap is max(-1.5, 0), the end stays 6.0
    assert got == [(0.0, 2.0, 1), (2.5, 3.0, 2), (4.0, 6.0, 2), (9.0, 9.5, 3)]
    # the reference's own tests (:852-887)
    assert D.speaker_segments([0.0, 1.1], [1.0, 2.0], [0, 0], 0.5) == [(0.0, 2.0, 1)]
    assert len(D.speaker_segments([0.0, 1.1], [1.0, 2.0], [0, 1], 0.5)) == 2
    assert len(D.speaker_segments([0.0, 5.0], [1.0, 6.0], [0, 0], 0.5)) == 2
    assert D.speaker_segments([], [], [], 0.5) == []
    # equal starts keep their order (stable sort); the first to SPEAK in the input is Speaker 1 even when it starts later
    assert D.speaker_segments([3.0, 1.0, 1.0], [4.0, 2.0, 1.5], [7, 5, 7], 0.0) == [(1.0, 2.0, 2), (1.0, 1.5, 1), (3.0, 4.0, 1)]
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(1, 30))
        s = np.round(rng.uniform(0, 50, n), 1)
        e = s + np.round(rng.uniform(0, 4, n), 1)
        lb = rng.integers(0, 4, n)
        gap = float(rng.choice([0.0, 0.3, 1.0]))
        assert D.speaker_segments(s, e, lb, gap) == O.speaker_segments(list(s), list(e), list(lb), gap)


def test_find_speaker():
    two = [(0.0, 5.0, 1), (5.5, 10.0, 2)]
    assert D.find_speaker(2.5, two) == 1 and D.find_speaker(7.0, two) == 2            # :891-899
    assert D.find_speaker(0.0, [(0.0, 5.0, 1)]) == 1 and D.find_speaker(5.0, [(0.0, 5.0, 1)]) == 1
    gap = [(0.0, 3.0, 1), (7.0, 10.0, 2)]
    assert D.find_speaker(4.0, gap) == 1 and D.find_speaker(6.0, gap) == 2            # :911-921
    assert D.find_speaker(5.0, gap) == 1                                              # equal distances: the first
    assert D.find_speaker(-3.0, gap) == 1 and D.find_speaker(99.0, gap) == 2
    assert D.find_speaker(1.0, []) == 0 and D.speaker_name(0) == "Speaker ?"
    assert D.find_speaker(2.0, [(0.0, 3.0, 4), (1.0, 5.0, 9)]) == 4                   # overlapping: the first that holds it
    rng = np.random.default_rng(6)
    segs = [(float(a), float(a + b), int(w)) for a, b, w in zip(rng.uniform(0, 20, 8), rng.uniform(0, 3, 8), rng.integers(1, 4, 8))]
    for t in rng.uniform(-2, 25, 50):
        assert D.find_speaker(float(t), segs) == O.find_speaker(float(t), segs)


def test_format_text_reference_cases():
    assert D.format_diarized_text([(0.0, 0.5, "Hello"), (0.5, 1.0, "world")], []) == "Hello world"      # :925-933
    assert D.format_diarized_text([], []) == ""
    assert D.format_diarized_text([], [(0.0, 1.0, 1)]) == ""
    words = [(0.0, 0.5, "Hello"), (0.5, 1.0, "there"), (5.0, 5.5, "Hi")]
    segs = [(0.0, 2.0, 1), (4.0, 7.0, 2)]
    assert D.format_diarized_text(words, segs) == "[Speaker 1|0.0]\nHello there\n\n[Speaker 2|5.0]\nHi"
    words = [(0.0, 0.5, "Hello"), (0.5, 1.0, "  "), (1.0, 1.5, "world")]
    assert D.format_diarized_text(words, [(0.0, 2.0, 1)]) == "[Speaker 1|0.0]\nHello world"              # :959-972
    # without segments the texts are joined as they are, blank ones included
    assert D.format_diarized_text([(0, 1, " a "), (1, 2, ""), (2, 3, "b")], []) == " a   b"


def test_format_text_rounding_white_space_and_gaps():
    segs = [(0.0, 1.0, 1), (1000.0, 2000.0, 2)]
    # {:.1}: the exact decimal value of the f64, half to even -- 0.05 is above its decimal, 0.25 is exact, 0.15 below
    for t0, want in ((0.05, "0.1"), (0.15, "0.1"), (0.25, "0.2"), (0.35, "0.3"), (0.75, "0.8"), (2.5, "2.5"), (0.0, "0.0"),
                     (1234.25, "1234.2"), (1234.75, "1234.8"), (99999.96, "100000.0"), (1e15 + 0.25, "1000000000000000.2")):
        got = D.format_diarized_text([(t0, t0, "w")], [(0.0, 1e16, 1)])
        assert got == "[Speaker 1|%s]\nw" % want, (t0, got)
        assert got == O.format_diarized_text([(t0, t0, "w")], [(0.0, 1e16, 1)])
    # NBSP and U+3000 are Rust white space: trimmed off words, a word made of them is blank; U+200B is not
    words = [(0.0, 0.2, "\u00a0Hello\u3000"), (0.2, 0.4, "\u3000\u00a0"), (0.4, 0.6, " \u200b "), (0.6, 0.8, "\tworld\n")]
    got = D.format_diarized_text(words, segs)
    assert got == "[Speaker 1|0.0]\nHello \u200b world" and got == O.format_diarized_text(words, segs)
    # a midpoint in the gap between segments goes to the closest one; the header shows the word's START
    words = [(0.5, 0.9, "a"), (400.0, 402.0, "b"), (600.0, 700.0, "c"), (1500.0, 1501.0, "d")]
    got = D.format_diarized_text(words, segs)
    assert got == "[Speaker 1|0.5]\na b\n\n[Speaker 2|600.0]\nc d" and got == O.format_diarized_text(words, segs)
    # all words blank: only nothing is left after the outer trim
    assert D.format_diarized_text([(0.0, 1.0, " "), (1.0, 2.0, " ")], segs) == ""
    # speaker changes back and forth, multi-byte text
    words = [(0.0, 0.4, " Добрый"), (0.4, 0.9, " день"), (1200.0, 1201.0, " 你好"), (0.9, 1.0, " да")]
    got = D.format_diarized_text(words, segs)
    assert got == "[Speaker 1|0.0]\nДобрый день\n\n[Speaker 2|1200.0]\n你好\n\n[Speaker 1|0.9]\nда"
    assert got == O.format_diarized_text(words, segs)


def test_format_text_buffer_protocol():
    L = N.lib()
    t = (C.c_double * 1)(0.0)
    txt = (C.c_char_p * 1)(b"hello")
    need = C.c_size_t(0)
    assert L.crispy_diar_format_text(t, t, txt, 1, None, None, None, 0, None, 0, C.byref(need)) == 0 and need.value == 6
    small = C.create_string_buffer(3)
    assert L.crispy_diar_format_text(t, t, txt, 1, None, None, None, 0, small, 3, C.byref(need)) == -1 and need.value == 6
    assert small.value == b""
    buf = C.create_string_buffer(6)
    assert L.crispy_diar_format_text(t, t, txt, 1, None, None, None, 0, buf, 6, None) == 0 and buf.value == b"hello"
    assert L.crispy_diar_format_text(t, t, None, 1, None, None, None, 0, buf, 6, None) == -1
    assert L.crispy_diar_format_text(t, t, txt, 1, None, None, None, 2, buf, 6, None) == -1      # segments announced, none given


def test_format_result_takes_the_words_of_an_asr_result():
    words = (N.AsrWord * 3)()
    for w, (t0, t1, text) in zip(words, ((0.0, 0.5, b" Hello"), (0.5, 1.0, b" there"), (5.0, 5.5, b" Hi"))):
        w.t0, w.t1, w.text = t0, t1, text
    r = N.AsrResult()
    r.n_words = 3
    r.words = C.cast(words, C.c_void_p)
    segs = [(30.0, 32.0, 1), (34.0, 37.0, 2)]
    assert D.format_result(C.byref(r), 30.0, segs) == "[Speaker 1|30.0]\nHello there\n\n[Speaker 2|35.0]\nHi"
    assert D.format_result(C.byref(r), 0.0, []) == " Hello  there  Hi"
    empty = N.AsrResult()
    assert D.format_result(C.byref(empty), 0.0, segs) == ""
    assert N.lib().crispy_diar_format_result(None, 0.0, None, None, None, 0, None, 0, None) == -1

"""The word-alignment oracle (tests/align_oracle.py) against HF transformers' own median filter and DTW, and its word
split / punctuation merge on a written vocabulary; the alignment kernels' resource budget (no GPU needed)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import align_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _hf():
    pytest.importorskip("transformers")
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter
    return _dynamic_time_warping, _median_filter


@pytest.mark.parametrize("seed,shape", [(0, (6, 40)), (1, (17, 90)), (2, (3, 9))])
def test_median_filter_and_dtw_match_transformers_on_random_matrices(seed, shape):
    import torch
    hf_dtw, hf_med = _hf()
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2,) + shape)
    mine = AO.median_filter(x, 7)
    theirs = hf_med(torch.from_numpy(x), 7).numpy()
    assert np.array_equal(mine, theirs)
    m = rng.standard_normal(shape).astype(np.float32)
    ti, tj = AO.dtw(-m)
    hi, hj = hf_dtw(-m.astype(np.float64))
    assert np.array_equal(ti, hi) and np.array_equal(tj, hj)


@pytest.mark.parametrize("kind", ["zeros", "constant_rows", "constant_cols", "two_values"])
def test_dtw_ties_match_transformers(kind):
    hf_dtw, _ = _hf()
    n, m = 7, 23
    if kind == "zeros":
        x = np.zeros((n, m), np.float32)
    elif kind == "constant_rows":
        x = np.repeat(np.arange(n, dtype=np.float32)[:, None], m, 1)
    elif kind == "constant_cols":
        x = np.repeat(np.arange(m, dtype=np.float32)[None, :] % 3, n, 0)
    else:
        x = (np.indices((n, m)).sum(0) % 2).astype(np.float32)
    ti, tj = AO.dtw(x)
    hi, hj = hf_dtw(x.astype(np.float64))
    assert np.array_equal(ti, hi) and np.array_equal(tj, hj)
    assert len(AO.jump_indices(ti, tj)) == n


def test_word_split_and_punctuation_merge_on_a_written_vocabulary():
    euro = "€".encode()
    pieces = [b" Hello", b",", b" wor", b"ld", b" (", b"costs", b" 5", euro[:2], euro[2:], b")", b".", b" \"", b"ok", b"\""]
    words = AO.split_words(pieces)
    # " (" is punctuation once stripped: a word of its own, which "costs" (no space) then continues
    assert [w[0] for w in words] == [" Hello", ",", " world", " (costs", " 5€", ")", ".", " \"ok", "\""]
    assert [(w[1], w[2]) for w in words] == [(0, 1), (1, 1), (2, 2), (4, 2), (6, 3), (9, 1), (10, 1), (11, 2), (13, 1)]
    idx = list(range(0, 2 * (len(pieces) + 1), 2))
    ww = AO.window_words(pieces, idx, 100)
    assert [w[2] for w in ww] == [" Hello,", " world", " (costs", " 5€).", " \"ok\""]
    assert [(w[3], w[4]) for w in ww] == [(0, 2), (2, 2), (4, 2), (6, 5), (11, 3)]
    # a merged word keeps the times of the word it was merged into; times = seek x 0.01 + index x 0.02
    assert ww[2][0] == AO.token_time(100, idx[4]) and ww[0][1] == AO.token_time(100, idx[1])
    # languages without spaces: every UTF-8 unit is a word (the split character stays whole)
    assert [w[0] for w in AO.split_words([b"\xe4\xbd", b"\xa0", b"\xe5\xa5\xbd"], unicode_only=True)] == ["你", "好"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_alignment_kernels_have_no_scratch_and_no_scalar_stores(tmp_path):
    """The project's rule for every ASR kernel (test_build_resources.py): ScratchSize 0, no spilled VGPR; the three
    alignment kernels are there under readable names."""
    src = os.path.join(ROOT, "crispy_amd", "csrc", "whisper_align.hip")
    text = open(os.path.join(ROOT, "crispy_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    flags = [f for f in flags if f != "-fPIC" and not f.startswith("-W")] + ["-Wno-unused-function"]
    asm = tmp_path / "a.s"
    out = subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(asm)],
                         capture_output=True, text=True, timeout=900, cwd=os.path.dirname(src))
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    for must in ("align_rowstats_kernel", "align_matrix_kernel", "align_dtw_kernel"):
        assert sum(must in k for k in res) == 1, (must, list(res))
    bad = {k: r for k, r in res.items() if r.get("ScratchSize", 0) != 0 or r.get("VGPRs Spill", 0) != 0}
    assert not bad, bad
    s = asm.read_text()
    assert "scratch_store" not in s and "scratch_load" not in s
    assert not re.search(r"\bs_(buffer_|scratch_)?(store|atomic)", s)

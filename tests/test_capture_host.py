"""CPU tests of the capture callbacks' host side (crispy_rn_capture* / crispy_rn_bypass_configure /
crispy_rn_record_app_push_at*, include/crispy_hip.h): the entry points validate without a device, the bindings know them,
tests/capture_oracle.py gives hand-checked vectors, and the kernels of rn_capture.hip (cross-compiled here) use no scratch and
contract no multiply-add."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import capture_oracle as CO
from tests import record_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("crispy_rn_bypass_configure", "crispy_rn_capture_out_len", "crispy_rn_capture_device", "crispy_rn_capture",
         "crispy_rn_record_app_push_at_device", "crispy_rn_record_app_push_at")
BRANCH_44K, BRANCH_N, NO_BRANCH_N = CO.BRANCH_44K, CO.BRANCH_N, CO.NO_BRANCH_N      # hard-coded there, searched for below
f = np.float32


def _lib():
    from crispy_amd import _native as N
    return N.lib()


# ---- 1 -------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_without_a_device():
    L = _lib()
    n = C.c_long(7)
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    calls = {
        "crispy_rn_bypass_configure": lambda: L.crispy_rn_bypass_configure(None, 44100.0),
        "crispy_rn_capture_out_len": lambda: L.crispy_rn_capture_out_len(None, 480),
        "crispy_rn_capture_device": lambda: L.crispy_rn_capture_device(None, p, 4, 2, 2, 1, p, 16, p, 4, p, C.byref(n), None),
        "crispy_rn_capture": lambda: L.crispy_rn_capture(None, p, 4, 2, 2, 1, p, 16, p, C.byref(n)),
        "crispy_rn_record_app_push_at_device": lambda: L.crispy_rn_record_app_push_at_device(None, p, 4, 2, 2, 44100, None),
        "crispy_rn_record_app_push_at": lambda: L.crispy_rn_record_app_push_at(None, p, 4, 2, 2, 44100),
    }
    assert set(calls) == set(NAMES)
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.crispy_last_error().decode()
        assert msg.startswith(name + ":") and "NULL handle" in msg, (name, msg)
    assert n.value == 7 and not any(buf)
    assert L.crispy_abi_version() == 6          # new entry points only: no struct grew, no argument changed meaning


def test_names_are_bound_and_declared():
    from crispy_amd import _native as N
    from crispy_amd.denoise import CaptureBuffers, DenoiseState
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "crispy_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in N.RN_SYMBOLS and name in N.ALL_SYMBOLS
        assert getattr(L, name).argtypes, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    assert L.crispy_rn_capture_out_len.restype is C.c_long
    assert re.search(r"#define CRISPY_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6
    for m in ("capture", "capture_device", "capture_out_len", "bypass_configure", "record_app_push"):
        assert callable(getattr(DenoiseState, m)), m
    import inspect
    assert "from_rate" in inspect.signature(DenoiseState.record_app_push).parameters
    for m in ("push_mono", "push_mono_block", "capture_block"):
        assert callable(getattr(CaptureBuffers, m)), m


# ---- 2 -------------------------------------------------------------------------------------------------------------
def test_oracle_conversions_and_mic_downmix_by_hand():
    assert CO.convert(np.array([[-32768, 32767, 0, 1]], np.int16)).tolist() == [[-1.0, 32767 / 32768, 0.0, 1 / 32768]]
    assert CO.convert(np.array([[0, 32768, 65535, 32767]], np.uint16)).tolist() == [[-1.0, 0.0, 32767 / 32768, -1 / 32768]]
    x = np.array([[0.25, -0.0]], np.float32)
    assert CO.convert(x) is x
    # the mic path sums from +0.0 for one channel too: -0.0 becomes +0.0; the app handlers' downmix keeps it
    mono = CO.capture_mono(np.array([[-0.0, 0.5]], np.float32), 1)
    assert mono.tolist() == [[0.0, 0.5]] and not np.signbit(mono[0, 0])
    assert np.signbit(RO.downmix(np.array([[-0.0]], np.float32), 1)[0, 0])
    # two channels: (0.0 + a + b) / 2.0 -- the same value as the app handlers' (a + b) / 2.0 except for the sign of a zero
    assert CO.capture_mono(np.array([[-0.0, -0.0]], np.float32), 2).tobytes() == np.array([[0.0]], np.float32).tobytes()
    assert RO.downmix(np.array([[-0.0, -0.0]], np.float32), 2).tobytes() == np.array([[-0.0]], np.float32).tobytes()
    # three channels whose order matters: ((0 + 1) + 2^-24) + 2^-24 = 1, but ((0 + 2^-24) + 2^-24) + 1 = 1 + 2^-23
    tiny = f(2.0) ** f(-24)
    a = CO.capture_mono(np.array([[1.0, tiny, tiny]], np.float32), 3)
    b = CO.capture_mono(np.array([[tiny, tiny, 1.0]], np.float32), 3)
    assert a[0, 0] == f(1.0) / f(3) and b[0, 0] == (f(1.0) + f(2.0) ** f(-23)) / f(3) and a[0, 0] != b[0, 0]
    # i16 stereo: conversion first, then the sum, then the division
    got = CO.capture_mono(np.array([[32767, -32768, 3, 5]], np.int16), 2)
    assert got.tolist() == [[(f(0) + f(32767 / 32768) + f(-1.0)) / f(2), (f(0) + f(3 / 32768) + f(5 / 32768)) / f(2)]]
    for ch in range(1, 9):              # every channel count: one operation per Rust operation
        x = np.random.default_rng(ch).uniform(-1, 1, size=(2, 5 * ch)).astype(np.float32)
        want = np.zeros((2, 5), np.float32)
        for c in range(ch):
            want = want + x[:, c::ch]
        assert CO.capture_mono(x, ch).tobytes() == (want / f(ch)).tobytes()


def test_oracle_resample_audio_by_hand():
    s = np.random.default_rng(3).uniform(-1, 1, size=(2, 441)).astype(np.float32)
    out = CO.resample_audio(s, 44100)
    assert out.shape == (2, 480) and out[:, 0].tobytes() == s[:, 0].tobytes()
    ratio = 44100.0 / 48000.0
    frac = f(1 * ratio - 0.0)
    assert out[:, 1].tobytes() == (s[:, 0] + (s[:, 1] - s[:, 0]) * frac).tobytes()
    assert CO.resample_audio(s, 48000).tobytes() == s.tobytes()
    # one sample: two outputs, both the sample (src_index 0, nothing to interpolate with)
    one = CO.resample_audio(s[:, :1], 44100)
    assert one.shape == (2, 2) and (one == s[:, :1]).all()
    # decimation: every other sample exactly
    assert CO.resample_audio(s[:, :8], 96000).tobytes() == np.ascontiguousarray(s[:, 0:8:2]).tobytes()
    # the branch `src_index + 1 == n` at the end of a buffer, searched here and hard-coded for the GPU test.  Upsampling
    # (ratio < 1) ends every buffer with it: the last position lies above n - ratio > n - 1.  Decimating by two ends the odd
    # lengths with it and the even ones with an interpolation.
    for rate in (44100, 32000):
        assert all(CO.last_output_takes_the_copy_branch(n, rate) for n in range(1, 2000)), rate
    hits = [n for n in range(1000, 1030) if CO.last_output_takes_the_copy_branch(n, 96000)]
    assert hits == list(range(1001, 1030, 2))
    assert BRANCH_N in hits and CO.last_output_takes_the_copy_branch(BRANCH_44K, 44100) and NO_BRANCH_N not in hits
    b = CO.resample_audio(s, 44100)
    assert b[:, -1].tobytes() == s[:, BRANCH_44K - 1].tobytes() and b[:, -2].tobytes() != s[:, BRANCH_44K - 1].tobytes()
    t = np.random.default_rng(4).uniform(-1, 1, size=(2, BRANCH_N)).astype(np.float32)
    assert CO.resample_audio(t, 96000)[:, -1].tobytes() == t[:, BRANCH_N - 1].tobytes()
    assert CO.resample_audio(t[:, :NO_BRANCH_N], 96000)[:, -1].tobytes() == t[:, NO_BRANCH_N - 2].tobytes()      # frac == 0


def test_bypass_oracle_equals_the_per_sample_capture_buffers():
    """The vectorised bypass oracle against `CaptureBuffers.push_mono(ns=None)`, the per-sample form, stream by stream."""
    from crispy_amd.denoise import CaptureBuffers
    B = 2
    x = np.random.default_rng(8).uniform(-1, 1, size=(B, 700)).astype(np.float32)
    for rate in (44100.0, 16000.0, 47999.5, 48000.0):
        orc = CO.BypassOracle(B, rate, RO.RecordOracle(B, 1000))
        outs = [orc.capture(x[:, a:b]) for a, b in ((0, 1), (1, 3), (3, 444), (444, 700))]
        got = np.concatenate(outs, axis=1)
        for b in range(B):
            cb = CaptureBuffers()
            cb.max_len = 1000
            for v in x[b]:
                cb.push_mono(v, None, rate)
            want_ring = np.array(cb.rec_buffer, np.float32)
            assert np.array([r[b] for r in orc.rec.mic], np.float32).tobytes() == want_ring.tobytes(), (rate, b)
            if got.shape[1] <= 1000:
                assert got[b].tobytes() == want_ring.tobytes(), (rate, b)
            else:
                assert got[b, -1000:].tobytes() == want_ring.tobytes(), (rate, b)
        if abs(rate - 48000.0) < 1.0:
            assert got.tobytes() == x.tobytes()


# ---- 3 -------------------------------------------------------------------------------------------------------------
def _kernel_sections(isa):
    """{mangled name: its instructions} of an AMDGPU assembly listing."""
    out, cur = {}, None
    for line in isa.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and re.match(r"^\s+(s_endpgm)\b", line):
            out[cur].append(line)
            cur = None
        elif cur:
            out[cur].append(line)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_capture_kernels_have_no_scratch_and_contract_nothing(tmp_path):
    """The method of tests/test_record_host.py: the listing is the same, instruction for instruction, when contraction is
    switched off for the whole compilation, so the fused operations left over are those of the correctly rounded divisions.
    The kernels that divide by nothing but a power of two hold no fused multiply-add at all."""
    text = open(os.path.join(ROOT, "crispy_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", text, re.M).group(1).split()
    assert "rn_capture.hip" in srcs and "rn_capture_io.cpp" in srcs
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    assert not any("fast" in x or "contract" in x or "unsafe" in x or "approx" in x for x in flags), flags
    flags = [x for x in flags if x != "-fPIC" and not x.startswith("-W")]
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_capture.hip")

    def compile_to(asm, extra=()):
        out = subprocess.run([HIPCC, *flags, *extra, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(asm)],
                             capture_output=True, text=True, timeout=600, cwd=os.path.dirname(src))
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stderr, asm.read_text()

    remarks, isa = compile_to(tmp_path / "cap.s")
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    # the capture kernel in three formats x (fallback, 16-byte loads for 1, 2, 4 channels and, 16-bit only, 8), the bypass
    # resampler with and without positions, the app pass
    count = lambda word: sum(word in k for k in res)
    assert (count("rn_capture_kernel"), count("rn_capture_resample_kernel"), count("rn_rec_app_at_kernel"), len(res)) == (14, 2, 1, 17), list(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (name, r)
    sec = _kernel_sections(isa)
    assert set(sec) == set(res)
    fma = r"\bv_(fma|fmac|mad|mac|pk_fma)_(f32|f16|f64|legacy|mix)"
    for name, lines in sec.items():
        body = "\n".join(lines)
        if "rn_capture_resample_kernel" in name or re.search(r"rn_capture_kernelILi\d+ELi[1248]E", name):
            assert not re.search(fma, body), f"a fused multiply-add in {name}"
        else:
            assert "v_div_fixup_f32" in body, name                     # the division by a channel count known at run time
    resample = next(v for k, v in sec.items() if "rn_capture_resample_kernelILb1E" in k)
    assert any("v_sub_f32" in ln for ln in resample) and any("v_mul_f32" in ln for ln in resample) and any("v_add_f32" in ln for ln in resample)
    at = "\n".join(next(v for k, v in sec.items() if "rn_rec_app_at_kernel" in k))
    assert "v_mul_f64" in at and "v_floor_f64" in at and "v_cvt_f32_f64" in at and not re.search(r"\bv_fma_f64", at)
    # no contraction anywhere: compiled with contraction off for everything, the listing is the same
    _, isa_off = compile_to(tmp_path / "cap_off.s", extra=("-ffp-contract=off",))
    strip = lambda s: [ln for ln in s.splitlines() if "__hip_cuid" not in ln]        # (a hash of the command line)
    assert strip(isa) == strip(isa_off), "rn_capture.hip contracts a multiply-add somewhere"

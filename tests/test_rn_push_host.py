"""CPU tests of the capture-rate adapter's host side (crispy_rn_push*, include/crispy_hip.h): the pure counting function
crispy_linear_resampler_count against the Python mirror of the reference's LinearResampler (audio.rs:73-134), and the two
adapter kernels' ISA (cross-compiled here): no scratch, and the interpolation's multiply and add not fused."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RATES = (8000.0, 16000.0, 44100.0, 47999.0, 48000.0, 48000.5, 96000.0)
COUNTS = (0, 1, 2, 479, 480, 4410)


def _lib():
    from crispy_amd import _native as N
    return N.lib()


@pytest.fixture(scope="module")
def emitted():
    """emitted[rate][n] = samples a fresh denoise.LinearResampler(rate, 48000) has emitted after n inputs, n <= 2 x 4410."""
    from crispy_amd.denoise import LinearResampler
    table = {}
    for rate in RATES:
        rs, out, acc = LinearResampler(rate, 48000.0), [], [0]
        for i in range(2 * max(COUNTS)):
            rs.process_sample(0.25 if i & 1 else -0.5, out.append)
            acc.append(len(out))
        table[rate] = acc
    return table


@pytest.mark.parametrize("rate", RATES)
def test_count_matches_the_python_resampler(emitted, rate):
    L = _lib()
    acc = emitted[rate]
    for n_before, n_in in itertools.product(COUNTS, COUNTS):
        got = L.crispy_linear_resampler_count(rate, 48000.0, n_before, n_in)
        assert got == acc[n_before + n_in] - acc[n_before], (rate, n_before, n_in, got)


@pytest.mark.parametrize("rate", RATES)
def test_count_is_additive(rate):
    L = _lib()
    for a, b in itertools.product(COUNTS, COUNTS):
        whole = L.crispy_linear_resampler_count(rate, 48000.0, 0, a + b)
        assert whole == L.crispy_linear_resampler_count(rate, 48000.0, 0, a) + L.crispy_linear_resampler_count(rate, 48000.0, a, b)


def test_count_passes_through_within_one_hertz():
    L = _lib()
    for rate in (48000.0, 48000.5, 47999.5):
        for n_before, n_in in itertools.product(COUNTS, COUNTS):
            assert L.crispy_linear_resampler_count(rate, 48000.0, n_before, n_in) == n_in
    # one whole hertz away the resampler is in: the first sample only primes it
    assert L.crispy_linear_resampler_count(47999.0, 48000.0, 0, 1) == 0
    assert L.crispy_linear_resampler_count(48001.0, 48000.0, 0, 1) == 0


def test_count_rejects_negative_arguments():
    L = _lib()
    assert L.crispy_linear_resampler_count(44100.0, 48000.0, -1, 10) < 0
    assert b"crispy_linear_resampler_count" in L.crispy_last_error()
    assert L.crispy_linear_resampler_count(44100.0, 48000.0, 10, -1) < 0
    assert L.crispy_linear_resampler_count(48000.0, 48000.0, 0, -1) < 0
    assert L.crispy_linear_resampler_count(-44100.0, 48000.0, 0, 10) < 0
    assert L.crispy_linear_resampler_count(44100.0, 0.0, 0, 10) < 0


def test_adapter_entry_points_validate_without_a_device():
    import ctypes as C
    L = _lib()
    n = C.c_long(7)
    assert L.crispy_rn_adapter_configure(None, 44100.0, 1.0) == -1 and b"crispy_rn_adapter_configure" in L.crispy_last_error()
    assert L.crispy_rn_adapter_set_volume(None, 0.5) == -1
    assert L.crispy_rn_adapter_produced_rate_hz(None, None) == -1
    assert L.crispy_rn_push_out_len(None, 480) == -1
    assert L.crispy_rn_push_device(None, None, 0, 0, None, 0, None, 0, None, C.byref(n), None) == -1
    assert b"crispy_rn_push_device" in L.crispy_last_error()
    assert L.crispy_rn_push(None, None, 0, 0, None, 0, None, C.byref(n)) == -1
    assert L.crispy_abi_version() == 6


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_adapter_kernels_have_no_scratch_and_no_fused_multiply_add(tmp_path):
    """Rust rounds `last + (sample - last) * t` twice; a fused multiply-add would round once and differ in the last bit.
    The two kernels do no other multiply-add, so no fused form may appear in the file at all."""
    text = open(os.path.join(ROOT, "crispy_amd", "csrc", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    flags = [f for f in flags if f != "-fPIC" and not f.startswith("-W")]
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_adapter.hip")
    asm = tmp_path / "ad.s"
    out = subprocess.run([HIPCC, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", str(asm)],
                         capture_output=True, text=True, timeout=600, cwd=os.path.dirname(src))
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
    assert sum("rn_adapt_in_kernel" in k for k in res) == 2 and sum("rn_adapt_out_kernel" in k for k in res) == 2, list(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r["VGPRs"] <= 32, (name, r)
    isa = asm.read_text()
    assert not re.search(r"\bv_(fma|fmac|mad|mac|pk_fma)_(f32|f16|legacy|mix)", isa), "a fused multiply-add in rn_adapter.hip"
    assert isa.count("v_sub_f32") >= 4 and not re.search(r"\bscratch_(load|store)", isa)

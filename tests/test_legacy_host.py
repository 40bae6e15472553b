"""CPU tests of the Legacy arm's host side (crispy_rn_model_configure / crispy_rn_model / crispy_ns_noise_state,
include/crispy_hip.h): the LCG jump-ahead that the host bookkeeping and the kernels share against a step-by-step LCG, the noise
values against numpy f32, the entry points' argument checks without a device, the two Python restatements of SharedAudio
against each other, and the ISA of rn_legacy.hip (cross-compiled here): no scratch, and no fused multiply-add -- the reference
rounds `x * volume`, `noise * 0.05` and every add on its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import legacy_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("crispy_rn_model_configure", "crispy_rn_model", "crispy_ns_noise_state")
STARTS = (0x1234ABCD, 0, 0xFFFFFFFF)
STEPS = (0, 1, 2, 3, 255, 256, 257, 4410, 70001, 1 << 24, (1 << 31) + 5)


def _lib():
    from crispy_amd import _native as N
    return N.lib()


def test_oracle_jump_ahead_is_the_step_by_step_lcg():
    for s in STARTS:
        for n in (0, 1, 2, 3, 255, 256, 257, 4410, 70001):
            assert LO.lcg_after(s, n) == LO.lcg_naive(s, n), (s, n)


@pytest.mark.parametrize("start", STARTS)
def test_noise_state_is_the_naive_lcg(start):
    L = _lib()
    naive, at = start, 0
    for n in STEPS:
        if n <= 70001:                    # step by step as far as a test can walk; beyond, the oracle's squaring (checked above)
            naive, at = LO.lcg_naive(naive, n - at), n
            want = naive
        else:
            want = LO.lcg_after(start, n)
        assert L.crispy_ns_noise_state(start, n, None) == want, (hex(start), n)


def test_noise_state_walks_when_it_writes_the_values_and_composes():
    L = _lib()
    n = 4410
    for start in STARTS + (0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFE):
        buf = np.full(n + 1, np.nan, dtype=np.float32)
        end = L.crispy_ns_noise_state(start, n, buf.ctypes.data)
        assert end == L.crispy_ns_noise_state(start, n, None) == LO.lcg_naive(start, n)
        assert np.isnan(buf[n])
        s, want = start, np.empty(n, dtype=np.float32)
        for k in range(n):
            s = (s * LO.LCG_A + LO.LCG_C) & 0xFFFFFFFF
            want[k] = np.float32(np.uint32(s)) / np.float32(4294967296) * 2 - 1
        assert want.dtype == np.float32 and np.array_equal(buf[:n].view(np.uint32), want.view(np.uint32)), hex(start)
    # composition: (a then b) equals (a + b), also across the 32-bit period
    for a, b in ((1, 1), (257, 4410), (70001, 1 << 24), ((1 << 31) + 5, (1 << 31) + 7), ((1 << 32) - 1, 3)):
        for start in STARTS:
            mid = L.crispy_ns_noise_state(start, a, None)
            assert L.crispy_ns_noise_state(mid, b, None) == L.crispy_ns_noise_state(start, a + b, None), (hex(start), a, b)


def test_a_state_from_0xffffff80_on_gives_exactly_plus_one():
    """`rng as f32` rounds to nearest even: from 0xffffff80 on the state rounds up to 2^32 and the noise is exactly +1.0,
    where a truncating conversion would stay below it.  The state in front of the hand-picked one is found by inverting
    the LCG (the multiplier is odd)."""
    L = _lib()
    inv = pow(LO.LCG_A, -1, 1 << 32)
    for target in (0xFFFFFF80, 0xFFFFFFFF, 0xFFFFFF7F, 0x80000000, 0):
        before = ((target - LO.LCG_C) * inv) & 0xFFFFFFFF
        v = np.zeros(1, dtype=np.float32)
        assert L.crispy_ns_noise_state(before, 1, v.ctypes.data) == target
        want = LO.noise_of(target)
        assert v[0].view(np.uint32) == want.view(np.uint32), hex(target)
        if target >= 0xFFFFFF80:
            assert v[0] == np.float32(1.0)
        elif target == 0xFFFFFF7F:
            assert v[0] < np.float32(1.0)
    assert LO.noise_of(0) == np.float32(-1.0) and LO.noise_of(0x80000000) == np.float32(0.0)


def test_entry_points_validate_without_a_device():
    L = _lib()
    model = C.c_int(7)
    calls = {
        "crispy_rn_model_configure": lambda: L.crispy_rn_model_configure(None, 1),
        "crispy_rn_model": lambda: L.crispy_rn_model(None, C.byref(model)),
        "crispy_ns_noise_state": lambda: L.crispy_ns_noise_state(-1, 1, None),
    }
    assert set(calls) == set(NAMES)
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.crispy_last_error().decode()
        assert msg.startswith(name + ":"), (name, msg)
    assert model.value == 7
    for args in ((1 << 32, 1), (0, -1)):
        assert L.crispy_ns_noise_state(*args, None) == -1 and L.crispy_last_error().decode().startswith("crispy_ns_noise_state:")
    # an unknown model and a NULL out-pointer are refused in front of everything that needs the device: a handle that is never
    # dereferenced stands in for a real one
    fake = C.c_void_p(0x1000)
    assert L.crispy_rn_model(fake, None) == -1 and L.crispy_last_error().decode().startswith("crispy_rn_model:")
    for bad in (3, -1):
        assert L.crispy_rn_model_configure(fake, bad) == -1
        msg = L.crispy_last_error().decode()
        assert msg.startswith("crispy_rn_model_configure:") and "unknown model" in msg, msg
    assert L.crispy_abi_version() == 6          # new entry points only: no struct grew, no argument changed meaning


def test_names_are_bound_and_declared():
    from crispy_amd import _native as N
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "crispy_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name in N.RN_SYMBOLS and name in N.ALL_SYMBOLS
        assert getattr(L, name).argtypes, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name
    assert L.crispy_ns_noise_state.restype is C.c_long
    for name, val in (("CRISPY_NS_RNNOISE", 0), ("CRISPY_NS_DUMMY", 1), ("CRISPY_NS_NOISY", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
        assert re.search(r"pub const %s: c_int = %d;" % (name, val), rs), name
    assert (N.NS_RNNOISE, N.NS_DUMMY, N.NS_NOISY) == (0, 1, 2)
    assert "pub fn set_model(&mut self" in rs


@pytest.mark.parametrize("model", ["dummy", "noisy"])
def test_the_two_restatements_of_shared_audio_agree(model):
    """crispy_amd.denoise.SharedAudio (per sample) and tests/legacy_oracle.py (per block), written apart: 3 streams x 5000
    samples at 44.1 -> 48 kHz with pulls in between, one of them running dry, and a volume change."""
    from crispy_amd.denoise import SharedAudio
    B, n = 3, 5000
    x = np.random.default_rng(7).uniform(-1.5, 1.5, size=(B, n)).astype(np.float32)
    mirror = SharedAudio(44100.0, 48000.0, model, 0.8, n_streams=B)
    orc = LO.SharedAudioOracle(B, 44100.0, 48000.0, model == "noisy", 0.8)
    pos = 0
    for k, (n_push, n_pull) in enumerate(((1, 3), (7, 2), (480, 400), (1025, 1300), (2000, 700), (1487, 2500))):
        if k == 3:
            mirror.volume = np.float32(0.37)
            orc.set_volume(0.37)
        blk = x[:, pos:pos + n_push]
        pos += n_push
        got = np.concatenate([mirror.push_sample(blk[:, i]) for i in range(n_push)], axis=0).T
        assert LO.same_bits(got, orc.push(blk)), ("push", k)
        got = np.stack([mirror.next_sample() for _ in range(n_pull)], axis=1)
        want, live = orc.pull(n_pull)
        assert LO.same_bits(got, want), ("pull", k)
        assert len(mirror.buffer) == len(orc) and mirror.rng_state == orc.rng and mirror.resample_pos == orc.pos
    assert pos == n and orc.zeros > 0 and orc.pops > 0
    assert (orc.rng != LO.LCG_SEED) == (model == "noisy")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_legacy_kernels_have_no_scratch_and_no_fused_multiply_add(tmp_path):
    text = open(os.path.join(ROOT, "crispy_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", text, re.M).group(1).split()
    assert "rn_legacy.hip" in srcs and "rn_legacy_io.cpp" in srcs
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    flags = [f for f in flags if f != "-fPIC" and not f.startswith("-W")]
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_legacy.hip")
    asm = tmp_path / "lg.s"
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
    # the push: (dummy, noisy) x (16-byte rows, fallback); the pull: three formats x (dummy, noisy) x (16-byte stores, fallback)
    assert sum("rn_legacy_push_kernel" in k for k in res) == 4 and sum("rn_legacy_pull_kernel" in k for k in res) == 12, list(res)
    assert not any("rn_pull_kernel" in k or "rn_ring_append_kernel" in k for k in res), list(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    isa = asm.read_text()
    assert not re.search(r"\bv_(fma|fmac|mad|mac|pk_fma)_(f32|f16|legacy|mix)", isa), "a fused multiply-add in rn_legacy.hip"
    assert isa.count("v_sub_f32") >= 12         # s1 - s0 of every pull kernel
    assert isa.count("v_cvt_f32_u32") >= 8      # `rng as f32` of every noisy kernel, to nearest even

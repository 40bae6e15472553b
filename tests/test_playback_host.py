"""CPU tests of the playback half's host side (crispy_rn_playback_* / crispy_rn_pull*, include/crispy_hip.h): the entry
points validate without a device, the binding knows them, and the kernels of rn_playback.hip (cross-compiled here) use no
scratch and hold no fused multiply-add -- next_sample's `s0 + (s1 - s0) * frac` and the u16 conversion's `s * 0.5 + 0.5`
round every operation in the reference."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
NAMES = ("crispy_rn_playback_configure", "crispy_rn_playback_buffered", "crispy_rn_pull_device", "crispy_rn_pull")


def _lib():
    from crispy_amd import _native as N
    return N.lib()


def test_entry_points_validate_without_a_device():
    L = _lib()
    live = C.c_long(7)
    buf = (C.c_float * 16)()
    calls = {
        "crispy_rn_playback_configure": lambda: L.crispy_rn_playback_configure(None, 44100.0),
        "crispy_rn_playback_buffered": lambda: L.crispy_rn_playback_buffered(None),
        "crispy_rn_pull_device": lambda: L.crispy_rn_pull_device(None, 4, 1, 0, C.addressof(buf), 4, C.byref(live), None),
        "crispy_rn_pull": lambda: L.crispy_rn_pull(None, 4, 1, 0, C.addressof(buf), 4, C.byref(live)),
    }
    assert set(calls) == set(NAMES)
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.crispy_last_error().decode()
        assert msg.startswith(name + ":") and "NULL handle" in msg, (name, msg)
    assert live.value == 7 and not any(buf)
    assert L.crispy_abi_version() == 6          # new entry points only: no struct grew, no argument changed meaning


def test_names_are_bound_and_declared():
    from crispy_amd import _native as N
    L = _lib()
    hdr = open(os.path.join(ROOT, "include", "crispy_hip.h")).read()
    for name in NAMES:
        assert name in N.RN_SYMBOLS and name in N.ALL_SYMBOLS
        assert getattr(L, name).argtypes, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    assert L.crispy_rn_playback_buffered.restype is C.c_long
    for name, val in (("CRISPY_PCM_F32", 0), ("CRISPY_PCM_I16", 1), ("CRISPY_PCM_U16", 2)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr), name
    assert (N.PCM_F32, N.PCM_I16, N.PCM_U16) == (0, 1, 2)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_playback_kernels_have_no_scratch_and_no_fused_multiply_add(tmp_path):
    text = open(os.path.join(ROOT, "crispy_amd", "csrc", "Makefile")).read()
    assert "rn_playback.hip" in re.search(r"^SRCS := (.*)$", text, re.M).group(1).split()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    flags = [f for f in flags if f != "-fPIC" and not f.startswith("-W")]
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_playback.hip")
    asm = tmp_path / "pb.s"
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
    # the append, and the pull in three formats x (16-byte stores, fallback)
    assert sum("rn_ring_append_kernel" in k for k in res) == 1 and sum("rn_pull_kernel" in k for k in res) == 6, list(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    isa = asm.read_text()
    assert not re.search(r"\bv_(fma|fmac|mad|mac|pk_fma)_(f32|f16|legacy|mix)", isa), "a fused multiply-add in rn_playback.hip"
    assert isa.count("v_sub_f32") >= 6          # s1 - s0 of every pull kernel

"""Scratch and LDS of the speaker-clustering kernels (crispy_amd/csrc/diar_kernels.hip), cross-compiled here with the
flags of the shipped build: no kernel spills to scratch, the static LDS of each stays inside the default 64 KB, and the
one-workgroup eigensolver's dynamic LDS (sized in the file from kLdsN) fits the 160 KB of a gfx950 compute unit."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "crispy_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_scratch_and_lds_within_limits(tmp_path):
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([HIPCC, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "diar_kernels.hip"),
                          "-o", str(tmp_path / "diar.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr)]
    assert len(names) >= 14 and len(names) == len(scratch) == len(lds)
    for n, s, l in zip(names, scratch, lds):
        assert s == 0, f"{n} spills {s} bytes per lane"
        assert l <= 64 * 1024, f"{n} holds {l} bytes of static LDS"
    hdr = open(os.path.join(CSRC, "diar_jacobi.h")).read()
    lds_n = int(re.search(r"constexpr int kLdsN = (\d+);", hdr).group(1))
    threads = int(re.search(r"constexpr int kLdsThreads = (\d+);", open(os.path.join(CSRC, "diar_kernels.hip")).read()).group(1))
    assert (lds_n * lds_n + 3 * (lds_n // 2 + 1) + threads) * 4 <= 160 * 1024

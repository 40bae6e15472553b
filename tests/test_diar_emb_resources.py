"""Scratch and LDS of the embedding network's kernels (crispy_amd/csrc/diar_emb.hip), cross-compiled here with the flags of the
shipped build: no kernel spills to scratch memory and the static LDS of each stays inside the default 64 KB."""
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
    out = subprocess.run([HIPCC, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "diar_emb.hip"),
                          "-o", str(tmp_path / "diar_emb.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", out.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out.stderr)]
    # eight forms of the head convolution, the tdnn, two forms of the GEMM, gates, local convolution, pooling, dense
    assert len(names) >= 15 and len(names) == len(scratch) == len(lds)
    for family in ("emb_conv2d_kernel", "emb_tdnn_kernel", "emb_gemm_kernel", "emb_gates_kernel", "emb_local_kernel", "emb_pool_kernel",
                   "emb_dense_kernel"):
        assert any(family in n for n in names), family
    for n, s, l in zip(names, scratch, lds):
        assert s == 0, f"{n} spills {s} bytes per lane"
        assert l <= 64 * 1024, f"{n} holds {l} bytes of static LDS"

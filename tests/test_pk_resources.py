"""Register / LDS / scratch budget of the Parakeet encoder's kernels (cross-compiled here, no GPU needed): nothing spills, and the
attention kernel keeps the budget its two workgroups per CU rest on -- at most 256 registers per lane, two waves per SIMD
(its 68 KB of LDS are dynamic and sized in the launch)."""
import os
import re
import subprocess

import pytest

from tests.test_build_resources import CGFLAGS, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crispy_amd", "csrc")


def resources(src, tmp_path):
    out = subprocess.run([HIPCC, *CGFLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, src), "-o",
                          str(tmp_path / (src + ".s"))], capture_output=True, text=True, timeout=600, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z/\[\] ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src,kernels", [("pk_sub.hip", 5), ("pk_gemm.hip", 4), ("pk_attn.hip", 1)])
def test_no_kernel_spills(tmp_path, src, kernels):
    res = resources(src, tmp_path)
    assert len(res) == kernels, list(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)      # static LDS; the attention kernel's is dynamic
    if src == "pk_attn.hip":
        (name, r), = res.items()
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256 and r["Occupancy"] >= 2, (name, r)

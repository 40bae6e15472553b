"""Register / LDS / scratch budget of the kernel of the Parakeet encoder's attention mode 1 (pk_attn_f16.hip; cross-compiled here, no
GPU needed), as DESIGN section 15 states it: one kernel, nothing spills, at most 256 registers per lane (two waves per SIMD), and
dynamic LDS of which two workgroups fit the CU's 160 KB; the three products are 32 f16 matrix instructions per key tile and wave,
with V read by 16 transposed LDS reads."""
import os
import re

import pytest

from tests.test_build_resources import HIPCC
from tests.test_pk_resources import CSRC, resources

SRC = "pk_attn_f16.hip"


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    tmp = tmp_path_factory.mktemp("pk_attn_f16")
    return resources(SRC, tmp), open(tmp / (SRC + ".s")).read()


def test_one_kernel_no_spills_two_waves_per_simd(built):
    res, _asm = built
    (name, r), = res.items()
    assert "pk_attn_f16_kernel" in name
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["VGPRs"] + r.get("AGPRs", 0) <= 256 and r["Occupancy"] >= 2, r
    assert r["LDS Size"] == 0, r      # dynamic, sized in the launch


def test_lds_budget_fits_two_workgroups():
    src = open(os.path.join(CSRC, SRC)).read()
    row_k, row_v = (int(x) for x in re.search(r"kRowK = kD \* 2 \+ (\d+), kRowV = kD \* 2 \+ (\d+);", src).groups())
    total = 32 * (256 + row_k) + 32 * (256 + row_v) + 4 * 32 * 32 * 4 + 5 * 32 * (256 + row_k)      # K, V, the waves' band results, the ring
    assert f"static_assert(kLdsBytes == {total}" in src
    assert 2 * total <= 160 * 1024


def test_instruction_mix(built):
    _res, asm = built
    assert asm.count("v_mfma_f32_32x32x16_f16") == 32      # 16 band, 8 key, 8 value products per tile
    assert asm.count("ds_read_b64_tr_b16") == 16
    assert "v_mfma_f32_32x32x2" not in asm

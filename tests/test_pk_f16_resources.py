"""Register / LDS / scratch budget of the kernels of the Parakeet encoder's precision mode 1 (pk_gemm_f16.hip; cross-compiled here, no
GPU needed): nothing spills, static LDS within 64 KB, and the GEMM keeps the three waves per SIMD (three workgroups per CU) that
DESIGN section 14 states for it: at most 168 registers per lane."""
import os

import pytest

from tests.test_build_resources import HIPCC
from tests.test_pk_resources import resources

SRC = "pk_gemm_f16.hip"


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return resources(SRC, tmp_path_factory.mktemp("pk_f16"))


def test_kernel_set(res):
    names = sorted(res)
    assert len(names) == 6, names      # four epilogues of the GEMM, the pack kernel, the stage's transposition
    assert sum("pk_gemm_f16_kernel" in n for n in names) == 4 and sum("pk_pack_f16_kernel" in n for n in names) == 1, names


def test_no_kernel_spills(res):
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)


def test_gemm_occupancy(res):
    for name, r in res.items():
        if "pk_gemm_f16_kernel" in name:
            assert r["VGPRs"] + r.get("AGPRs", 0) <= 168 and r["Occupancy"] >= 3, (name, r)
            assert r["LDS Size"] == 2 * 128 * 32 * 2, (name, r)      # two A images of 128 rows x 32 halves

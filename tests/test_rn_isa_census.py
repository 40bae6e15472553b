"""Static instruction census of the RNNoise frame kernel (tools/isa_census.py: the file cross-compiled with the Makefile's
flags, instructions counted by class from the kernel's label to its s_endpgm).  The vector issue port is what bounds
rn_frame_kernel<false> (NOTEBOOK.md section 16), so its vector-instruction count is held where the instruction-removal pass
left it; the LDS and memory counts may not rise above the figures from before that pass.  No GPU needed."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT = {"vector": 5960, "matrix": 456, "lds": 906, "memory": 332}    # the commit before the removal pass, same flags
VECTOR_NOW = 5388                                                      # reached by the removal pass: 9.6 % below PARENT


@pytest.fixture(scope="module")
def frame_census():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_kernels.hip")
    res = tool.census(tool.assemble(src, []), src)
    names = tool.demangle(list(res))
    hit = [r for sym, r in res.items() if "rn_frame_kernel<false>" in names[sym]]
    assert len(hit) == 1, sorted(names.values())
    return hit[0]["classes"]


def test_frame_kernel_vector_count_stays_down(frame_census):
    print(dict(frame_census))
    assert frame_census["vector"] <= VECTOR_NOW, f"{frame_census['vector']} vector instructions (parent of the pass: {PARENT['vector']})"
    assert VECTOR_NOW <= 0.92 * PARENT["vector"]


def test_frame_kernel_lds_and_memory_counts_did_not_rise(frame_census):
    assert frame_census["lds"] <= PARENT["lds"]
    assert frame_census["memory"] <= PARENT["memory"]
    assert frame_census["matrix"] == PARENT["matrix"]      # removals only: no product moved onto or off the matrix pipe

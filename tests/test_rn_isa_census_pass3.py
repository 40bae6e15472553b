"""Static instruction census of the RNNoise frame kernel after the third removal pass (NOTEBOOK.md section 28): index,
select and move code -- the half-empty trips of the joint X/P transform merged, the row-joining steps of the wave sums and
the shifted adds of band_sum as single DPP adds, pass twiddles from row tables, the pitch buffer at a 256-byte multiple
of LDS, 32-bit offsets in the windowed first pass.  Same tool, flags and fixture style as tests/test_rn_isa_census.py and
tests/test_rn_isa_census_pass2.py.  No GPU needed.

No floating-point operation was added, dropped or moved to another pipe, so the matrix count is the parent's; the vector
and LDS counts are regression guards at what the pass reached."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_VECTOR = 5154          # the commit before this pass
VECTOR_NOW = 4982             # what the pass achieved: -172
MATRIX = 456
PARENT_LDS = 868
LDS_NOW = 855
PARENT_MEMORY = 292
MEMORY_NOW = 276


@pytest.fixture(scope="module")
def frame_kernel():
    spec = importlib.util.spec_from_file_location("isa_census", os.path.join(ROOT, "tools", "isa_census.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    src = os.path.join(ROOT, "crispy_amd", "csrc", "rn_kernels.hip")
    res = tool.census(tool.assemble(src, []), src)
    names = tool.demangle(list(res))
    hit = [r for sym, r in res.items() if "rn_frame_kernel<false>" in names[sym]]
    assert len(hit) == 1, sorted(names.values())
    return hit[0]


def test_vector_count_stays_where_the_pass_left_it(frame_kernel):
    c = frame_kernel["classes"]
    print(dict(c))
    assert c["vector"] <= VECTOR_NOW, f"{c['vector']} vector instructions (this pass: {VECTOR_NOW}, its parent: {PARENT_VECTOR})"


def test_matrix_count_is_unchanged(frame_kernel):
    assert frame_kernel["classes"]["matrix"] == MATRIX


def test_lds_count_is_at_most_the_parents(frame_kernel):
    n = frame_kernel["classes"]["lds"]
    print(f"lds: {n} (this pass: {LDS_NOW}, parent {PARENT_LDS})")
    assert n <= PARENT_LDS


def test_memory_count_did_not_grow_with_the_row_tables(frame_kernel):
    n = frame_kernel["classes"]["memory"]
    print(f"memory: {n} (this pass: {MEMORY_NOW}, parent {PARENT_MEMORY})")
    assert n <= PARENT_MEMORY

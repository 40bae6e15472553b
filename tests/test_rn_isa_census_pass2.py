"""Static instruction census of the RNNoise frame kernel after the second removal pass (NOTEBOOK.md section 24): the top-2
arg-max of the coarse pitch search as selects over fixed cross-lane patterns, the digit-scale pair on the scalar unit, and
one accumulator chain per row in the one-wave kernel's int8 products.  Same tool, flags and fixture style as
tests/test_rn_isa_census.py.  No GPU needed.

The single accumulator chain was kept (it timed no slower than two, section 24), so the bar that applies is the full one:
5 388 - 228 = 5 160 vector instructions (had the chain item been dropped for speed it would have been 5 388 - 175 = 5 213)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_VECTOR = 5388          # the commit before this pass (tests/test_rn_isa_census.py: VECTOR_NOW)
VECTOR_BAR = 5160             # 80 % of the -285 the pass was sized at
MATRIX = 456
PARENT_EXECZ = 124            # s_cbranch_execz in rn_frame_kernel<false> at the commit before this pass, same flags


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


def test_vector_count_is_below_the_bar_of_the_pass(frame_kernel):
    c = frame_kernel["classes"]
    print(dict(c))
    assert c["vector"] <= VECTOR_BAR, f"{c['vector']} vector instructions (parent of the pass: {PARENT_VECTOR})"


def test_matrix_count_is_unchanged(frame_kernel):
    assert frame_kernel["classes"]["matrix"] == MATRIX


def test_fewer_divergent_regions_than_the_parent(frame_kernel):
    n = frame_kernel["mnemonics"]["s_cbranch_execz"]
    print(f"s_cbranch_execz: {n} (parent {PARENT_EXECZ})")
    assert n < PARENT_EXECZ

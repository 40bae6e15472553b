"""The device-free host logic of Parakeet's log-mel front end under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU box (the way
of tests/test_pk_tdt_sanitizers.py): pk_mel_api.cpp is compiled unmodified by tests/asan/pk_mel_harness.cpp, a stand-alone program,
against the host-memory stand-in for the HIP runtime (tests/asan/hip/hip_runtime.h), and fed the row count at its edges, filter
matrices cut to runs from arrays of exactly the stated sizes, the tap cap on, one above and far above, hostile sample offsets
(descending, negative, overflowing, fewer than 320 samples, too many rows), ragged calls at the tile's edges and at 40 000 rows with
buffers and workspace at their computed sizes, NULL and non-NULL taps, and a device too small for the workspace.

Done = zero sanitizer reports and every case answered as expected.  CPU build only; nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

pytestmark = pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang++ (sanitizer runtimes) not installed")


def test_host_logic_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "pk_mel_harness")
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "tests", "asan"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "asan", "pk_mel_harness.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "pk_mel_harness: 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])

"""rn_prio_of / rn_prio_at (crispy_amd/csrc/rn_prio.h, the text the frame kernel compiles) on the host: the issue priority a wave
of the one-wave RNNoise frame kernel takes from its slot on the SIMD and the frame inside the launch.  For the mode the header
ships: the four slots of a SIMD hold four distinct priorities at every frame; under a rotating rule (mode 2 or 3) a slot takes
each priority once over any four consecutive frames, so no wave is the arbitration loser for a whole launch; and the values
stay in 0 .. 3 (the operand range of s_setprio) for slots 0 .. 15.  The other modes of the developer knob are held to the
properties that apply to them.  tests/host/rn_prio_check.cpp is the program.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crispy_amd", "csrc")


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def _run(tmp_path, flags):
    exe = str(tmp_path / "rn_prio_check")
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", CSRC] + flags +
                       [os.path.join(ROOT, "tests", "host", "rn_prio_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    return r


def test_shipped_rule_keeps_slots_distinct_and_rotates(tmp_path):
    r = _run(tmp_path, [])
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"rn_prio mode (\d): ok", r.stdout)
    assert m, r.stdout
    shipped = int(re.search(r"^#define RN_PRIO_MODE (\d)", open(os.path.join(CSRC, "rn_prio.h")).read(), re.M).group(1))
    assert int(m.group(1)) == shipped


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_every_mode_of_the_knob(tmp_path, mode):
    r = _run(tmp_path, [f"-DRN_PRIO_MODE={mode}"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"rn_prio mode {mode}: ok" in r.stdout

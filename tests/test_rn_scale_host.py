"""scale_of and scale_shift of the RNNoise gain network (crispy_amd/csrc/rn_scale.h, the text the frame kernel compiles) on the
host, over every exponent byte: the scale pair against the min(max()) form it had before the arithmetic moved to the scalar
unit, and the exponent add against the multiplications by 2^8, 2^16, 2^24 it replaced -- bit for bit, at and beyond both ends
of the clamp [64, 250].  The GPU tests cannot reach those ends: scale_of sees the largest feature or activation of a frame, and
PCM from 2^-13 of full scale to full scale moves that only between 6.8 and 62 (exponent bytes 129 .. 132), see
tests/test_gpu_rn_pitch_edges.py.  tests/host/rn_scale_check.cpp is the program.  No GPU needed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_scale_pair_and_exponent_add_over_every_exponent(tmp_path):
    exe = str(tmp_path / "rn_scale_check")
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "crispy_amd", "csrc"),
                        os.path.join(ROOT, "tests", "host", "rn_scale_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clamped exponent 64 .. 250" in r.stdout

"""The host-built tables of the RNNoise frame kernel that replace index arithmetic in the kernel (NOTEBOOK.md section 28), on
the host: RnTables::tw8 / tw3 / tw5 (crispy_amd/csrc/rn_twiddle_rows.h: the twiddles of one butterfly side by side) against
w960[k r (960 / (NS R))] for all 64 lanes and every trip of every pass, the joint trip of two signals included; and
RnTables::band_piece (crispy_amd/csrc/rn_band_piece.h), whose two add flags now sit in the giving lane, against the
taking-lane form it replaces -- flag by flag, and the band sums of both forms bit for bit.  The headers are the text the
library compiles; tests/host/rn_tables_check.cpp is the program.  No GPU needed."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crispy_amd", "csrc")


def _compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(c) or (c if os.path.isabs(c) and os.path.exists(c) else None)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_twiddle_rows_and_band_pieces_match_the_formulas_they_replace(tmp_path):
    exe = str(tmp_path / "rn_tables_check")
    r = subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", CSRC,
                        os.path.join(ROOT, "tests", "host", "rn_tables_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rn twiddle rows: ok" in r.stdout and "rn band pieces: ok" in r.stdout


def test_the_library_builds_its_tables_with_these_headers():
    api = open(os.path.join(CSRC, "crispy_api.cpp")).read()
    assert "rn_build_twiddle_rows(t->w960, t->tw8, t->tw3, t->tw5)" in api
    assert "rn_build_band_piece(t->band_piece)" in api

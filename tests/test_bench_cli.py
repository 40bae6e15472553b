"""bench.py's options that need no GPU: the output sample of --dump-outputs (size cap, fixed selection) and the workloads
that option accepts.  The plain and --full runs themselves are in tests/test_gpu_bench_paths.py."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_selection_fits_the_cap_and_is_fixed():
    for B, T in ((4096, 100), (1024, 50), (16384, 3001), (8, 200000)):
        f0, idx = bench.dump_selection(B, T)
        assert 0 <= f0 < T and idx.ndim == 1 and idx.size >= 1
        assert (T - f0) * idx.size * 480 * 4 <= bench.DUMP_BYTES <= 64e6
        assert idx[0] >= 0 and idx[-1] < B and (np.diff(idx) > 0).all()
        f1, idx1 = bench.dump_selection(B, T)
        assert f1 == f0 and np.array_equal(idx1, idx)
    f0, idx = bench.dump_selection(4096, 100)
    assert f0 == 0 and idx.size == bench.DUMP_BYTES // (100 * 480 * 4)      # every frame of as many streams as fit
    f0, idx = bench.dump_selection(64, 10)
    assert f0 == 0 and idx.tolist() == list(range(64))                      # small outputs whole


def test_dump_outputs_writes_the_selection_as_float32(tmp_path):
    B, T = 1024, 50
    out = np.random.default_rng(1).standard_normal((T, B, 480), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "d"), out, B, T)
    f0, idx = bench.dump_selection(B, T)
    got = np.load(tmp_path / "d" / "denoised.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out[f0:, idx])
    assert not (tmp_path / "d" / "vad.npy").exists()
    vad = np.random.default_rng(2).random((T, B), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "h"), out, B, T, vad=vad)
    got = np.load(tmp_path / "h" / "vad.npy")
    assert got.dtype == np.float32 and np.array_equal(got, vad[f0:, idx])


def test_dump_outputs_is_refused_for_other_workloads(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg5", "--dump-outputs",
                        str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "cfg2 only" in r.stderr

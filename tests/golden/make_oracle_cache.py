"""Computes and commits the slow, GPU-independent oracle results of the full-size GPU tests (tests/oracle_cases.py) into
tests/golden/oracle_cache/*.json.  CPU only; about ten minutes (the three catalog encoders at full depth are most of it).

    python tests/golden/make_oracle_cache.py [scripted] [catalog] [enc_attn]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["CRISPY_ORACLE_CACHE"] = "write"

from tests import oracle_cases as OC  # noqa: E402

what = set(sys.argv[1:]) or {"scripted", "catalog", "enc_attn"}
if "scripted" in what:
    for W, hp, n, mode, kw in OC.scripted_cases():
        t0 = time.time()
        OC.scripted_ref(W, hp, n, mode, **kw)
        print(f"scripted whisper_full: {n} samples, mode {mode}, {kw}: {time.time() - t0:.1f} s", flush=True)
if "catalog" in what:
    for name in ("small", "medium", "large_v3"):
        t0 = time.time()
        OC.catalog_ref(name)
        print(f"catalog {name}: {time.time() - t0:.1f} s", flush=True)
if "enc_attn" in what:      # tests/enc_attn_cases.py: the noise runs behind the bars of tests/test_gpu_encoder_attention.py, ~2 minutes
    from tests import enc_attn_cases as EC  # noqa: E402
    for d in EC.HEADS:
        t0 = time.time()
        for mode in (1, 2):
            EC.bars(d, mode)
        EC.mode0_gap(d)
        print(f"encoder attention fixture, width {d}: {time.time() - t0:.1f} s", flush=True)
    for clip in (0, 1):
        t0 = time.time()
        EC.chain_ref(clip)
        print(f"peaked chain, clip {clip}: {time.time() - t0:.1f} s", flush=True)

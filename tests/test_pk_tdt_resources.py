"""Resources of Parakeet's TDT decoder.  Cross-compiled here, no GPU needed: none of its kernels spills, the skinny products keep
the static LDS of one tile and the two waves per SIMD their launches can fill.  On the GPU: create, load, decode and destroy in a loop
leave device memory where it was."""
import os

import numpy as np
import pytest

from tests import pk_tdt_oracle as TO
from tests.test_build_resources import HIPCC
from tests.test_pk_resources import resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_no_kernel_spills(tmp_path):
    res = resources("pk_tdt.hip", tmp_path)
    assert len(res) == 5, list(res)      # init, LSTM layer, decoder_projector, joint, advance
    for name, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["LDS Size"] <= 32 * 1024, (name, r)      # one tile: 8 KB of inputs, 16 KB of wave sums, the row pointers
        # The largest launch of a 64-clip call is the joint's 516 workgroups on 256 CUs, an LSTM layer's is 160: two workgroups of four
        # waves per CU, two waves per SIMD, is all a launch can fill, and at two waves a lane may hold 256 registers.  The products
        # spend them on two blocks of weights in flight.
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256 and r["Occupancy"] >= 2, (name, r)


@pytest.mark.gpu
def test_create_load_decode_destroy_leaves_device_memory_where_it_was():
    import torch
    from crispy_amd import ParakeetTDT
    cfg = TO.TdtConfig(hidden=256, decoder_hidden=512, decoder_layers=1, vocab=4096, blank=4095)
    w = TO.make_tdt_weights(cfg, 1, **TO.MIX)
    per_handle = sum(v.size for v in w.values()) * 4      # 27 MB of weights alone
    clips = [TO.frames(t, cfg.hidden, t) for t in (0, 3, 17)]

    def once():
        h = ParakeetTDT(0)
        try:
            h.load(cfg.as_dict(), w)
            h.load(cfg.as_dict(), w)      # a reload lets the first copy go
            steps = h.decode(clips, taps=True)[0]
            assert len(steps[0]) == 0 and len(steps[2]) > 0
        finally:
            h.close()

    once()      # what the runtime keeps after a first use is not a leak
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        once()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print(f"pk tdt resources: free device memory {before} -> {after} over 6 rounds of {per_handle} bytes of weights each")
    assert per_handle > 24 << 20
    assert before - after < 8 << 20, (before, after)      # one leaked copy is 27 MB, six are 160 MB; the runtime's own pools move in 2 MB steps

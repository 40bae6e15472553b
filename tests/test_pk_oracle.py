"""Host side of the Parakeet encoder (crispy_pk_*, include/crispy_hip.h), no GPU: the oracle (tests/pk_oracle.py) pinned on
transformers' ParakeetEncoder and on the committed outputs of it, the rel_shift identity, the frame formula, the tensor table
against the oracle's state dict, the new symbols on every layer, and what the load and the encode refuse before a device is
touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import pk_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "parakeet_enc_golden.npz")
NEW = ("crispy_pk_create", "crispy_pk_destroy", "crispy_pk_frames", "crispy_pk_tensor_spec", "crispy_pk_load", "crispy_pk_loaded",
       "crispy_pk_config_of", "crispy_pk_encode_device", "crispy_pk_encode")
NO_FLAGS = PO.with_flags(PO.TINY, attention_bias=0, convolution_bias=0, scale_input=0)

# The oracle against the library, float64 both, TINY on GOLDEN_ROWS: the two differ only in how inv_freq is rounded (the library
# forms 10000^(2k/H) in float32, the specification in double), so they are close and not bit-equal.
LIBRARY_MEASURED = 3.5e-8      # the largest distance measured (rows 300; 1.8e-8 at rows 73, 0 at one frame); outputs are about 3.7 large
LIBRARY_BOUND = 3.5e-7         # 10 x that
# The committed file against this machine's float64 forward of the oracle: the same distance plus float64 rounding of another
# BLAS (1e-13), so the same bound.


def _lib():
    from crispy_amd import _native as N
    return N, N.lib()


@pytest.fixture(scope="module")
def weights():
    return PO.make_weights(PO.TINY, PO.GOLDEN_SEED)


@pytest.fixture(scope="module")
def oracle_outputs(weights):
    """float64 and float32 oracle outputs on the golden clips; shared and left unchanged"""
    import torch
    clips = [PO.clip(r, PO.TINY.mel_bins, r) for r in PO.GOLDEN_ROWS]
    o64 = PO.Encoder(PO.TINY, weights, torch.float64).forward(clips)
    o32 = PO.Encoder(PO.TINY, weights, torch.float32).forward(clips)
    return clips, [r[0] for r in o64], [r[0] for r in o32]


def test_oracle_against_the_transformers_encoder(weights, oracle_outputs):
    pytest.importorskip("transformers.models.parakeet")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_parakeet_golden as G
    finally:
        sys.path.pop(0)
    net = G.library_encoder(PO.TINY, weights)      # asserts the state-dict keys and their order
    clips, o64, _o32 = oracle_outputs
    worst = 0.0
    for rows, x, mine in zip(PO.GOLDEN_ROWS, clips, o64):
        lib = G.library_forward(net, x)
        assert lib.shape == mine.shape == (PO.frames(rows), PO.TINY.hidden)
        err = float(np.abs(lib - mine).max())
        print(f"pk oracle rows {rows}: {err:.3e} from transformers' ParakeetEncoder in float64 (largest value {np.abs(lib).max():.2f})")
        worst = max(worst, err)
    assert worst <= LIBRARY_BOUND, (worst, LIBRARY_MEASURED)


def test_oracle_against_the_committed_library_outputs(oracle_outputs):
    gold = np.load(GOLDEN)
    assert sorted(gold.files) == sorted(f"rows{r}" for r in PO.GOLDEN_ROWS)
    _clips, o64, o32 = oracle_outputs
    for rows, mine, single in zip(PO.GOLDEN_ROWS, o64, o32):
        want = gold[f"rows{rows}"]
        assert want.dtype == np.float64 and want.shape == mine.shape
        err, f32 = float(np.abs(want - mine).max()), float(np.abs(single - mine).max())
        print(f"pk golden rows {rows}: float64 oracle {err:.3e} from the file, float32 oracle {f32:.3e} from float64")
        assert err <= LIBRARY_BOUND, (rows, err)
        assert single.dtype == np.float32 and 0 < f32 <= 2e-5, (rows, f32)      # f32 eps is 6e-8: some hundred roundings deep, not more


def test_rel_shift_direct_equals_pad_and_reshape():
    import torch
    for t in (1, 2, 7, 38):
        full = torch.from_numpy(np.random.default_rng(t).standard_normal((2, t, 2 * t - 1)))
        a, b = PO.rel_shift_direct(full), PO.rel_shift_pad(full)
        assert a.shape == b.shape == (2, t, t) and torch.equal(a, b)
        for i, j in ((0, 0), (t - 1, 0), (0, t - 1)):
            assert a[1, i, j] == full[1, i, (t - 1) - (i - j)]


def test_frames_formula():
    import torch
    N, L = _lib()
    assert L.crispy_pk_frames.restype is C.c_long
    sub = PO.Subsampling(PO.TINY).eval()
    for rows in range(1, 65):
        want = rows
        for _ in range(3):
            want = (want - 1) // 2 + 1
        with torch.no_grad():
            got = sub(torch.zeros(rows, PO.TINY.mel_bins)).shape[0]
        assert L.crispy_pk_frames(rows) == want == PO.frames(rows) == got, rows
    assert L.crispy_pk_frames(0) == 0 and L.crispy_pk_frames(-5) == 0 and L.crispy_pk_frames(40000) == 5000


def test_new_symbols_on_every_layer_and_abi_unchanged():
    N, L = _lib()
    assert N.PK_SYMBOLS == NEW and set(NEW) <= set(N.ALL_SYMBOLS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crispy_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(L, s).argtypes is not None, s
        assert re.search(r"pub fn %s\(" % s, rust), s
    assert L.crispy_abi_version() == 6 == N.ABI_VERSION and "#define CRISPY_ABI_VERSION 6" in hdr
    fields = re.search(r"typedef struct crispy_pk_config \{\s*int ([^;]*);", hdr).group(1)
    assert tuple(f.strip() for f in fields.split(",")) == tuple(k for k, _t in N.PkConfig._fields_)
    assert tuple(re.findall(r"pub (\w+): c_int,", re.search(r"pub struct crispy_pk_config \{(.*?)\n\}", rust, flags=re.S).group(1))) == \
        tuple(k for k, _t in N.PkConfig._fields_)
    import crispy_amd
    from crispy_amd.parakeet import ParakeetEncoder
    assert crispy_amd.ParakeetEncoder is ParakeetEncoder


@pytest.mark.parametrize("cfg", [PO.TINY, NO_FLAGS, PO.with_flags(PO.TINY, mel_bins=80), PO.with_flags(PO.CATALOG_V3, layers=2)],
                         ids=["tiny", "flags0", "mel80", "catalog widths"])
def test_tensor_spec_is_the_oracles_state_dict(cfg):
    from crispy_amd.parakeet import pk_tensor_spec
    want = PO.tensor_list(cfg)
    assert pk_tensor_spec(cfg.as_dict()) == want
    assert not any(k.endswith("num_batches_tracked") for k, _n in want)
    if cfg is NO_FLAGS:
        assert not any(k.endswith("proj.bias") or "conv.pointwise_conv1.bias" in k or "linear1.bias" in k for k, _n in want)


def test_tensor_spec_refuses_what_is_outside_the_supported_set():
    N, L = _lib()
    from crispy_amd.parakeet import make_config
    ok = make_config(PO.TINY.as_dict())
    n = L.crispy_pk_tensor_spec(C.byref(ok), 0, None, None)
    assert n == len(PO.tensor_list(PO.TINY))
    for i in (-1, n):
        assert L.crispy_pk_tensor_spec(C.byref(ok), i, None, None) == -1 and b"outside" in L.crispy_last_error()
    assert L.crispy_pk_tensor_spec(None, 0, None, None) == -1 and b"cfg is NULL" in L.crispy_last_error()
    for field, bad in (("heads", 0), ("heads", 17), ("hidden", 257), ("layers", 0), ("ffn", 500), ("conv_kernel", 8), ("conv_kernel", 33),
                       ("mel_bins", 84), ("sub_channels", 48), ("attention_bias", 2), ("convolution_bias", -1), ("scale_input", 2)):
        cfg = make_config(dict(PO.TINY.as_dict(), **{field: bad}))
        assert L.crispy_pk_tensor_spec(C.byref(cfg), 0, None, None) == -1, (field, bad)
        assert field.encode() in L.crispy_last_error(), (field, L.crispy_last_error())


def _load(L, h, cfg, tensors, counts=None, null=None, extra=()):
    from crispy_amd.parakeet import make_config
    names = list(tensors) + list(extra)
    arrs = [np.ascontiguousarray(tensors[k], dtype=np.float32).reshape(-1) for k in names]
    cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
    cd = (C.c_void_p * len(names))(*[None if k == null else a.ctypes.data for k, a in zip(names, arrs)])
    cnt = np.array([a.size if counts is None or k not in counts else counts[k] for k, a in zip(names, arrs)], np.int64)
    c = make_config(cfg if isinstance(cfg, dict) else cfg.as_dict())
    rc = L.crispy_pk_load(h, C.byref(c), cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), len(names))
    return rc, L.crispy_last_error()


def test_load_validates_before_touching_a_device(weights):
    N, L = _lib()
    fake = C.c_void_p(1)      # never dereferenced: every case below fails before the handle is used
    rc, msg = _load(L, None, PO.TINY, weights)
    assert rc == -1 and b"NULL handle" in msg
    assert L.crispy_pk_loaded(None) == 0
    for name in ("subsampling.layers.0.weight", "subsampling.linear.bias", "layers.0.self_attn.bias_v", "layers.2.conv.norm.running_var",
                 "layers.1.self_attn.relative_k_proj.weight", "layers.2.norm_out.bias"):
        rc, msg = _load(L, fake, PO.TINY, {k: v for k, v in weights.items() if k != name})
        assert rc == -1 and name.encode() in msg and b"missing" in msg, (name, msg)
    rc, msg = _load(L, fake, PO.TINY, weights, extra=["layers.1.conv.depthwise_conv.weight"])
    assert rc == -1 and b"layers.1.conv.depthwise_conv.weight" in msg and b"twice" in msg
    rc, msg = _load(L, fake, PO.TINY, dict(weights, **{"layers.0.conv.norm.num_batches_tracked": np.zeros(1, np.float32)}))
    assert rc == -1 and b"layers.0.conv.norm.num_batches_tracked" in msg and b"unknown" in msg
    rc, msg = _load(L, fake, PO.TINY, dict(weights, **{"layers.3.norm_out.bias": np.zeros(256, np.float32)}))      # a fourth block
    assert rc == -1 and b"layers.3.norm_out.bias" in msg and b"unknown" in msg
    rc, msg = _load(L, fake, NO_FLAGS, weights)      # the flags at 0: the bias tensors are not expected
    assert rc == -1 and b"unknown" in msg and b".bias" in msg
    for name, off in (("layers.0.feed_forward1.linear1.weight", -1), ("subsampling.layers.3.bias", 1), ("layers.2.self_attn.bias_u", 128),
                      ("layers.1.conv.depthwise_conv.weight", -256)):
        rc, msg = _load(L, fake, PO.TINY, weights, counts={name: int(np.asarray(weights[name]).size) + off})
        assert rc == -1 and name.encode() in msg and b"expected" in msg, (name, msg)
    rc, msg = _load(L, fake, PO.TINY, weights, null="layers.1.feed_forward2.linear2.weight")
    assert rc == -1 and b"layers.1.feed_forward2.linear2.weight" in msg and b"NULL" in msg
    for name, bad, what in (("layers.2.self_attn.q_proj.bias", np.nan, b"non-finite"), ("subsampling.layers.5.weight", np.inf, b"non-finite"),
                            ("layers.1.conv.norm.running_var", -1e-3, b"negative variance")):
        w = dict(weights)
        w[name] = np.array(weights[name], np.float32)
        w[name].reshape(-1)[-1] = bad
        rc, msg = _load(L, fake, PO.TINY, w)
        assert rc == -1 and name.encode() in msg and what in msg, (name, msg)
    for field, bad in (("heads", 3), ("ffn", 520), ("mel_bins", 100), ("conv_kernel", 10), ("sub_channels", 33), ("scale_input", 7)):
        rc, msg = _load(L, fake, dict(PO.TINY.as_dict(), **{field: bad}), weights)
        assert rc == -1 and field.encode() in msg, (field, msg)
    c = N.PkConfig(**PO.TINY.as_dict())
    assert L.crispy_pk_load(fake, C.byref(c), None, None, None, 129) == -1 and b"NULL" in L.crispy_last_error()
    assert L.crispy_pk_load(fake, None, None, None, None, 129) == -1 and b"cfg is NULL" in L.crispy_last_error()


def test_encode_validates_before_touching_a_device():
    N, L = _lib()
    fake, ptr = C.c_void_p(1), C.c_void_p(256)
    lp = C.POINTER(C.c_long)
    off = np.array([0, 5, 5], np.int64)
    for fn, tail in ((L.crispy_pk_encode_device, (None,)), (L.crispy_pk_encode, ())):
        assert fn(None, ptr, off.ctypes.data_as(lp), 2, ptr, None, 0, None, None, *tail) == -1 and b"NULL handle" in L.crispy_last_error()
        for n in (0, -1, 4097):
            assert fn(fake, ptr, off.ctypes.data_as(lp), n, ptr, None, 0, None, None, *tail) == -1
            assert b"n_clips %d" % n in L.crispy_last_error()
        assert fn(fake, ptr, None, 2, ptr, None, 0, None, None, *tail) == -1 and b"frame_offset is NULL" in L.crispy_last_error()
        assert fn(fake, ptr, off.ctypes.data_as(lp), 2, ptr, None, 0, None, None, *tail) == -1 and b"clip 1 has 0 rows" in L.crispy_last_error()
        big = np.array([0, 40001], np.int64)
        assert fn(fake, ptr, big.ctypes.data_as(lp), 1, ptr, None, 0, None, None, *tail) == -1 and b"40001 rows" in L.crispy_last_error()
        shifted = np.array([1, 9], np.int64)
        assert fn(fake, ptr, shifted.ctypes.data_as(lp), 1, ptr, None, 0, None, None, *tail) == -1 and b"frame_offset[0]" in L.crispy_last_error()
    assert N.PK_MAX_ROWS == 40000 and N.PK_MAX_CLIPS == 4096 and PO.frames(N.PK_MAX_ROWS) == 5000


def test_state_dict_forms_are_taken_as_they_are(weights):
    import torch
    from crispy_amd.parakeet import state_dict_items
    full = {"encoder." + k: torch.from_numpy(v) for k, v in weights.items()}
    full["encoder.layers.0.conv.norm.num_batches_tracked"] = torch.zeros((), dtype=torch.long)
    full["decoder.embedding.weight"] = torch.zeros(4, 4)
    full["joint.head.weight"] = torch.zeros(4, 4)
    items = state_dict_items(full)
    assert [k for k, _a in items] == list(weights)
    assert all(a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, weights[k].reshape(-1)) for k, a in items)

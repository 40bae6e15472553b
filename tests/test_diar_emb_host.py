"""Host side of the embedding network (crispy_diar_emb_*, crispy_diar_embed*, include/crispy_hip.h), no GPU: the tensor table
against the oracle's state dict, the frame formula against the oracle's output shapes, the new symbols on every layer, what
the load and the entry points refuse before a device is touched, and the oracle itself (tests/emb_oracle.py): float32 against
float64, the segment mean against a written-out loop, a chunk's independence of the rest of the list."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from tests import emb_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("crispy_diar_emb_frames", "crispy_diar_emb_tensor_spec", "crispy_diar_emb_load", "crispy_diar_emb_loaded",
       "crispy_diar_emb_dim", "crispy_diar_emb_forward_device", "crispy_diar_embed_device", "crispy_diar_embed")


def _lib():
    from crispy_amd import _native as N
    return N, N.lib()


def feats(rows, seed):
    x = np.random.default_rng(seed).standard_normal((rows, 80))
    return (x - x.mean(0)).astype(np.float32)


@pytest.fixture(scope="module")
def weights():
    return EO.make_weights(1)


@pytest.fixture(scope="module")
def oracles(weights):
    import torch
    return EO.CAMPPlus(weights, torch.float64), EO.CAMPPlus(weights, torch.float32)


def test_new_symbols_on_every_layer_and_abi_unchanged():
    N, L = _lib()
    assert N.DIAR_EMB_SYMBOLS == NEW and set(NEW) <= set(N.ALL_SYMBOLS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crispy_hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "rust", "crispy-hip-sys", "src", "lib.rs")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert getattr(L, s).argtypes is not None, s
        assert re.search(r"pub fn %s\(" % s, rust), s
    assert L.crispy_diar_emb_frames.restype is C.c_long
    assert L.crispy_abi_version() == 6 == N.ABI_VERSION
    assert "#define CRISPY_ABI_VERSION 6" in hdr


@pytest.mark.parametrize("dim", [512, 192])
def test_tensor_spec_is_the_oracles_state_dict(dim):
    from crispy_amd.diarize import emb_tensor_spec
    N, L = _lib()
    sd = EO.CAMPPlusModules(dim).state_dict()
    want = [(k, int(v.numel())) for k, v in sd.items() if not k.endswith("num_batches_tracked")]
    assert len(want) == 815 == N.EMB_TENSORS == EO.N_TENSORS
    assert emb_tensor_spec(dim) == want
    assert L.crispy_diar_emb_tensor_spec(0, dim, None, None) == 815 and L.crispy_diar_emb_tensor_spec(814, dim, None, None) == 815
    for i, d in ((-1, dim), (815, dim), (0, 0), (0, 1025)):
        assert L.crispy_diar_emb_tensor_spec(i, d, None, None) == -1 and b"outside" in L.crispy_last_error()
    assert L.crispy_diar_emb_tensor_spec(0, 1024, None, None) == 815 and L.crispy_diar_emb_tensor_spec(0, 1, None, None) == 815


def test_frames_equal_the_oracles_output_length(oracles):
    from crispy_amd.diarize import emb_frames
    for t in list(range(1, 13)) + [398]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # one position (rows 1 and 2): torch warns that the unbiased variance is NaN
            _emb, head, xvec, _stats = oracles[1].forward([feats(t, t)])[0]
        assert head.shape == (t, 320)
        assert emb_frames(t) == xvec.shape[0] == (t - 1) // 2 + 1 == EO.emb_frames(t), t
    assert emb_frames(0) == 0 and emb_frames(-3) == 0


def test_oracle_float32_agrees_with_float64(oracles):
    for t in (3, 9, 201):
        x = feats(t, 40 + t)
        a, b = oracles[0].forward([x])[0], oracles[1].forward([x])[0]
        for name, p, q in zip(("embedding", "head", "out_nonlinear", "statistics"), a, b):
            assert p.dtype == np.float64 and q.dtype == np.float32 and p.shape == q.shape
            err, size = float(np.abs(p - q).max()), float(np.abs(p).max())
            print(f"oracle rows {t} {name}: float32 {err:.3e} from float64, largest value {size:.3f}")
            assert 0 < err <= 2e-5 * max(size, 1.0), (t, name, err, size)      # f32 eps is 6e-8: some hundred roundings deep, not more


@pytest.mark.parametrize("t2", [100, 101, 201])
def test_segment_mean_against_a_loop(t2):
    import torch
    h = torch.from_numpy(np.random.default_rng(t2).standard_normal((1, 4, t2)))
    got = EO.seg_mean(h).numpy()
    want = np.zeros_like(got)
    for start in range(0, t2, EO.SEG_LEN):
        end = min(start + EO.SEG_LEN, t2)
        for c in range(4):
            want[0, c, start:end] = h[0, c, start:end].numpy().sum() / (end - start)
    assert got.shape == (1, 4, t2) and np.abs(got - want).max() < 1e-14


def test_a_chunks_oracle_output_does_not_depend_on_the_list(oracles):
    a, b, c = feats(9, 1), feats(201, 2), feats(30, 3)
    alone = oracles[1].forward([b])[0]
    among = oracles[1].forward([a, b, c])[1]
    for p, q in zip(alone, among):
        assert np.array_equal(p, q)


def _load(L, h, tensors, counts=None, null=None):
    names = list(tensors)
    arrs = [np.ascontiguousarray(tensors[k], dtype=np.float32).reshape(-1) for k in names]
    cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
    cd = (C.c_void_p * len(names))(*[None if k == null else a.ctypes.data for k, a in zip(names, arrs)])
    cnt = np.array([a.size if counts is None or k not in counts else counts[k] for k, a in zip(names, arrs)], np.int64)
    rc = L.crispy_diar_emb_load(h, cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), len(names))
    return rc, L.crispy_last_error()


def test_load_validates_before_touching_a_device(weights):
    N, L = _lib()
    fake = C.c_void_p(1)      # never dereferenced: every case below fails before the handle is used
    assert len(weights) == 815
    rc, msg = _load(L, None, weights)
    assert rc == -1 and b"NULL handle" in msg
    assert L.crispy_diar_emb_loaded(None) == 0 and L.crispy_diar_emb_dim(None) == 0
    for name in ("head.conv1.weight", "head.layer2.0.shortcut.1.running_var", "xvector.block2.tdnnd24.cam_layer.linear2.bias",
                 "xvector.dense.linear.weight", "xvector.dense.nonlinear.batchnorm.running_mean"):
        rc, msg = _load(L, fake, {k: v for k, v in weights.items() if k != name})
        assert rc == -1 and name.encode() in msg and b"missing" in msg, (name, msg)
    names = list(weights) + ["xvector.tdnn.linear.weight"]
    arrs = [np.ascontiguousarray(weights[k]).reshape(-1) for k in names]
    cn = (C.c_char_p * len(names))(*[k.encode() for k in names])
    cd = (C.c_void_p * len(names))(*[a.ctypes.data for a in arrs])
    cnt = np.array([a.size for a in arrs], np.int64)
    assert L.crispy_diar_emb_load(fake, cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), len(names)) == -1
    assert b"xvector.tdnn.linear.weight" in L.crispy_last_error() and b"twice" in L.crispy_last_error()
    rc, msg = _load(L, fake, dict(weights, **{"head.bn1.num_batches_tracked": np.zeros(1, np.float32)}))
    assert rc == -1 and b"head.bn1.num_batches_tracked" in msg and b"unknown" in msg
    for name, off in (("xvector.block1.tdnnd3.linear1.weight", -1), ("head.bn2.bias", 1), ("xvector.dense.linear.weight", 1),
                      ("xvector.dense.nonlinear.batchnorm.running_var", -1)):
        rc, msg = _load(L, fake, weights, counts={name: int(np.asarray(weights[name]).size) + off})
        assert rc == -1 and name.encode() in msg, (name, msg)
    rc, msg = _load(L, fake, weights, null="xvector.transit2.linear.weight")
    assert rc == -1 and b"xvector.transit2.linear.weight" in msg and b"NULL" in msg
    for name, bad, what in (("xvector.block3.tdnnd16.cam_layer.linear1.bias", np.nan, b"non-finite"), ("head.conv2.weight", np.inf, b"non-finite"),
                            ("xvector.out_nonlinear.batchnorm.running_var", -1e-3, b"negative variance")):
        w = dict(weights)
        w[name] = np.array(weights[name], np.float32)
        w[name].reshape(-1)[-1] = bad
        rc, msg = _load(L, fake, w)
        assert rc == -1 and name.encode() in msg and what in msg, (name, msg)
    assert L.crispy_diar_emb_load(fake, None, None, None, 815) == -1
    assert L.crispy_diar_emb_load(fake, cn, cd, cnt.ctypes.data_as(C.POINTER(C.c_long)), 0) == -1


def test_forward_and_embed_validate_before_touching_a_device():
    N, L = _lib()
    fake, ptr = C.c_void_p(1), C.c_void_p(256)
    lp = C.POINTER(C.c_long)
    off = np.array([0, 5, 7], np.int64)
    assert L.crispy_diar_emb_forward_device(None, ptr, off.ctypes.data_as(lp), 2, ptr, None, None, None, None) == -1
    assert b"NULL handle" in L.crispy_last_error()
    for n in (0, -1, 16385):
        assert L.crispy_diar_emb_forward_device(fake, ptr, off.ctypes.data_as(lp), n, ptr, None, None, None, None) == -1
        assert b"n_chunks" in L.crispy_last_error()
    assert L.crispy_diar_emb_forward_device(fake, None, off.ctypes.data_as(lp), 2, ptr, None, None, None, None) == -1
    assert L.crispy_diar_emb_forward_device(fake, ptr, off.ctypes.data_as(lp), 2, ptr, None, None, None, None) == -1
    assert b"chunk 1 has 2 rows" in L.crispy_last_error()
    big = np.array([0, 30001], np.int64)
    assert L.crispy_diar_emb_forward_device(fake, ptr, big.ctypes.data_as(lp), 1, ptr, None, None, None, None) == -1
    assert b"30001 rows" in L.crispy_last_error() and N.EMB_MAX_ROWS == 30000 >= 3000
    first, ln = np.array([0, 0], np.int64), np.array([4000, 560], np.int64)
    assert L.crispy_diar_embed(None, ptr, N.PCM_I16, first.ctypes.data_as(lp), ln.ctypes.data_as(lp), 2, 1.0, ptr) == -1
    assert L.crispy_diar_embed_device(None, ptr, N.PCM_I16, first.ctypes.data_as(lp), ln.ctypes.data_as(lp), 2, 1.0, ptr, None) == -1


def test_run_diarization_without_an_embedding_network_is_a_clear_error():
    from crispy_amd import diarize as D

    class NoNetwork:
        segmentation_loaded = True
        embedding_loaded = False

    with pytest.raises(ValueError, match="no embedding network is loaded"):
        D.run_diarization(np.zeros(16000, np.int16), None, None, 2, 0.5, NoNetwork())

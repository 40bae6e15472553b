"""GPU tests of the embedding network (crispy_diar_emb_*, crispy_diar_embed*, include/crispy_hip.h) against tests/emb_oracle.py:
the embedding and the three stage outputs within a bound taken from the float32 torch oracle's own distance to the float64
oracle, on ragged chunks over every edge of the stride-2 layer and of the context segments, on silent, constant and
Kaldi-scale rows, after a reload at another width; batch, position and turn independence byte for byte; the recording entry
points against the forward; the limits; and run_diarization end to end with emb_fn=None.

The bound (the rule of tests/test_gpu_diar_seg.py and tests/test_gpu_diar_fbank.py): per chunk and per tensor, the GPU's largest
distance to float64 stays within 4 x the float32 oracle's.  Both are f32 arithmetic on the same operands; a different but
equally valid summation order lands within a small multiple of another implementation's error.  Where the float32 oracle is
exact the bound is 0 and the GPU has to be exact as well."""
import numpy as np
import pytest

from tests import emb_oracle as EO
from tests import fbank_oracle as FO
from tests.native_variant import library_variant

pytestmark = pytest.mark.gpu

SR = 16000
FACTOR = 4.0
# rows -> positions after the tdnn {2, 2, 3, 3, 5, 100, 100, 101, 101, 199, 200, 201, 301}: odd and even rows at the stride, fewer
# positions than the dilation, exactly one, one plus one, two, two plus one and three plus one context segments
ROWS = (3, 4, 5, 6, 9, 199, 200, 201, 202, 398, 399, 401, 601)
NAMES = ("embedding", "head", "out_nonlinear", "statistics")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def feats(rows, seed, scale=1.0):
    """seeded rows with the per-column mean removed, as the fbank delivers them"""
    x = np.random.default_rng(seed).standard_normal((rows, 80)) * scale
    return (x - x.mean(0)).astype(np.float32)


@pytest.fixture(scope="module")
def weights():
    return EO.make_weights(1)


@pytest.fixture(scope="module")
def oracles(weights):
    import torch
    return EO.CAMPPlus(weights, torch.float64), EO.CAMPPlus(weights, torch.float32)


@pytest.fixture(scope="module")
def diar(weights):
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    d.load_embedding(weights)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ragged():
    return [feats(t, 100 + t) for t in ROWS]


@pytest.fixture(scope="module")
def ragged_gpu(diar, ragged):
    """(embedding, heads, out_nonlinear, statistics) of all chunks in one ragged call; shared and left unchanged"""
    return diar.embed(ragged, taps=True)


def per_chunk(got, c):
    emb, heads, xvecs, stats = got
    return emb[c], heads[c], xvecs[c], stats[c]


def check(got, x, oracles, what):
    """got = (embedding, head, out_nonlinear, statistics) of the GPU on the chunk x -> asserts the ratios GPU / float32 oracle"""
    o64, o32 = oracles
    r64, r32 = o64.forward([x])[0], o32.forward([x])[0]
    ratios = []
    for name, g, a, b in zip(NAMES, got, r64, r32):
        assert g.shape == a.shape, (what, name, g.shape, a.shape)
        assert np.isfinite(g).all(), (what, name)
        yard = float(np.abs(b.astype(np.float64) - a).max())
        err = float(np.abs(g.astype(np.float64) - a).max())
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
        print(f"emb {what} {name}: float32 oracle {yard:.3e}, GPU {err:.3e} from float64 (ratio {ratio:.2f}, bound {FACTOR:g})")
        ratios.append((name, err, yard))
    for name, err, yard in ratios:
        assert err <= FACTOR * yard, (what, name, err, yard)


@pytest.mark.parametrize("c", range(len(ROWS)))
def test_ragged_values(diar, oracles, ragged, ragged_gpu, c):
    from crispy_amd.diarize import emb_frames
    assert diar.embedding_loaded and diar.embedding_dim == 512
    assert ragged_gpu[0].shape == (len(ROWS), 512) and ragged_gpu[3].shape == (len(ROWS), 1024)
    assert per_chunk(ragged_gpu, c)[2].shape == (emb_frames(ROWS[c]), 512)
    check(per_chunk(ragged_gpu, c), ragged[c], oracles, f"rows {ROWS[c]}")


def test_silent_constant_and_kaldi_scale_rows(diar, oracles):
    cases = {"all zeros": np.zeros((37, 80), np.float32),
             "constant over time": np.repeat(np.random.default_rng(7).uniform(-2, 2, (1, 80)).astype(np.float32), 64, 0),
             "rows at +-20": np.random.default_rng(8).choice(np.array([-20.0, 20.0], np.float32), (101, 80))}
    got = diar.embed(list(cases.values()), taps=True)
    for c, (what, x) in enumerate(cases.items()):
        check(per_chunk(got, c), x, oracles, what)


def test_bytes_alone_in_a_batch_and_in_turns(diar, weights, ragged, ragged_gpu):
    from crispy_amd.diarize import Diarizer
    for t in (398, 201):
        c = ROWS.index(t)
        mine = ragged[c]
        alone = diar.embed([mine], taps=True)
        first = diar.embed([mine, ragged[0], ragged[7]], taps=True)
        last = diar.embed(ragged[c + 1:] + ragged[:c + 1], taps=True)      # last of 13: the ragged list rotated
        for a, b, l, r in zip(per_chunk(alone, 0), per_chunk(first, 0), per_chunk(last, len(ROWS) - 1), per_chunk(ragged_gpu, c)):
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(l)) and np.array_equal(bits(a), bits(r))
    # the developer build with turns of 2 chunks: 2 + 2 + ... + 1, the bytes of the single turn
    with library_variant("dev", {"CRISPY_DIAR_EMB_TURN": "2"}):
        d = Diarizer(0)
        try:
            d.load_embedding(weights)
            turns = d.embed(ragged, taps=True)
        finally:
            d.close()
    for c in range(len(ROWS)):
        for a, b in zip(per_chunk(turns, c), per_chunk(ragged_gpu, c)):
            assert np.array_equal(bits(a), bits(b))


def pcm(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = 0.2 * np.sin(2 * np.pi * 180.0 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.05 * rng.standard_normal(n)
    return x.astype(np.float32)


def test_embed_chunks_equals_embed_on_the_fbank_rows(diar):
    import torch
    from crispy_amd.diarize import f32_to_i16
    f = pcm(5 * SR, 11)
    x = f32_to_i16(f)
    chunks = [(0, 64000), (1234, 720), (16000, 32000), (40000, 40000)]      # 398, 3, 198 and 248 rows
    want = diar.embed(diar.fbank(x, chunks))
    assert want.shape == (4, 512) and np.isfinite(want).all()
    assert np.array_equal(bits(diar.embed_chunks(x, chunks)), bits(want))
    assert np.array_equal(bits(diar.embed_chunks(f, chunks)), bits(want))      # f32 through f32_to_i16 on the device
    assert np.array_equal(bits(diar.embed_chunks_device(torch.from_numpy(x).cuda(), chunks).cpu().numpy()), bits(want))
    assert np.array_equal(bits(diar.embed_chunks_device(torch.from_numpy(f).cuda(), chunks).cpu().numpy()), bits(want))
    # the device form on the device rows
    rows, off = diar.fbank_device(torch.from_numpy(x).cuda(), chunks)
    dev = diar.embed([rows[off[c]:off[c + 1]] for c in range(len(chunks))])
    assert np.array_equal(bits(dev.cpu().numpy()), bits(want))


def test_limits_are_refused_before_a_launch(diar):
    from crispy_amd import _native as N
    x = np.zeros(SR, np.int16)
    with pytest.raises(N.CrispyError, match="2 rows") as e:
        diar.embed([feats(5, 1), feats(2, 2)])
    assert e.value.code == -1
    with pytest.raises(N.CrispyError, match="n_chunks 0") as e:
        diar.embed([])
    assert e.value.code == -1
    with pytest.raises(N.CrispyError, match="n_chunks 16385") as e:
        diar.embed([np.zeros((3, 80), np.float32)] * 16385)
    assert e.value.code == -1
    with pytest.raises(N.CrispyError, match="2 rows") as e:
        diar.embed_chunks(x, [(0, 4000), (0, 560)])
    assert e.value.code == -1
    with pytest.raises(N.CrispyError, match="n_chunks 0"):
        diar.embed_chunks(x, [])
    with pytest.raises(N.CrispyError, match="n_chunks 16385"):
        diar.embed_chunks(x, [(0, 4000)] * 16385)


def test_reload_at_another_width_and_forward_before_a_load(oracles):
    import torch
    from crispy_amd.diarize import Diarizer
    from crispy_amd import _native as N
    x = [feats(9, 31), feats(120, 32)]
    d = Diarizer(0)
    try:
        assert not d.embedding_loaded and d.embedding_dim == 0
        with pytest.raises(N.CrispyError, match="no embedding network is loaded") as e:
            d.embed(x)
        assert e.value.code == -1
        with pytest.raises(N.CrispyError, match="no embedding network is loaded"):
            d.embed_chunks(np.zeros(SR, np.int16), [(0, 8000)])
        d.load_embedding(EO.make_weights(1))
        assert d.embedding_loaded and d.embedding_dim == 512
        first = d.embed(x, taps=True)
        for c in range(2):
            check(per_chunk(first, c), x[c], oracles, f"first load, chunk {c}")
        second_w = EO.make_weights(2, dim=192)
        d.load_embedding(second_w)
        assert d.embedding_dim == 192
        second = d.embed(x, taps=True)
        assert second[0].shape == (2, 192)
        second_oracles = (EO.CAMPPlus(second_w, torch.float64), EO.CAMPPlus(second_w, torch.float32))
        for c in range(2):
            check(per_chunk(second, c), x[c], second_oracles, f"second load (dim 192), chunk {c}")
    finally:
        d.close()


def test_run_diarization_without_a_callable():
    """(a) Composition, byte for byte: run_diarization(pcm, None, None, ...) against the same call with Diarizer.embed as emb_fn,
    on the segmentation fixture of tests/test_gpu_diar_seg.py (weights 1, classifier 9594, recording 100: 7 chunks)."""
    from crispy_amd import diarize as D
    from tests import seg_oracle as SO
    from tests.test_gpu_diar_seg import E2E_CLASSIFIER, E2E_RECORDING, E2E_WEIGHTS, recording
    x = recording(E2E_RECORDING)
    merge_gap, max_speakers = 0.5, 2
    d = D.Diarizer(0)
    try:
        with pytest.raises(ValueError, match="no embedding network is loaded"):
            D.run_diarization(x, lambda w: np.zeros((589, 7), np.float32), None, max_speakers, merge_gap, d)
        d.load_segmentation(SO.make_weights(E2E_WEIGHTS, classifier_seed=E2E_CLASSIFIER))
        d.load_embedding(EO.make_weights(1))
        calls = []

        def emb_fn(f):
            calls.append(len(f))
            return d.embed([f])[0]

        got = D.run_diarization(x, None, None, max_speakers, merge_gap, d)
        want = D.run_diarization(x, None, emb_fn, max_speakers, merge_gap, d)
    finally:
        d.close()
    assert len(calls) == 7 and min(calls) >= 3
    assert len(want) >= 1 and got == want, (got, want)


E2E_EMB_WEIGHTS = 3      # chosen on the CPU: see test_run_diarization_against_the_oracle


def test_run_diarization_against_the_oracle():
    """(b) The same call against the run with the float32 oracle as emb_fn.  A random network does not tell the synthetic
    stretches apart by speaker, so the clustering of its embeddings could ride on a near-tie; the embedding weights' seed was
    chosen on the CPU, against the oracles alone, over seeds 1 ... 30 on the segmentation fixture's 7 chunks (266, 287, 287, 244,
    244, 180, 279 rows): the float64 and the float32 oracle's embeddings give the same labels through tests/nme_sc_oracle.py with
    two speakers, and so do eight draws of the float32 embeddings perturbed by 4 x the yardstick (26 of the 30 seeds pass;
    seed 3: yardstick 3.6e-6, labels 0 1 0 0 0 1 1, eigengap margin 1.00, ratio margin 3.49, k-means margin 2.0 -- the widest
    of them).  The agreement and the margins are asserted here before anything is compared."""
    import torch
    from crispy_amd import diarize as D
    from tests import nme_sc_oracle as NO
    from tests import seg_oracle as SO
    from tests.test_gpu_diar_seg import E2E_CLASSIFIER, E2E_RECORDING, E2E_WEIGHTS, recording
    x = recording(E2E_RECORDING)
    w = EO.make_weights(E2E_EMB_WEIGHTS)
    o64, o32 = EO.CAMPPlus(w, torch.float64), EO.CAMPPlus(w, torch.float32)
    merge_gap, max_speakers = 0.5, 2
    seen = []

    def emb_fn(f):
        seen.append(np.array(f, np.float32))
        return o32.embed(f)

    d = D.Diarizer(0)
    try:
        d.load_segmentation(SO.make_weights(E2E_WEIGHTS, classifier_seed=E2E_CLASSIFIER))
        d.load_embedding(w)
        got = D.run_diarization(x, None, None, max_speakers, merge_gap, d)
        want = D.run_diarization(x, None, emb_fn, max_speakers, merge_gap, d)
    finally:
        d.close()
    e64 = np.stack([r[0] for r in o64.forward(seen)])
    e32 = np.stack([r[0] for r in o32.forward(seen)])
    yard = float(np.abs(e32 - e64).max())
    r64, r32 = NO.nme_sc(e64.astype(np.float32), max_speakers), NO.nme_sc(e32, max_speakers)
    print(f"end to end fixture: {len(seen)} chunks, yardstick {yard:.2e}, labels {r64['labels'].tolist()}, eigengap margin "
          f"{r64['gap_margin']:.3f}, ratio margin {r64['ratio_margin']:.3f}, k-means margin {r64['kmeans_margin']:.3f}")
    assert len(seen) == 7 and r64["k"] == 2 == r32["k"] and np.array_equal(r64["labels"], r32["labels"])
    assert r64["gap_margin"] > 0.5 and r64["ratio_margin"] > 1.0 and r64["kmeans_margin"] > 1.0
    rng = np.random.default_rng(0)
    for _ in range(4):
        p = NO.nme_sc((e32 + 4 * yard * rng.uniform(-1, 1, e32.shape)).astype(np.float32), max_speakers)
        assert p["k"] == 2 and np.array_equal(p["labels"], r64["labels"])
    assert len(want) >= 2 and got == want, (got, want)

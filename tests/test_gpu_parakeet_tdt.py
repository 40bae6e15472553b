"""GPU tests of Parakeet's TDT decoder (crispy_pk_tdt_*, include/crispy_hip.h) against tests/pk_tdt_oracle.py on seeded frames (no
encoder in this file): logits along the GPU's own path and the projected frames, the path itself, the shapes at which the loop can
go wrong (T' 0 ... 65 side by side, ends on the budget, overshoots, only blanks, no blanks, the prediction mask, exact ties, clip
counts around the row tile), batch, position, neighbour and call independence byte for byte, the host form, the catalog widths
once, and the interface.

Values (the rule of tests/test_gpu_parakeet_encoder.py): per clip, the GPU's largest distance to float64 stays within 4 x the float32
oracle's, both taken along the GPU's path.  Path: the GPU's steps equal the float64 oracle's free-running loop exactly; this is
claimed where every step's top-two gap among the token logits and among the duration logits is at least 16 x the float32 oracle's
largest logit error on the float64 path -- a flip needs a gap under 8 x -- and the condition is asserted here on every clip."""
import numpy as np
import pytest

from tests import pk_tdt_oracle as TO

pytestmark = pytest.mark.gpu

FACTOR = 4.0
CFG = TO.TINY_TDT


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def oracles(cfg, weights):
    import torch
    return TO.Tdt(cfg, weights, torch.float64), TO.Tdt(cfg, weights, torch.float32)


def ratio_of(got, r64, r32, what):
    yard = float(np.abs(r32.astype(np.float64) - r64).max()) if r64.size else 0.0
    err = float(np.abs(got.astype(np.float64) - r64).max()) if r64.size else 0.0
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    print(f"pk tdt {what}: float32 oracle {yard:.3e}, GPU {err:.3e} from float64 (ratio {ratio:.2f}, bound {FACTOR:g})")
    return err, yard


def check_values(o64, o32, e, steps, proj, logits, what):
    """the GPU's projected frames and its logits along its own path against the oracles"""
    assert proj.shape == (e.shape[0], o64.cfg.decoder_hidden) and logits.shape == (len(steps), o64.cfg.width)
    assert np.isfinite(proj).all() and np.isfinite(logits).all()
    rows = [ratio_of(proj, o64.project(e), o32.project(e), f"{what} projector")]
    rows.append(ratio_of(logits, o64.logits_along(e, steps), o32.logits_along(e, steps), f"{what} logits along {len(steps)} steps"))
    for err, yard in rows:
        assert err <= FACTOR * yard, (what, err, yard)


def check_path(o64, o32, e, steps, what):
    """the GPU's steps are the float64 oracle's, where the oracle's own gaps allow the claim -- which is asserted, not assumed"""
    want, logits = o64.decode(e, with_logits=True)
    if len(want):
        err = float(np.abs(o32.logits_along(e, want) - logits).max())
        gaps = TO.top_two_gaps(logits, o64.cfg.vocab)
        print(f"pk tdt {what}: {len(want)} steps, smallest top-two gap {min(gaps):.3e}, float32 oracle's error {err:.3e} (x {min(gaps) / err:.0f}, needs {TO.GAP_FACTOR:g})")
        assert min(gaps) >= TO.GAP_FACTOR * err, (what, gaps, err)
    assert steps.dtype == np.int32 and steps.shape == want.shape and np.array_equal(steps, want), (what, steps[:8], want[:8])
    return want


@pytest.fixture(scope="module")
def sets():
    """per weight set of the fixture: (weights, float64 oracle, float32 oracle, loaded handle)"""
    from crispy_amd import ParakeetTDT
    out = {}
    for name, (kw, seed) in TO.FIXTURE_SETS.items():
        w = TO.make_tdt_weights(CFG, seed, **kw)
        h = ParakeetTDT(0)
        h.load(CFG.as_dict(), w)
        out[name] = (w, *oracles(CFG, w), h)
    yield out
    for _w, _a, _b, h in out.values():
        h.close()


@pytest.fixture(scope="module")
def clips():
    return [TO.frames(t, CFG.hidden, seed) for _name, t, seed in TO.FIXTURE_CLIPS]


@pytest.fixture(scope="module")
def gpu(sets, clips):
    """per clip of the fixture (steps, projected frames, logits): each weight set's clips in one ragged call; shared, unchanged"""
    out = [None] * len(clips)
    for name in TO.FIXTURE_SETS:
        idx = [i for i, (which, _t, _s) in enumerate(TO.FIXTURE_CLIPS) if which == name]
        steps, proj, logits = sets[name][3].decode([clips[i] for i in idx], taps=True)
        for j, i in enumerate(idx):
            out[i] = (steps[j], proj[j], logits[j])
    return out


IDS = [f"{name}-T{t}" for name, t, _s in TO.FIXTURE_CLIPS]


@pytest.mark.parametrize("i", range(len(TO.FIXTURE_CLIPS)), ids=IDS)
def test_values_along_the_gpus_path(sets, clips, gpu, i):
    name, t, _seed = TO.FIXTURE_CLIPS[i]
    _w, o64, o32, h = sets[name]
    assert h.loaded and h.config == CFG.as_dict()
    steps, proj, logits = gpu[i]
    assert len(steps) <= TO.max_steps(CFG, t)
    check_values(o64, o32, clips[i], steps, proj, logits, IDS[i])


@pytest.mark.parametrize("i", range(len(TO.FIXTURE_CLIPS)), ids=IDS)
def test_path_is_the_float64_oracles(sets, clips, gpu, i):
    name, t, _seed = TO.FIXTURE_CLIPS[i]
    _w, o64, o32, _h = sets[name]
    steps = check_path(o64, o32, clips[i], gpu[i][0], IDS[i])
    if t == 0:
        assert len(steps) == 0
    else:
        assert steps[0, 1] == 0 and np.array_equal(steps[1:, 1], np.cumsum(steps[:, 2])[:-1])
        assert (steps[:, 1] < t).all() and (steps[:, 0] >= 0).all() and (steps[:, 0] < CFG.vocab).all()


def test_shapes_at_which_the_loop_can_go_wrong(gpu):
    """what the fixture covers, read off the GPU's own steps"""
    by = {IDS[i]: gpu[i][0] for i in range(len(IDS))}
    ends = {IDS[i]: int(gpu[i][0][-1, 1] + gpu[i][0][-1, 2]) - TO.FIXTURE_CLIPS[i][1] for i in range(len(IDS)) if len(gpu[i][0])}
    for name, t in (("stall-T1", 1), ("stall-T3", 3)):      # ends on the budget, all at one frame
        assert len(by[name]) == TO.max_steps(CFG, t) and ends[name] < 0 and (by[name][:, 0] != CFG.blank).all() and (by[name][:, 2] == 0).all()
    assert max(ends.values()) >= 2                                                   # a last jump past T' by more than one frame
    assert (by["blanks-T7"][:, 0] == CFG.blank).all() and len(by["blanks-T7"]) > 0      # only blanks
    assert (by["tokens-T7"][:, 0] != CFG.blank).all() and len(by["tokens-T7"]) > 0      # none
    assert len(by["mix-T0"]) == 0
    mix = [by[k] for k in IDS if k.startswith("mix-") and len(by[k])]
    both = [s for s in range(max(len(m) for m in mix))
            if {bool(m[s, 0] == CFG.blank) for m in mix if len(m) > s} == {True, False}]
    assert both, "no step at which some clips skip the prediction network while others run it"
    assert set(int(d) for m in mix for d in m[:, 2]) >= {1, 2, 3, 4}


def tie_weights(cfg):
    """integer-valued weights whose sums are exact in any order: decoder_projector gives a constant integer g, token rows 5, 70 and
    100 of the head are equal and the largest, duration rows 1 and 3 likewise"""
    rng = np.random.default_rng(11)
    w = {k: np.zeros(n, np.float32) for k, n in TO.tensor_list(cfg)}
    shape = {k: tuple(v.shape) for k, v in TO.TdtModules(cfg).state_dict().items()}
    w = {k: v.reshape(shape[k]) for k, v in w.items()}
    w["encoder_projector.weight"][:] = rng.integers(-1, 2, shape["encoder_projector.weight"])
    w["decoder.embedding.weight"][:] = rng.integers(-2, 3, shape["decoder.embedding.weight"])
    for k in w:
        if "lstm" in k:
            w[k][:] = rng.integers(-1, 2, shape[k])
    w["decoder.decoder_projector.bias"][:] = rng.integers(0, 3, shape["decoder.decoder_projector.bias"])
    head = rng.integers(-1, 2, shape["joint.head.weight"]).astype(np.float32)
    head[70] = head[100] = head[5]
    head[cfg.vocab + 3] = head[cfg.vocab + 1]
    w["joint.head.weight"][:] = head
    w["joint.head.bias"][[5, 70, 100, cfg.vocab + 1, cfg.vocab + 3]] = 4096.0
    return w


def test_ties_go_to_the_lowest_index():
    """two column tiles apart (5 and 70, 100) and inside one (the durations), exact in f32"""
    from crispy_amd import ParakeetTDT
    cfg = TO.TdtConfig(hidden=256, decoder_hidden=128, decoder_layers=2, vocab=130, blank=129)
    w = tie_weights(cfg)
    clips = [np.random.default_rng(s).integers(-3, 4, (t, 256)).astype(np.float32) for s, t in ((1, 6), (2, 1), (3, 9))]
    h = ParakeetTDT(0)
    try:
        h.load(cfg.as_dict(), w)
        steps, _proj, logits = h.decode(clips, taps=True)
    finally:
        h.close()
    o64, _o32 = oracles(cfg, w)
    for e, s, l in zip(clips, steps, logits):
        t = e.shape[0]
        assert np.array_equal(s, np.stack([np.full(t, 5), np.arange(t), np.ones(t, int)], 1)), s
        assert np.array_equal(s, o64.decode(e))
        assert np.array_equal(bits(l[:, 5]), bits(l[:, 70])) and np.array_equal(bits(l[:, 5]), bits(l[:, 100]))
        assert np.array_equal(bits(l[:, cfg.vocab + 1]), bits(l[:, cfg.vocab + 3]))
        assert (l[:, :cfg.vocab].max(1) == l[:, 5]).all() and (l[:, cfg.vocab:].max(1) == l[:, cfg.vocab + 1]).all()
        assert np.array_equal(l.astype(np.float64), o64.logits_along(e, s))      # integers: exact, whatever the order


@pytest.mark.parametrize("n", [1, 2, 17], ids=["one clip", "two clips", "row tile + 1"])
def test_clip_counts_around_the_row_tile(sets, n):
    from crispy_amd import _native as N
    assert N.PK_TDT_ROWS == 16
    _w, o64, o32, h = sets["mix"]
    clips = [TO.frames(1 + (c * 5) % 9, CFG.hidden, 500 + c) for c in range(n)]
    steps, proj, logits = h.decode(clips, taps=True)
    assert len(steps) == n
    for c in (0, n - 1):
        check_values(o64, o32, clips[c], steps[c], proj[c], logits[c], f"{n} clips, clip {c}")
    alone = [h.decode([e], taps=True) for e in clips]
    for c in range(n):      # every clip: its bytes alone, and the oracle's path
        for a, b in zip((steps[c], proj[c], logits[c]), (alone[c][0][0], alone[c][1][0], alone[c][2][0])):
            assert np.array_equal(bits(a), bits(b)), (n, c)
        check_path(o64, o32, clips[c], steps[c], f"{n} clips, clip {c}")


def test_bytes_alone_rotated_beside_loud_neighbours_and_in_a_second_call(sets, clips, gpu):
    _w, _o64, _o32, h = sets["mix"]
    n = len(TO.RAGGED_FRAMES)
    ragged = clips[:n]
    for i in (3, 5, 7):      # T' 5, 32, 65
        mine = ragged[i]
        settings = {"alone": (h.decode([mine], taps=True), 0),
                    "rotated": (h.decode(ragged[i + 1:] + ragged[:i + 1], taps=True), n - 1),
                    "loud neighbours": (h.decode([TO.frames(40, CFG.hidden, 7, scale=1e4), mine, TO.frames(9, CFG.hidden, 8, scale=1e4)], taps=True), 1),
                    "second call": (h.decode([ragged[4], mine], taps=True), 1)}
        for what, (got, at) in settings.items():
            for a, b in zip(gpu[i], (got[0][at], got[1][at], got[2][at])):
                assert np.isfinite(np.asarray(b, np.float64)).all() and np.array_equal(bits(a), bits(b)), (i, what)


def test_host_form_equals_device_form(sets, clips, gpu):
    import torch
    _w, _o64, _o32, h = sets["mix"]
    n = len(TO.RAGGED_FRAMES)
    dev = h.decode_device([torch.from_numpy(x).cuda() for x in clips[:n]], taps=True)
    for c in range(n):
        for part, want in zip(dev, gpu[c]):
            assert np.array_equal(bits(part[c].cpu().numpy()), bits(want)), c
    plain = h.decode(clips[:n])
    plain_dev = h.decode_device([torch.from_numpy(x).cuda() for x in clips[:n]])
    for c in range(n):
        assert np.array_equal(plain[c], gpu[c][0]) and np.array_equal(plain_dev[c].cpu().numpy(), gpu[c][0])


def test_catalog_widths_once():
    """D 640, L 2, V 8193, 5 durations, H 1024: the real K-loop lengths, 129 column tiles with the durations in the last"""
    from crispy_amd import ParakeetTDT
    cfg = TO.CATALOG_TDT
    w = TO.make_tdt_weights(cfg, TO.CATALOG_SEED, **TO.MIX)
    o64, o32 = oracles(cfg, w)
    clips = [TO.frames(t, cfg.hidden, 700 + t) for t in TO.CATALOG_FRAMES]
    h = ParakeetTDT(0)
    try:
        h.load(cfg.as_dict(), w)
        steps, proj, logits = h.decode(clips, taps=True)
    finally:
        h.close()
    for c, e in enumerate(clips):
        what = f"catalog widths T' {e.shape[0]}"
        check_values(o64, o32, e, steps[c], proj[c], logits[c], what)
        check_path(o64, o32, e, steps[c], what)


def test_limits_are_refused_and_the_handle_still_works(sets, clips, gpu):
    from crispy_amd import _native as N
    _w, _o64, _o32, h = sets["mix"]
    ok = clips[3]
    for bad, text in (([ok, np.zeros((5001, 256), np.float32)], "clip 1 has 5001 frames"), ([], "n_clips 0"),
                      ([np.zeros((1, 256), np.float32)] * 4097, "n_clips 4097")):
        with pytest.raises(N.CrispyError, match=text) as e:
            h.decode(bad)
        assert e.value.code == -1
    from crispy_amd.parakeet import pk_tdt_max_steps
    for t in (0, 1, 5, 5000):
        assert pk_tdt_max_steps(h.config, t) == TO.max_steps(CFG, t)
    assert np.array_equal(h.decode([ok])[0], gpu[3][0])


def test_decode_before_load_and_a_reload_replaces_the_model(sets, clips, gpu):
    from crispy_amd import ParakeetTDT
    from crispy_amd import _native as N
    e = clips[3]
    h = ParakeetTDT(0)
    try:
        assert not h.loaded
        with pytest.raises(N.CrispyError, match="no decoder is loaded") as err:
            h.decode([e])
        assert err.value.code == -1
        with pytest.raises(N.CrispyError, match="no decoder is loaded"):
            _ = h.config
        with pytest.raises(N.CrispyError, match="joint.head.bias.*missing"):
            h.load(CFG.as_dict(), {k: v for k, v in sets["mix"][0].items() if k != "joint.head.bias"})
        assert not h.loaded
        h.load(CFG.as_dict(), sets["mix"][0])
        assert np.array_equal(h.decode([e])[0], gpu[3][0])
        h.load(CFG.as_dict(), sets["tokens"][0])      # the same shape, another model
        got = h.decode([e])[0]
        assert (got[:, 0] != CFG.blank).all() and np.array_equal(got, sets["tokens"][1].decode(e))
        cfg = TO.TdtConfig(hidden=128, decoder_hidden=256, decoder_layers=1, vocab=70, blank=0, durations=(1, 2, 5), max_symbols_per_step=3)
        w = TO.make_tdt_weights(cfg, 5, blank_bias=4.0, duration_bias=(0.0, 0.0, 0.0))
        h.load(cfg.as_dict(), w)      # another shape: one layer, blank first, three durations without a zero
        assert h.config == cfg.as_dict()
        o64, o32 = oracles(cfg, w)
        e2 = TO.frames(23, 128, 9)
        steps, proj, logits = h.decode([e2], taps=True)
        check_values(o64, o32, e2, steps[0], proj[0], logits[0], "second load (H 128, D 256, L 1, V 70)")
        check_path(o64, o32, e2, steps[0], "second load")
    finally:
        h.close()

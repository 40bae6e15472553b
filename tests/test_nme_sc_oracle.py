"""CPU tests of tests/nme_sc_oracle.py, the numpy restatement of the reference's speaker clustering: the reference's own
unit tests (src-tauri/src/managers/diarization.rs:753-782, 817-960) restated against it.

On the reference's axis-aligned cluster_emb inputs the graph at p = 1 falls into star components whose eigenvalues are
exactly {0, 1, ..., 1, 2}; several eigengaps then tie exactly and "the first maximum wins" holds only in exact
arithmetic.  The reference's expectation is asserted where the oracle's margins are not zero; a tie is reported
(test_cluster_emb_ties_are_ties) instead of being tuned away.

One of the reference's expectations does not follow from its arithmetic: nme_sc_single_speaker (:765-769) expects one
label for cluster_emb(&[0], 6, 6), six vectors (1, 0, 0, 0, 0, 0.010 ... 0.015) that fan out by about 0.001 rad each.
The nearest neighbour of a vector is the next one (the angles shrink with the index), so the graph at p = 1 is a path
(in f32: the path 0-1-2-3 and the pair 4-5), p* = 1 by a wide margin (ratio 0.17 against 0.47 at p = 2), and the largest
eigengap of a path sits in the middle: k = 3 with a gap margin of 0.5, in exact arithmetic (P6: gaps .19 .5 .62 .5 .19)
as in f32.  The test below asserts what the arithmetic gives and says so; NOTEBOOK records it."""
import numpy as np
import pytest

from tests import nme_sc_oracle as O

CASES = {"two": ([0, 1], 5, 6, 8, 2), "three": ([0, 1, 2], 5, 6, 8, 3), "single": ([0], 6, 6, 8, 1), "capped": ([0, 1, 2], 5, 6, 2, None)}


@pytest.fixture(scope="module")
def runs():
    return {k: (O.nme_sc(O.cluster_emb(c, per, dim), ms, "f64"), O.nme_sc(O.cluster_emb(c, per, dim), ms, "f32"))
            for k, (c, per, dim, ms, _) in CASES.items()}


def decisive(r):
    return r["gap_margin"] > 0 and r["ratio_margin"] > 0 and r["kmeans_margin"] > 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_unit_tests_where_the_oracle_is_decisive(runs, name):
    r64, r32 = runs[name]
    want = CASES[name][4]
    print(f"{name}: p*={r64['p_star']} k={r64['k']} gap margin {r64['gap_margin']:.3g} ratio margin {r64['ratio_margin']:.3g} "
          f"k-means margin {r64['kmeans_margin']:.3g} labels {r64['labels'].tolist()} (f32 run: k={r32['k']})")
    if name == "capped":
        assert len(set(r64["labels"].tolist())) <= 2 and len(set(r32["labels"].tolist())) <= 2      # holds whatever the ties
        return
    if name == "single":
        # the reference expects 1 label; its arithmetic gives 3, decisively (module docstring)
        assert decisive(r64) and r64["gap_margin"] > 0.4 and r64["p_star"] == 1
        assert r64["labels"].tolist() == [0, 0, 1, 1, 2, 2] and r32["labels"].tolist() == [0, 0, 1, 1, 2, 2]
        return
    if decisive(r64):
        assert len(set(r64["labels"].tolist())) == want, r64


def test_cluster_emb_ties_are_ties(runs):
    """What NOTEBOOK records: which of the reference's inputs are decided by an exact tie (gap margin 0 at p*)."""
    tied = sorted(k for k, (r64, _) in runs.items() if not decisive(r64))
    print("tied cluster_emb cases:", tied)
    for k in tied:
        r64 = runs[k][0]
        assert min(r64["gap_margin"], r64["ratio_margin"], r64["kmeans_margin"]) <= 1e-6      # a tie to rounding, not a near miss


def test_trivial_small_input():
    assert O.nme_sc(np.array([[1.0, 0.0]], np.float32), 8)["labels"].tolist() == [0]
    assert O.nme_sc(np.array([[1.0, 0.0], [0.0, 1.0]], np.float32), 8)["labels"].tolist() == [0, 0]
    assert O.nme_sc(np.zeros((0, 4), np.float32), 8)["labels"].tolist() == []


def test_cosine_distance_cases():
    def dist(a, b):
        return 1.0 - float(O.affinity(np.array([a, b], np.float32))[0, 1])      # similarity = clamp(1 - distance)
    assert abs(dist([1, 2, 3], [1, 2, 3])) < 1e-3
    assert abs(dist([1, 0], [0, 1]) - 1.0) < 1e-3
    assert dist([1, 0], [-1, 0]) == 1.0            # distance 2 -> similarity clamps at 0
    assert dist([0, 0], [1, 1]) == 1.0             # a zero vector: distance 1
    aff = O.affinity(np.array([[1, 0], [0, 0], [1, 0]], np.float32))
    assert aff[0, 1] == 0 and aff[0, 2] == 1 and aff[0, 0] == 0 and (aff == aff.T).all()


def test_laplacian_properties():
    emb = O.gaussian_clusters(3, 3, 5, 16, 0.8)
    aff = O.affinity(emb)
    for p in range(1, O.p_max_of(15) + 1):
        lap = O.pruned_normalized_laplacian(aff, p)
        # (dinv[i] * a) * dinv[j] rounds differently from (dinv[j] * a) * dinv[i]: symmetric to an ulp, not to the bit
        assert lap.dtype == np.float32 and np.abs(lap - lap.T).max() <= 2.0 ** -23
        w = np.linalg.eigvalsh(lap.astype(np.float64))
        assert w[0] > -1e-6 and w[-1] < 2 + 1e-6 and abs(w[0]) < 1e-6
        assert ((lap != 0).sum(1) - 1 >= min(p, 14)).all()      # every row keeps at least its own p neighbours
    # ties keep the lower index: duplicated rows
    emb = np.array([[1, 0], [1, 0.1], [1, 0.1], [0, 1]], np.float32)
    lap = O.pruned_normalized_laplacian(O.affinity(emb), 1)
    assert lap[0, 1] != 0 and lap[0, 2] == 0


def test_max_eigengap_first_maximum_and_clamp():
    ev = np.array([0, 0, 0.5, 1.0, 1.0], np.float32)
    assert O.max_eigengap(ev, 8) == (2, np.float32(0.5))            # gaps 0, .5, .5, 0: the first
    assert O.max_eigengap(ev, 1) == (1, np.float32(0.0))
    assert O.max_eigengap(np.array([0.5, 0.25], np.float32), 4) == (1, np.float32(0.0))      # negative gap: max(0)


def test_kmeans_rules():
    pts = np.array([[0, 0], [0, 0.1], [5, 5], [5, 5.1], [9, 0]], np.float32)
    labels, margin, _ = O.kmeans(pts, 3)
    assert labels.tolist() == [0, 0, 2, 2, 1] and margin > 1      # seeds: point 0, the farthest (9, 0), then (5, 5.1)
    assert O.kmeans(pts, 1)[0].tolist() == [0] * 5 and O.kmeans(pts, 5)[0].tolist() == [0, 1, 2, 3, 4]


def test_affinity_follows_f32_max_where_a_nan_arises():
    """:625 `(1.0 - (dot / ..)).max(0.0)`: f32::max returns the operand that is a number, so inf / inf gives distance 0 and
    similarity 1; a norm that underflows to 0 takes the `== 0.0` branch (:622): distance 1, similarity 0."""
    big, tiny, part = [1e20] * 3, [1e-25] * 3, [3e19, 1, -2]
    aff = O.affinity(np.array([big, [-1e20] * 3, tiny, part, [1, 2, 3], [3, 2, 1]], np.float32))
    assert np.isfinite(aff).all() and (aff == aff.T).all()
    assert aff[0, 1] == 1 and aff[0, 3] == 1 and aff[1, 3] == 1      # NaN quotients, the opposite rows 0 and 1 included
    assert not aff[2].any()                                          # 3e-50 is 0 in f32
    assert not aff[[0, 1, 3], 4:].any()                              # finite / inf = 0: distance 1
    assert abs(aff[4, 5] - 10 / 14) < 1e-6


def test_decide_is_the_sweep_of_the_reference():
    f = np.float32
    assert O.decide([[0, .25, .75, 1.25, 1.25, 1.5]], 6, 1, 8) == (1, 2, f(1) / f(6) / f(.5), f(.5))      # first of two equal gaps
    rows = [[0, .25, .25, .25, .25, .25], [0, 0, .5, .5, .5, .5]]
    p, k, ratio, gap, ratios = O.decide(rows, 6, 2, 8, trace=True)
    assert ratios[0].tobytes() == ratios[1].tobytes() and (p, k, gap) == (1, 1, f(.25))      # a tied ratio stays with the first p
    assert O.decide(rows[::-1], 6, 2, 8)[:2] == (1, 2)
    assert O.decide(np.full((3, 5), .75), 5, 3, 8) == (1, 1, f(f(1) / f(5)) / f(1e-6), f(0))      # the 1e-6 floor
    assert O.decide([[2, 1.5, 1.4, .5, 0]], 5, 1, 8)[1:] == (2, f(.2) / f(1e-6), f(0))              # unsorted: taken as it is
    ev = [[0, .1, .2, .35, .4, .5, 1.5, 1.6, 1.7, 1.8]]
    assert [O.decide(ev, 10, 1, ms)[1] for ms in (3, 5, 6, 50, 0, -3)] == [3, 3, 6, 6, 1, 1]      # kmax hides the gap at 6
    assert O.decide(ev, 2, 1, 8) == (0, 1, f(0), f(0)) and O.decide(ev, 0, 1, 8)[:2] == (0, 0) and O.decide(None, 9, 0, 8)[:2] == (0, 1)
    r = O.nme_sc(O.gaussian_clusters(8, 3, 11, 64, 0.5), 8)
    assert (r["p_star"], r["k"]) == (r["p_star"], 3) and r["ratio"].dtype == np.float32


def test_spectral_rows_threshold():
    v = np.array([[0, 0, 9], [5e-10, 0, 9], [2e-9, 0, 9], [3, 4, 9]], np.float32)
    got = O.spectral_rows(v, 2)
    assert got.dtype == np.float32 and np.array_equal(got, np.array([[0, 0], [5e-10, 0], [1, 0], [.6, .8]], np.float32))
    assert O.spectral_rows(v, 0).shape == (4, 0)


def test_kmeans_iteration_cap_and_details():
    pts = np.array([[0, 0], [0, 0.1], [5, 5], [5, 5.1], [9, 0]], np.float32)
    r = O.kmeans(pts, 3, details=True)
    assert r["labels"].tolist() == [0, 0, 2, 2, 1] and r["iterations"] == 2 and r["points"] is not None
    assert np.array_equal(r["centers"], np.array([[0, .05], [9, 0], [5, 5.05]], np.float32))
    assert O.kmeans(pts, 3)[0].tolist() == r["labels"].tolist() and len(O.kmeans(pts, 3)) == 3
    assert O.kmeans(pts, 5, details=True)["iterations"] == 0 and O.kmeans(pts, 5, details=True)["centers"] is None
    # a slow run: points crowded at one end of an arc; the cap cuts it, and each further iteration moves labels
    u = np.random.default_rng(5).random(2048)
    th = np.sort(u * u) * (np.pi / 2)
    arc = np.stack([np.cos(th), np.sin(th)], 1).astype(np.float32)
    free = O.kmeans(arc, 8, 1000, details=True)
    assert free["iterations"] == 61
    for cap in (1, 49, 50):
        capped = O.kmeans(arc, 8, cap, details=True)
        assert capped["iterations"] == cap and (capped["labels"] != free["labels"]).any()
    assert np.array_equal(O.kmeans(arc, 8)[0], O.kmeans(arc, 8, 50)[0])
    assert np.array_equal(O.kmeans(arc, 8, 61)[0], free["labels"])


def test_host_glue_reference_cases():
    assert O.speaker_segments([0.0, 1.1], [1.0, 2.0], [0, 0], 0.5) == [(0.0, 2.0, 1)]
    assert len(O.speaker_segments([0.0, 1.1], [1.0, 2.0], [0, 1], 0.5)) == 2
    assert len(O.speaker_segments([0.0, 5.0], [1.0, 6.0], [0, 0], 0.5)) == 2
    assert O.speaker_segments([], [], [], 0.5) == []
    gap = [(0.0, 3.0, 1), (7.0, 10.0, 2)]
    assert O.find_speaker(4.0, gap) == 1 and O.find_speaker(6.0, gap) == 2 and O.find_speaker(1.0, []) == 0
    assert O.format_diarized_text([(0.0, 0.5, "Hello"), (0.5, 1.0, "world")], []) == "Hello world"
    assert O.format_diarized_text([], []) == ""
    words = [(0.0, 0.5, "Hello"), (0.5, 1.0, "  "), (1.0, 1.5, "world")]
    assert O.format_diarized_text(words, [(0.0, 2.0, 1)]) == "[Speaker 1|0.0]\nHello world"
    assert O.rust_trim("\u00a0\u3000x\u200b \x1f\n") == "x\u200b \x1f"      # U+001F and U+200B are not White_Space

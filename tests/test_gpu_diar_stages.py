"""GPU tests of the speaker clustering stage by stage (crispy_diar_*_device, include/crispy_hip.h) at the edges the
end-to-end tests of tests/test_gpu_diar.py cannot reach, because they admit only inputs on which no decision is close:

* affinity, ranking and Laplacians bit for bit against tests/nme_sc_oracle.py above one block of every launch dimension
  (n > 64, > 256, = 2048) and on finite rows whose norms overflow or underflow;
* the decision and the k-means kernels through their own entry points, bit for bit on inputs made of ties, clamps, empty
  clusters and Lloyd runs that reach the cap of 50 iterations;
* the eigensolver at scales 2^-80 ... 2^100, on exact multiplicities and a mixed batch in its global-memory form, at
  orders 1 and 2, and at its sweep cap."""
import ctypes as C

import numpy as np
import pytest

from tests import nme_sc_oracle as O
from tests.test_gpu_diar import EIGH_CASES, EPS, LDS_N, bits, dev, stage_emb, star_blocks

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def diar():
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    yield d
    d.close()


# ---- affinity, ranking, Laplacians -----------------------------------------------------------------------------------
_STAGE = {}


def stage_ref(n, dim):
    """(embeddings, oracle affinity, oracle neighbour order), worked out once per module"""
    if (n, dim) not in _STAGE:
        emb = stage_emb(n, dim, 100 * n + dim)
        aff = O.affinity(emb)
        _STAGE[(n, dim)] = (emb, aff, O.neighbour_order(aff))
    return _STAGE[(n, dim)]


@pytest.mark.parametrize("n,dim", [(64, 6), (65, 6), (256, 6), (257, 6), (257, 1024), (300, 6), (2048, 6)])
def test_affinity_and_laplacians_above_one_block(diar, n, dim):
    """n = 64 / 65: one and two blocks of dinv_kernel; 256 / 257: one and two blocks in x of symrank_kernel and
    laplacian_kernel, and rank_kernel's threads striding over the row; 2048 fills row[kMaxN], and row 1 of stage_emb is
    the zero vector, whose affinities all tie at 0: its ranks run 0 ... 2046 in index order beside the 0xFFFF of the
    diagonal.  p >= n - 1 keeps every neighbour, whatever p."""
    emb, want, order = stage_ref(n, dim)
    assert not want[1].any() and np.array_equal(order[1], [j for j in range(n) if j != 1])      # the all-equal row
    d_aff = diar.affinity(dev(emb))
    got = d_aff.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (n, dim, np.abs(got - want).max())
    ps = [1, 2, O.p_max_of(n)] + ([n - 2, n - 1, n, 5000] if n == 257 else [])
    laps = {}
    for p in ps:
        laps[p] = diar.laplacian(d_aff, p).cpu().numpy()
        ref = O.pruned_normalized_laplacian(want, p, order)
        assert np.array_equal(bits(laps[p]), bits(ref)), (n, dim, p, np.abs(laps[p] - ref).max())
    if n == 257:
        assert laps[n - 1].tobytes() == laps[n].tobytes() == laps[5000].tobytes()


def extreme_emb():
    """Finite rows whose f32 norms leave the range, beside ordinary ones."""
    e = np.random.default_rng(77).standard_normal((7, 6)).astype(F)
    e[0] = 1e20                             # squares 1e40: norm inf
    e[1] = -1e20
    e[2] = 1e-25                            # squares 1e-50: norm 0
    e[3] = [3e19, 1, -2, 0.5, 1, 1]         # one square overflows, the others do not
    return e


def test_extreme_finite_rows(diar):
    """What cosine_distance / cosine_similarity (diarization.rs:412-414, 613-626) give in f32:
      rows 0 and 1, 0 and 3, 1 and 3: dot = +-inf and both norms inf, inf / inf = NaN, (1 - NaN).max(0.0) = 0 (f32::max
        returns the operand that is a number), similarity (1 - 0).clamp(0, 1) = 1 -- also for the opposite rows 0 and 1;
      row 2 and any row: its norm underflows to 0, the `norm == 0` branch: distance 1, similarity 0;
      rows 0, 1 or 3 and an ordinary row: finite dot / inf = 0, distance 1, similarity 0.
    The kernel's fmaxf has f32::max's rule; the oracle's np.fmax too.  Every affinity is finite, and so is all after it.

    crispy_diar_cluster takes the input; its labels are NOT compared: the oracle run is inadmissible (rows 0, 1 and 3 are
    at similarity exactly 1 and row 2 is isolated, so eigengaps and k-means distances tie exactly), which is asserted
    here; the call must return CRISPY_OK (Diarizer.cluster raises otherwise) with labels below its k."""
    emb = extreme_emb()
    assert np.isfinite(emb).all()
    want = O.affinity(emb)
    assert want[0, 1] == 1 and want[0, 3] == 1 and want[1, 3] == 1
    assert not want[2].any() and not want[[0, 1, 3], 4:].any() and np.isfinite(want).all()
    assert 0 < want[4, 6] < 1      # ordinary rows keep an ordinary cosine
    d_aff = diar.affinity(dev(emb))
    got = d_aff.cpu().numpy()
    assert np.array_equal(bits(got), bits(want)), (got, want)
    order = O.neighbour_order(want)
    for p in range(1, O.p_max_of(7) + 1):
        lap = diar.laplacian(d_aff, p).cpu().numpy()
        assert np.array_equal(bits(lap), bits(O.pruned_normalized_laplacian(want, p, order))), p
    r64, r32 = O.nme_sc(emb, 8, "f64"), O.nme_sc(emb, 8, "f32")
    assert O.admissible(7, r64, r32)      # reasons: the case is decided by exact ties
    labels, info = diar.cluster([emb], 8)
    assert info[0]["p_max"] == r64["p_max"] and 1 <= info[0]["k"] <= 6
    assert labels[0].min() >= 0 and labels[0].max() < info[0]["k"]
    assert np.isfinite(info[0]["ratio"]) and np.isfinite(info[0]["gap"])


# ---- decision --------------------------------------------------------------------------------------------------------
def check_decide(diar, evals, n, max_speakers):
    evals = np.ascontiguousarray(evals, dtype=F).reshape(-1, n)
    p_max = evals.shape[0]
    p_star, k, ratio, gap = O.decide(evals, n, p_max, max_speakers)
    got = diar.decide(dev(evals), n, max_speakers)
    assert (got["p_star"], got["k"], got["p_max"]) == (p_star, k, p_max), (got, p_star, k, n, max_speakers)
    assert F(got["ratio"]).tobytes() == F(ratio).tobytes() and F(got["gap"]).tobytes() == F(gap).tobytes(), (got, ratio, gap)
    return got


@pytest.mark.parametrize("n", [3, 4, 50, 2048])
def test_decide_random_spectra(diar, n):
    ev = np.sort(2 * np.random.default_rng(n).random((O.p_max_of(n), n)), 1).astype(F)
    ks = set()
    for ms in (1, 2, 8, n - 1, n + 5, 0, -3):
        ks.add(check_decide(diar, ev, n, ms)["k"])
    assert len(ks) > 1 or n == 3      # the cap changes the answer


def test_decide_ties_floor_and_clamps(diar):
    # two equal largest gaps (.5 at i = 2 and i = 3): the first
    got = check_decide(diar, [0, .25, .75, 1.25, 1.25, 1.5], 6, 8)
    assert got["k"] == 2 and got["gap"] == 0.5
    # ratios tied exactly across p: (1/n) / g and (2/n) / 2g are the same f32 (a factor of two is exact); p = 1 keeps it
    for n in (6, 8):
        rows = [[0, .25] + [.25] * (n - 2), [0, 0, .5] + [.5] * (n - 3), [0, .125] + [.125] * (n - 2)]
        ratios = O.decide(rows, n, 3, 8, trace=True)[4]
        assert ratios[0].tobytes() == ratios[1].tobytes() and ratios[2] > ratios[0]
        got = check_decide(diar, rows, n, 8)
        assert (got["p_star"], got["k"], got["gap"]) == (1, 1, 0.25)
    # all eigenvalues equal: gap 0, ratio (p / n) / 1e-6, k = 1, the first p
    got = check_decide(diar, np.full((3, 5), 0.75), 5, 8)
    assert (got["p_star"], got["k"], got["gap"]) == (1, 1, 0.0) and got["ratio"] == F(F(1) / F(5)) / F(1e-6)
    # a gap below the floor counts as the floor
    got = check_decide(diar, [[0, 1e-7, 1e-7, 1e-7], [0, 0, 3e-6, 3e-6]], 4, 8)
    assert (got["p_star"], got["k"]) == (2, 2) and got["gap"] == F(3e-6)
    got = check_decide(diar, [[0, 1e-7, 1e-7, 1e-7], [0, 0, 3e-7, 3e-7]], 4, 8)      # both floored: 1/4 < 2/4
    assert (got["p_star"], got["k"]) == (1, 1) and got["gap"] == F(1e-7) and got["ratio"] == F(0.25) / F(1e-6)
    # a descending spectrum, read as it is: every gap negative, the least negative gives k, the gap is clamped to 0
    got = check_decide(diar, [2, 1.5, 1.4, 0.5, 0], 5, 8)
    assert (got["k"], got["gap"]) == (2, 0.0)
    # the largest gap beyond kmax is not seen; one AT kmax is
    ev = [0, .1, .2, .35, .4, .5, 1.5, 1.6, 1.7, 1.8]
    assert (check_decide(diar, ev, 10, 3)["k"], check_decide(diar, ev, 10, 6)["k"], check_decide(diar, ev, 10, 5)["k"]) == (3, 6, 3)
    assert check_decide(diar, ev, 10, 3)["gap"] == F(.35) - F(.2)


def test_decide_trivial_inputs(diar):
    zero = dict(p_star=0, k=1, ratio=0.0, gap=0.0, p_max=0)
    assert diar.decide(dev(np.ones((2, 2), F)), 2, 8) == zero and diar.decide(dev(np.ones((1, 1), F)), 1, 8) == zero
    assert diar.decide(None, 5, 8) == zero and diar.decide(None, 0, 8) == dict(zero, k=0)
    L, h = diar._L, diar._h
    info = (C.c_int * 5)()
    assert L.crispy_diar_decide_device(h, 1, 2049, 1, 8, info) == -1 and b"2048" in L.crispy_last_error()
    assert L.crispy_diar_decide_device(h, 1, -1, 1, 8, info) == -1 and L.crispy_diar_decide_device(h, 1, 5, -1, 8, info) == -1
    assert L.crispy_diar_decide_device(h, None, 5, 1, 8, info) == -1 and L.crispy_diar_decide_device(h, 1, 5, 1, 8, None) == -1


# ---- k-means ---------------------------------------------------------------------------------------------------------
def check_kmeans(diar, rows, k, max_iter=50):
    """rows [n][k or fewer columns] -> the oracle's result; the kernel's labels are the oracle's, its points and centres
    the oracle's bits.  The columns of `vecs` from k on hold a value no result may show."""
    rows = np.asarray(rows, F)
    n = rows.shape[0]
    vecs = np.full((n, n), 7.0, F)
    kk = min(k, n)
    vecs[:, :kk] = 0
    vecs[:, :min(kk, rows.shape[1])] = rows[:, :kk]
    ref = O.kmeans(O.spectral_rows(vecs, kk), k, max_iter, details=True)
    labels, pts, ctr = diar.kmeans(dev(vecs), k, details=True)
    assert labels.cpu().numpy().tolist() == ref["labels"].tolist()
    if 1 < k < n:
        assert np.array_equal(bits(pts.cpu().numpy()), bits(ref["points"]))
        assert np.array_equal(bits(ctr.cpu().numpy()), bits(ref["centers"]))
    else:
        assert pts is None and ctr is None
    assert np.array_equal(diar.kmeans(dev(vecs), k).cpu().numpy(), ref["labels"])      # without the optional outputs
    return ref


def test_kmeans_seeding_ties(diar):
    e = np.eye(3, dtype=F)
    # one-hot rows: every distance is exactly 0 or 2, every seeding step a tie among all points not yet covered
    ref = check_kmeans(diar, e[[0, 0, 1, 2, 1, 0, 2]], 3)
    assert ref["labels"].tolist() == [0, 0, 1, 2, 1, 0, 2]
    # n = 600: indices 50 (thread 50), 299 (thread 43) and 300 (thread 44) tie for the second seed: the lowest INDEX, 50, not
    # the lowest thread
    idx = np.zeros(600, np.int64)
    idx[50] = 1
    idx[299] = 2
    idx[300:450] = 1
    idx[450:] = 2
    ref = check_kmeans(diar, e[idx], 3)
    assert ref["labels"][[0, 50, 299, 300]].tolist() == [0, 1, 2, 1] and ref["iterations"] == 2
    # two distinct points, k = 3: the third seed is point 0 again (every distance 0, first of equals) and cluster 2 stays
    # empty with the centre it was given
    ref = check_kmeans(diar, e[[0, 1, 0, 1, 0]], 3)
    assert ref["labels"].tolist() == [0, 1, 0, 1, 0] and np.array_equal(ref["centers"], e[[0, 1, 0]])


def test_kmeans_assignment_tie_and_norm_threshold(diar):
    # (1, 1) / sqrt 2 is as far from e0 as from e1, to the bit (x == y after the division): the lower cluster takes it
    ref = check_kmeans(diar, [[1, 0], [0, 1], [1, 1], [1, 0], [0, 1]], 2)
    assert ref["points"][2, 0] == ref["points"][2, 1] and ref["labels"].tolist() == [0, 1, 0, 0, 1]
    # norms 0, 5e-10 and 2e-9 about the 1e-9 threshold: the first two rows stay as they are, the third becomes (1, 0)
    rows = np.concatenate([np.array([[0, 0], [5e-10, 0], [2e-9, 0], [0, -2e-9], [0, 1e-9]], F),
                           np.random.default_rng(3).standard_normal((6, 2)).astype(F)])
    ref = check_kmeans(diar, rows, 2)
    assert np.array_equal(ref["points"][:5], np.array([[0, 0], [5e-10, 0], [1, 0], [0, -1], [0, 1e-9]], F))
    check_kmeans(diar, rows, 3)


def test_kmeans_trivial_k_and_n(diar):
    rows = np.random.default_rng(4).standard_normal((5, 6)).astype(F)
    assert check_kmeans(diar, rows, 1)["labels"].tolist() == [0] * 5
    assert len(set(check_kmeans(diar, rows, 4)["labels"].tolist())) == 4
    for k in (5, 6):
        assert check_kmeans(diar, rows, k)["labels"].tolist() == [0, 1, 2, 3, 4]      # the k >= n branch
    for n in (0, 1, 2):
        for k in (1, 2, 3):
            want = list(range(n)) if k >= max(n, 2) else [0] * n
            assert check_kmeans(diar, rows[:n], k)["labels"].tolist() == want
    L, h = diar._L, diar._h
    assert L.crispy_diar_kmeans_device(h, 1, 2049, 2, 1, None, None) == -1 and b"2048" in L.crispy_last_error()
    assert L.crispy_diar_kmeans_device(h, 1, 5, 0, 1, None, None) == -1 and L.crispy_diar_kmeans_device(h, 1, -1, 2, 1, None, None) == -1
    assert L.crispy_diar_kmeans_device(h, None, 5, 2, 1, None, None) == -1 and L.crispy_diar_kmeans_device(h, 1, 5, 2, None, None, None) == -1
    assert L.crispy_diar_kmeans_device(h, None, 0, 2, None, None, None) == 0


def test_kmeans_largest_recording(diar):
    ref = check_kmeans(diar, np.random.default_rng(5).standard_normal((2048, 8)).astype(F), 8)
    assert len(set(ref["labels"].tolist())) == 8 and 1 < ref["iterations"] <= 50


def arc_rows(n, k, seed):
    """n points on a quarter of the unit circle in the first two of k columns, crowded towards angle 0: Lloyd's borders
    creep along the arc a few points per iteration."""
    u = np.random.default_rng(seed).random(n)
    th = np.sort(u * u) * (np.pi / 2)
    x = np.zeros((n, k), F)
    x[:, 0] = np.cos(th)
    x[:, 1] = np.sin(th)
    return x


def test_kmeans_long_runs_and_the_iteration_cap(diar):
    """Seeds found with the oracle alone (12 seeds each of n = 600 ... 2048, k = 3 ... 8): n = 2048, k = 8 takes 39
    iterations at seed 0 and 61 at seed 5, where the labels after 49, 50 and 51 iterations differ pairwise (in 7, 6 and 13
    points): a kernel that stops one iteration early or late is told from one that stops at 50."""
    rows = arc_rows(2048, 8, 0)
    ref = check_kmeans(diar, rows, 8)
    print("arc seed 0:", ref["iterations"], "iterations")
    assert 20 <= ref["iterations"] <= 45
    rows = arc_rows(2048, 8, 5)
    pts = O.spectral_rows(rows, 8)
    free = O.kmeans(pts, 8, 1000, details=True)["iterations"]
    l49, l50, l51 = (O.kmeans(pts, 8, cap)[0] for cap in (49, 50, 51))
    print("arc seed 5:", free, "iterations uncapped; labels differ 49/50, 50/51, 49/51 in",
          int((l49 != l50).sum()), int((l50 != l51).sum()), int((l49 != l51).sum()), "points")
    assert free > 50 and (l49 != l50).any() and (l50 != l51).any() and (l49 != l51).any()
    ref = check_kmeans(diar, rows, 8)
    assert ref["iterations"] == 50 and np.array_equal(ref["labels"], l50)


# ---- eigensolver -----------------------------------------------------------------------------------------------------
def check_eigh(diar, a, name, scale=1.0):
    """The checks of test_eigh_against_float64 on a * scale (scale a power of two, so the product is exact): eigenvalues and
    residual within bar = n * eps * |a * scale|_2.  The orthogonality of the vectors has no unit and does not scale with
    the matrix, so its bar is the one that test holds the same matrix to at scale 1, n * eps * |a|_2 = bar / scale."""
    n = a.shape[0]
    a = (a * F(scale)).astype(F)
    assert np.isfinite(a).all() and (a == a.T).all()
    a64 = a.astype(np.float64)
    w64 = np.linalg.eigvalsh(a64)
    norm2 = float(np.abs(w64).max())
    bar = n * EPS * norm2
    ev, vec = diar.eigh(dev(a[None]), True)
    ev_only, none = diar.eigh(dev(a[None]), False)
    w, v = ev[0].cpu().numpy().astype(np.float64), vec[0].cpu().numpy().astype(np.float64)
    assert none is None and np.array_equal(bits(ev_only[0].cpu().numpy()), bits(ev[0].cpu().numpy()))
    assert (np.diff(w) >= 0).all()
    e_val = np.abs(w - w64).max()
    e_res = np.abs(a64 @ v - v * w[None, :]).max()
    e_orth = np.abs(v.T @ v - np.eye(n)).max() * scale
    r = [e / bar if bar else (0.0 if e == 0 else np.inf) for e in (e_val, e_res, e_orth)]
    print(f"eigh {name}: n={n} |A|_2={norm2:.3g} bar={bar:.3g}  eigenvalues {e_val:.3g} ({r[0]:.2f} bar)  "
          f"residual {e_res:.3g} ({r[1]:.2f} bar)  orthogonality {e_orth / scale:.3g} ({r[2]:.2f} bar)")
    assert e_val <= bar and e_res <= bar and e_orth <= bar
    return ev[0].cpu().numpy(), vec[0].cpu().numpy()


@pytest.mark.parametrize("name,s", [("n33", -80), ("n33", -40), ("n33", 40), ("n33", 70), ("n33", 100),
                                    ("lds_limit_plus_1", -80), ("lds_limit_plus_1", 70)])
def test_eigh_at_any_scale(diar, name, s):
    """With the squares of the convergence test summed in f32 the test passed at once where they all overflow (2^70, 2^100)
    or all underflow (2^-80), and the solver returned the matrix after ONE sweep with status 0: eigenvalue errors of
    1e3 ... 1e4 bar in both forms.  n33 is the LDS form, lds_limit_plus_1 the global one."""
    check_eigh(diar, EIGH_CASES[name](), f"{name} * 2^{s}", 2.0 ** s)


GLOBAL_MULTIPLE = {
    "stars_193": lambda: star_blocks([50, 40, 3, 2, 98]),
    "stars_194": lambda: star_blocks([100, 94]),
    "identity_193": lambda: np.eye(193, dtype=F),
    "diagonal_193": lambda: np.diag(np.resize(np.array([3, -1, 0.5, 0.5, 2, 0, -1, 7], F), 193)),
}


@pytest.mark.parametrize("name", sorted(GLOBAL_MULTIPLE))
def test_eigh_global_form_exact_multiplicities(diar, name):
    a = GLOBAL_MULTIPLE[name]()
    assert a.shape[0] > LDS_N
    w, v = check_eigh(diar, a, name)
    if "stars" not in name:      # nothing to rotate: the sorted diagonal and a permutation, exactly
        assert np.array_equal(w, np.sort(np.diagonal(a))) and np.array_equal(np.sort(v, 0)[-1], np.ones(193, F)) and (v != 0).sum() == 193


def test_eigh_global_form_batch_of_matrices_is_the_matrices_alone(diar):
    """The identity is done at sweep 0 and the stars a sweep or more before the dense Laplacian: two of the three sit
    out (`active` 0, and 2 during their last sweep) while the launches over all three go on."""
    mats = np.stack([np.eye(193, dtype=F), star_blocks([50, 40, 3, 2, 98]), EIGH_CASES["lds_limit_plus_1"]()])
    assert mats.shape[1] == LDS_N + 1
    for vectors in (True, False):
        ev, vec = diar.eigh(dev(mats), vectors)
        for m in range(3):
            e1, v1 = diar.eigh(dev(mats[m:m + 1]), vectors)
            assert np.array_equal(bits(e1[0].cpu().numpy()), bits(ev[m].cpu().numpy())), (vectors, m)
            if vectors:
                assert np.array_equal(bits(v1[0].cpu().numpy()), bits(vec[m].cpu().numpy())), m
    assert np.array_equal(ev[0].cpu().numpy(), np.ones(193, F))


def test_eigh_orders_one_and_two(diar):
    for x in (5.0, -3.0, 0.0):
        w, v = check_eigh(diar, np.array([[x]], F), f"[[{x}]]")
        assert w.tolist() == [x] and v.tolist() == [[1.0]]
    w, _ = check_eigh(diar, np.array([[2, 0.5], [0.5, 2]], F), "[[a, b], [b, a]]")
    assert w.tolist() == [1.5, 2.5]
    w, _ = check_eigh(diar, np.array([[-1, 3], [3, -1]], F), "[[a, b], [b, a]] b > |a|")
    assert w.tolist() == [-4.0, 2.0]
    w, v = check_eigh(diar, np.zeros((2, 2), F), "zero")
    assert w.tolist() == [0, 0] and v.tolist() == [[1, 0], [0, 1]]


@pytest.mark.parametrize("n", [4, 193])
def test_eigh_sweep_cap_is_an_error_and_the_handle_lives(diar, n):
    """A NaN never passes the convergence test: 40 sweeps of ordinary arithmetic, then CRISPY_ERR_INTERNAL (n = 4: the LDS
    form's status; 193: the global form's count of active matrices)."""
    import torch
    from crispy_amd import _native as N
    a = star_blocks([n - 2, 2])
    a[n // 2, n // 2] = np.nan
    d_a, d_w = dev(a), torch.zeros(n, dtype=torch.float32, device="cuda")
    rc = diar._L.crispy_diar_eigh_device(diar._h, d_a.data_ptr(), n, 1, d_w.data_ptr(), None)
    msg = diar._L.crispy_last_error()
    assert rc == N.ERR_INTERNAL and str(n).encode() in msg and b"sweeps" in msg, (rc, msg)
    good = star_blocks([n - 2, 2])
    check_eigh(diar, good, f"stars after the failed solve, n={n}")

"""GPU tests of the speaker clustering (crispy_diar_*, include/crispy_hip.h) against tests/nme_sc_oracle.py: affinity and
pruned Laplacians bit for bit, the symmetric eigensolver in both of its forms against float64 LAPACK within the
first-order bound of an orthogonal-similarity solver, nme_sc end to end on cases whose decisions the oracle shows to be
out of reach of an f32 solver's rounding, batch independence, the speaker cap and the argument errors."""
import ctypes as C

import numpy as np
import pytest

from tests import nme_sc_oracle as O

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
LDS_N = 192      # crispy_amd/csrc/diar_jacobi.h: kLdsN, the largest order of the one-workgroup form


@pytest.fixture(scope="module")
def diar():
    from crispy_amd.diarize import Diarizer
    d = Diarizer(0)
    yield d
    d.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stage_emb(n, dim, seed):
    """Gaussian rows with what the ranking has to get right: duplicated rows (exact ties), a zero vector (similarity 0
    to everything), a scaled copy (cosine 1 up to rounding)."""
    e = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    if n >= 4:
        e[n - 1] = e[0]
        e[1] = 0
    if n >= 7:
        e[4] = e[0]
        e[5] = 3 * e[2]
    return e


@pytest.mark.parametrize("n", [3, 4, 7, 33, 65])
def test_affinity_and_laplacians_bit_for_bit(diar, n):
    for dim in (1, 6, 192, 193):
        emb = stage_emb(n, dim, 100 * n + dim)
        want = O.affinity(emb)
        d_aff = diar.affinity(dev(emb))
        got = d_aff.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (n, dim, np.abs(got - want).max())
        order = O.neighbour_order(want)
        for p in range(1, O.p_max_of(n) + 1):
            lap = diar.laplacian(d_aff, p).cpu().numpy()
            ref = O.pruned_normalized_laplacian(want, p, order)
            assert np.array_equal(bits(lap), bits(ref)), (n, dim, p, np.abs(lap - ref).max())


def star_blocks(sizes):
    """block-diagonal normalised Laplacians of star graphs: eigenvalues 0, 1 (m - 2 times), 2 per star of m nodes"""
    n = sum(sizes)
    a = np.zeros((n, n))
    o = 0
    for m in sizes:
        a[o, o + 1:o + m] = a[o + 1:o + m, o] = 1
        o += m
    d = 1 / np.sqrt(a.sum(1))
    return (np.eye(n) - d[:, None] * a * d[None, :]).astype(np.float32)


def oracle_laplacian(seed, speakers, per, dim, noise, p):
    lap = O.pruned_normalized_laplacian(O.affinity(O.gaussian_clusters(seed, speakers, per, dim, noise)), p)
    return np.tril(lap) + np.tril(lap, -1).T      # the lower triangle, as LAPACK reads it


EIGH_CASES = {
    "diagonal": lambda: np.diag(np.array([3, -1, 0.5, 0.5, 2, 0, -1, 7], np.float32)),
    "identity": lambda: np.eye(9, dtype=np.float32),
    "stars": lambda: star_blocks([4, 3, 6, 2]),
    "stars_odd": lambda: star_blocks([5, 5, 3]),
    "two_tiny_offdiag": lambda: np.array([[1e-3, 1e-30], [1e-30, 1e-3]], np.float32),
    "two_unit_offdiag": lambda: np.array([[1e-3, 1.0], [1.0, 1e-3]], np.float32),
    "n5": lambda: oracle_laplacian(1, 2, [3, 2], 8, 0.5, 2),
    "n7": lambda: oracle_laplacian(2, 2, [4, 3], 8, 0.5, 2),
    "n33": lambda: oracle_laplacian(3, 3, 11, 64, 0.5, 4),
    "lds_limit": lambda: oracle_laplacian(4, 3, 64, 32, 0.6, 9),
    "lds_limit_plus_1": lambda: oracle_laplacian(5, 3, [64, 64, 65], 32, 0.6, 9),
    "n300": lambda: oracle_laplacian(1, 3, 100, 192, 0.7, 4),
}


@pytest.mark.parametrize("name", sorted(EIGH_CASES))
def test_eigh_against_float64(diar, name):
    """Eigenvalues within n * eps * |A|_2 of float64 eigvalsh (= 2 n eps for a normalised Laplacian: c = 1 in the
    first-order bound c n eps |A|_2), residual |AV - V Lambda|_max and orthogonality |V^T V - I|_max within the same."""
    a = EIGH_CASES[name]()
    n = a.shape[0]
    assert (a == a.T).all()
    if name == "lds_limit":
        assert n == LDS_N
    if name == "lds_limit_plus_1":
        assert n == LDS_N + 1
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
    e_orth = np.abs(v.T @ v - np.eye(n)).max()
    print(f"eigh {name}: n={n} |A|_2={norm2:.3g} bar={bar:.3g}  eigenvalues {e_val:.3g} ({e_val / bar:.2f} bar)  "
          f"residual {e_res:.3g} ({e_res / bar:.2f} bar)  orthogonality {e_orth:.3g} ({e_orth / bar:.2f} bar)")
    assert e_val <= bar and e_res <= bar and e_orth <= bar


def test_eigh_batch_of_matrices_is_the_matrices_alone(diar):
    mats = np.stack([oracle_laplacian(3, 3, 11, 64, 0.5, p) for p in (1, 3, 8)])
    ev, vec = diar.eigh(dev(mats), True)
    for m in range(3):
        e1, v1 = diar.eigh(dev(mats[m:m + 1]), True)
        assert np.array_equal(bits(e1[0].cpu().numpy()), bits(ev[m].cpu().numpy()))
        assert np.array_equal(bits(v1[0].cpu().numpy()), bits(vec[m].cpu().numpy()))


# (seed, speakers, cluster size(s), dim, noise, max_speakers): Gaussian clusters; speakers == 0: plain N(0, I) rows.
# Seeds chosen with the oracle alone (nme_sc_oracle.first_appearance_order says how); n = 5 takes max_speakers = 2 because
# with kmax = n - 1 the forest at p = 1 has a spectrum symmetric about 1 and its largest eigengap ALWAYS ties.
E2E_CASES = [(10, 3, 5, 16, 0.8, 8), (2, 2, 16, 32, 0.5, 8), (8, 3, 11, 64, 0.5, 8), (1, 4, 16, 192, 0.6, 8),
             (2, 5, 26, 192, 0.6, 8), (1, 3, 100, 192, 0.7, 8), (3, 0, 5, 8, 0.0, 2), (163, 0, 7, 8, 0.0, 8), (2374, 0, 7, 8, 0.0, 8)]


def e2e_emb(seed, speakers, per, dim, noise):
    if speakers == 0:
        return np.random.default_rng(seed).standard_normal((per, dim)).astype(np.float32)
    return O.gaussian_clusters(seed, speakers, per, dim, noise)


@pytest.mark.parametrize("case", E2E_CASES, ids=lambda c: "seed%d_%dx%s_dim%d" % c[:4])
def test_nme_sc_end_to_end_equals_the_float64_oracle(diar, case):
    seed, speakers, per, dim, noise, max_speakers = case
    emb = e2e_emb(seed, speakers, per, dim, noise)
    n = emb.shape[0]
    r64, r32 = O.nme_sc(emb, max_speakers, "f64"), O.nme_sc(emb, max_speakers, "f32")
    why = O.admissible(n, r64, r32)
    print(f"e2e n={n}: p*={r64['p_star']} k={r64['k']} gap margin {r64['gap_margin']:.3g} (bar {O.bar(n):.3g}) ratio margin "
          f"{r64['ratio_margin']:.3g} k-means margin {r64['kmeans_margin']:.3g} seeding margin {r64['seed_margin']:.3g}")
    assert not why, why      # an inadmissible case is a failure, never a skip
    if speakers:
        assert r64["k"] == speakers
    labels, info = diar.cluster([emb], max_speakers)
    assert (info[0]["p_star"], info[0]["k"], info[0]["p_max"]) == (r64["p_star"], r64["k"], r64["p_max"]), (info[0], r64)
    assert labels[0].tolist() == r64["labels"].tolist()
    assert abs(info[0]["gap"] - float(r64["gap"])) <= 2 * O.bar(n)
    assert abs(info[0]["ratio"] - float(r64["ratio"])) <= float(r64["ratio"]) * 4 * O.bar(n) / float(r64["gap"])


def test_batch_independence_and_device_form(diar):
    import torch
    recs = [np.zeros((0, 192), np.float32), e2e_emb(5, 0, 1, 192, 0), e2e_emb(6, 0, 2, 192, 0), e2e_emb(7, 0, 3, 192, 0),
            O.gaussian_clusters(4, 3, [20, 22, 23], 192, 0.6), O.gaussian_clusters(1, 3, 100, 192, 0.7)]
    assert [r.shape[0] for r in recs] == [0, 1, 2, 3, 65, 300]
    labels, info = diar.cluster(recs, 8)
    assert labels[0].size == 0 and labels[1].tolist() == [0] and labels[2].tolist() == [0, 0]
    assert (info[0]["k"], info[1]["k"], info[2]["k"], info[2]["p_max"]) == (0, 1, 1, 0)
    for i, r in enumerate(recs):
        solo_l, solo_i = diar.cluster([r], 8)
        assert solo_l[0].tobytes() == labels[i].tobytes(), i
        assert solo_i[0]["p_star"] == info[i]["p_star"] and solo_i[0]["k"] == info[i]["k"] and solo_i[0]["p_max"] == info[i]["p_max"]
        for f in ("ratio", "gap"):
            assert np.float32(solo_i[0][f]).tobytes() == np.float32(info[i][f]).tobytes(), (i, f)
    assert len(set(labels[5].tolist())) == 3 and info[5]["k"] == 3
    # reversed order in the call, and the device form
    rl, ri = diar.cluster(recs[::-1], 8)
    for i in range(len(recs)):
        assert rl[len(recs) - 1 - i].tobytes() == labels[i].tobytes() and ri[len(recs) - 1 - i] == info[i]
    n = np.array([r.shape[0] for r in recs], np.int32)
    d_labels, d_info = diar.cluster_device(dev(np.concatenate(recs, 0)), n, 8)
    torch.cuda.synchronize()
    assert d_labels.cpu().numpy().tobytes() == np.concatenate(labels).astype(np.int32).tobytes()
    for i in range(len(recs)):
        assert dict(p_star=d_info[i].p_star, k=d_info[i].k, ratio=d_info[i].ratio, gap=d_info[i].gap, p_max=d_info[i].p_max) == info[i]


def test_max_speakers_is_an_upper_bound(diar):
    emb = O.gaussian_clusters(8, 3, 11, 64, 0.5)
    full, _ = diar.cluster([emb], 8)
    two, i2 = diar.cluster([emb], 2)
    one, i1 = diar.cluster([emb], 1)
    zero, i0 = diar.cluster([emb], 0)
    neg, _ = diar.cluster([emb], -5)
    assert len(set(full[0].tolist())) == 3 and len(set(two[0].tolist())) <= 2 and i2[0]["k"] <= 2
    assert set(one[0].tolist()) == {0} and i1[0]["k"] == 1
    assert zero[0].tobytes() == one[0].tobytes() and i0[0] == i1[0] and neg[0].tobytes() == one[0].tobytes()


def test_errors_leave_the_handle_usable(diar):
    from crispy_amd import _native as N
    L, h = diar._L, diar._h
    emb = O.gaussian_clusters(10, 3, 5, 16, 0.8)
    good, _ = diar.cluster([emb], 8)
    lab = np.zeros(4096, np.int32)

    def call(e, n, dim, labels=lab):
        nn = (C.c_int * 1)(n)
        return L.crispy_diar_cluster(h, e.ctypes.data if e is not None else None, nn, 1, dim, 8,
                                     labels.ctypes.data if labels is not None else None, None)

    big = np.zeros((2049, 4), np.float32)
    assert call(big, 2049, 4) == -1 and b"2048" in L.crispy_last_error()
    assert call(emb, 15, 0) == -1
    assert call(emb, 15, 1025) == -1
    assert call(emb, -1, 16) == -1
    for bad in (np.nan, np.inf, -np.inf):
        e = emb.copy()
        e[7, 3] = bad
        assert call(e, 15, 16) == -1 and b"finite" in L.crispy_last_error()
        with pytest.raises(N.CrispyError):
            diar.cluster_device(dev(e), [15], 8)      # the device form finds it with a kernel of its own
    assert call(None, 15, 16) == -1 and call(emb, 15, 16, None) == -1
    n65 = (C.c_int * 65)(*([3] * 65))
    assert L.crispy_diar_cluster(h, emb.ctypes.data, n65, 65, 16, 8, lab.ctypes.data, None) == -1
    assert L.crispy_diar_cluster(h, emb.ctypes.data, None, 1, 16, 8, lab.ctypes.data, None) == -1
    assert L.crispy_diar_eigh_device(h, None, 4, 1, None, None) == -1
    assert L.crispy_diar_eigh_device(h, 1, 2049, 1, 1, None) == -1      # the order is checked before a pointer is touched
    assert L.crispy_diar_affinity_device(h, 1, 0, 4, 1) == -1 and L.crispy_diar_laplacian_device(h, 1, 4, 0, 1) == -1
    again, _ = diar.cluster([emb], 8)
    assert again[0].tobytes() == good[0].tobytes()

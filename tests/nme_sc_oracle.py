"""numpy restatement of the reference's speaker clustering and of its host glue (src-tauri/src/managers/diarization.rs:
311-338 chunking, 373-400 relabel / sort / merge, 412-626 nme_sc, 657-724 diarized text).  Test infrastructure.

The f32 parts (affinity, pruned Laplacian, eigengap decision, k-means) are f32 operation by f32 operation with sequential
sums, so the first two can be compared bit for bit.  The eigendecomposition is numpy.linalg.eigh in float64 on the f32
Laplacian (`solver="f64"`; its eigenvalues and vectors are then rounded to f32, what an exact f32 solver would return) or
in float32 (`solver="f32"`).  `nme_sc` also returns its decision margins, from the float64 eigenvalues."""
import math

import numpy as np

F = np.float32
EPS = 2.0 ** -24


def bar(n):
    """First-order eigenvalue error bound of an orthogonal-similarity f32 solver on a normalised Laplacian (norm <= 2)."""
    return 2.0 * n * EPS


def affinity(emb):
    """cosine_similarity (:412-414) of every pair, zero diagonal.  Where the quotient of cosine_distance (:625) is a NaN --
    finite rows whose norms overflow give inf / inf -- Rust's f32::max returns its other argument: (1 - NaN).max(0.0) = 0,
    the distance is 0 and the similarity (1 - 0).clamp(0, 1) = 1.  np.fmax has that rule (np.maximum would hand the NaN
    on); for every other value the two agree, so nothing else changes by a bit."""
    emb = np.asarray(emb, F)
    n, dim = emb.shape
    dot = np.zeros((n, n), F)
    nrm = np.zeros(n, F)
    with np.errstate(over="ignore", invalid="ignore"):
        for d in range(dim):
            c = emb[:, d]
            dot = dot + np.multiply.outer(c, c)
            nrm = nrm + c * c
    na, nb = nrm[:, None], nrm[None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dist = np.fmax(F(1) - dot / (np.sqrt(na) * np.sqrt(nb)), F(0))
    dist = np.where((na == 0) | (nb == 0), F(1), dist).astype(F)
    sim = np.clip(F(1) - dist, F(0), F(1)).astype(F)
    np.fill_diagonal(sim, F(0))
    return sim


def neighbour_order(aff):
    """row i: the j != i in the order of a stable descending sort of aff[i] (ties keep the lower index), [n][n-1]"""
    aff = np.asarray(aff, F)
    n = aff.shape[0]
    out = np.zeros((n, max(n - 1, 0)), np.int64)
    for i in range(n):
        idx = np.array([j for j in range(n) if j != i], np.int64)
        out[i] = idx[np.argsort(-aff[i, idx], kind="stable")]
    return out


def pruned_normalized_laplacian(aff, p, order=None):
    aff = np.asarray(aff, F)
    n = aff.shape[0]
    order = neighbour_order(aff) if order is None else order
    a = np.zeros((n, n), F)
    sel = order[:, :min(p, max(n - 1, 0))]
    rows = np.repeat(np.arange(n), sel.shape[1])
    a[rows, sel.ravel()] = aff[rows, sel.ravel()]
    a = np.maximum(a, a.T)
    s = np.zeros(n, F)
    for j in range(n):
        s = s + a[:, j]
    dinv = (F(1) / np.sqrt(np.maximum(s, F(1e-9)))).astype(F)
    x = (dinv[:, None] * a) * dinv[None, :]
    lap = (-x).astype(F)
    lap[np.arange(n), np.arange(n)] = F(1) - np.diagonal(x)
    return lap


def max_eigengap(ev, kmax):
    """ev: f32 ascending -> (k, gap) as the reference; gaps in f32, first maximum."""
    lim = min(kmax + 1, len(ev))
    best_k, best_gap = 1, F(np.finfo(F).min)
    for i in range(1, lim):
        gap = F(ev[i] - ev[i - 1])
        if gap > best_gap:
            best_gap, best_k = gap, i
    return max(best_k, 1), max(best_gap, F(0))


def p_max_of(n):
    return min(n - 1, max(int(math.sqrt(n)), 2) * 2)


def _sq_dist(pts, c):
    """sequential f32 sum of (x - y)^2 over the dimensions, for every row of pts"""
    s = np.zeros(pts.shape[0], F)
    for d in range(pts.shape[1]):
        t = pts[:, d] - c[d]
        s = s + t * t
    return s


def decide(evals, n, p_max, max_speakers, trace=False):
    """The sweep's decision (:570-582) on given eigenvalues: evals[p - 1] the f32 eigenvalues at p, taken as they are.
    -> (p_star, k, ratio, gap), ratio and gap f32; with `trace` also the list of every p's ratio.  n <= 2 or p_max <= 0:
    the zero decision (0, 1 or 0 for n == 0, 0, 0)."""
    if n <= 2 or p_max <= 0:
        out = (0, 1 if n else 0, F(0), F(0))
        return out + ([],) if trace else out
    kmax = min(max(max_speakers, 1), n - 1)
    best, ratios = None, []
    for p in range(1, p_max + 1):
        k, gap = max_eigengap(np.asarray(evals[p - 1], F), kmax)
        ratio = F(F(p) / F(n)) / max(gap, F(1e-6))
        ratios.append(ratio)
        if best is None or ratio < best[0]:
            best = (ratio, p, k, gap)
    ratio, p_star, k, gap = best
    out = (p_star, min(max(k, 1), kmax), F(ratio), F(gap))
    return out + (ratios,) if trace else out


def spectral_rows(vecs, k):
    """The first k columns of vecs [n][>= k], each row divided by its norm (sequential f32 sum of squares) where the norm
    is > 1e-9 (:598-609) -> f32 [n][k]"""
    x = np.array(np.asarray(vecs)[:, :k], F)
    s = np.zeros(x.shape[0], F)
    for c in range(k):
        s = s + x[:, c] * x[:, c]
    norm = np.sqrt(s)
    big = norm > F(1e-9)
    x[big] = x[big] / norm[big, None]
    return x


def kmeans(points, k, max_iter=50, details=False):
    """-> (labels, assignment margin over all iterations, seeding margin).  The seeding margin is, over the seeding steps,
    the distance of the chosen point minus the largest distance of a point that ends in ANOTHER cluster: choosing another
    point of the same cluster leaves the order of the clusters, and so the numbering of the labels, as it is.
    `max_iter` is the cap on Lloyd iterations (the reference's 50).  With `details` a dict instead: those three as
    labels / margin / seed_margin, `iterations` (assignment passes run, the one that changed nothing included), `points`
    (f32, as given) and `centers` (f32 [k][dim], final; None where k <= 1 or k >= n)."""
    pts = np.asarray(points, F)
    res = _kmeans(pts, k, max_iter)
    if not details:
        return res[:3]
    return dict(labels=res[0], margin=res[1], seed_margin=res[2], iterations=res[3], points=pts, centers=res[4])


def _kmeans(pts, k, max_iter):
    n = pts.shape[0]
    if k <= 1 or n == 0:
        return np.zeros(n, np.int64), math.inf, math.inf, 0, None
    if k >= n:
        return np.arange(n), math.inf, math.inf, 0, None
    dim = pts.shape[1]
    centers = [pts[0].copy()]
    steps = []
    while len(centers) < k:
        d = np.full(n, np.finfo(F).max, F)
        for c in centers:
            d = np.minimum(d, _sq_dist(pts, c))
        best = int(np.argmax(d))                 # first of equals, and d >= 0 > -1
        steps.append((d.astype(np.float64), best))
        centers.append(pts[best].copy())
    centers = np.array(centers, F)
    labels = np.zeros(n, np.int64)
    margin = math.inf
    iterations = 0
    zero = np.zeros((1, dim), F)
    for _ in range(max_iter):
        iterations += 1
        dist = np.stack([_sq_dist(pts, centers[c]) for c in range(k)], 1)
        new = np.argmin(dist, 1)                 # first of equals == strict `<`
        srt = np.sort(dist.astype(np.float64), 1)
        margin = min(margin, float((srt[:, 1] - srt[:, 0]).min()))
        changed = bool((new != labels).any())
        labels = new
        for c in range(k):
            members = np.nonzero(labels == c)[0]
            if len(members):      # 0 + p0 + p1 + ... in f32, in point order (an accumulate is sequential)
                s = np.add.accumulate(np.concatenate([zero, pts[members]], 0), 0, dtype=F)[-1]
                centers[c] = s / F(len(members))
        if not changed:
            break
    seed_margin = math.inf
    for d, best in steps:
        other = d[labels != labels[best]]
        if len(other):
            seed_margin = min(seed_margin, float(d[best] - other.max()))
    return labels, margin, seed_margin, iterations, centers


def eigh(lap, solver):
    if solver == "f64":
        w, v = np.linalg.eigh(lap.astype(np.float64))
    else:
        w, v = np.linalg.eigh(lap.astype(F))
    return w, v


def nme_sc(emb, max_speakers, solver="f64"):
    """-> dict(labels, p_star, k, ratio, gap, p_max, gap_margin, ratio_margin, kmeans_margin, seed_margin)"""
    emb = np.asarray(emb, F)
    n = emb.shape[0]
    out = dict(labels=np.zeros(n, np.int64), p_star=0, k=1 if n else 0, ratio=F(0), gap=F(0), p_max=0,
               gap_margin=math.inf, ratio_margin=math.inf, kmeans_margin=math.inf, seed_margin=math.inf)
    if n <= 2:
        return out
    kmax = min(max(max_speakers, 1), n - 1)
    aff = affinity(emb)
    p_max = p_max_of(n)
    order = neighbour_order(aff)
    evs, gap_margins = [], []
    for p in range(1, p_max + 1):
        w, _ = eigh(pruned_normalized_laplacian(aff, p, order), solver)
        evs.append(w.astype(F))
        g64 = np.sort(np.diff(w.astype(np.float64)[:min(kmax + 1, n)]))
        gap_margins.append(float(g64[-1] - g64[-2]) if len(g64) > 1 else math.inf)
    p_star, k, ratio, gap, ratios = decide(evs, n, p_max, max_speakers, trace=True)
    rs = sorted(float(r) for r in ratios)
    out.update(p_star=p_star, k=k, ratio=ratio, gap=gap, p_max=p_max, gap_margin=gap_margins[p_star - 1],
               ratio_margin=(rs[1] - rs[0]) / rs[0] if len(rs) > 1 else math.inf)
    if k <= 1:
        return out
    w, v = eigh(pruned_normalized_laplacian(aff, p_star, order), solver)
    idx = np.argsort(w, kind="stable")
    spectral = spectral_rows(v[:, idx[:k]].astype(F), k)
    labels, margin, seed_margin = kmeans(spectral, k)
    out.update(labels=labels, kmeans_margin=margin, seed_margin=seed_margin)
    return out


def admissible(n, r64, r32):
    """The conditions under which an f32 solver within bar(n) must reproduce the float64 oracle's decisions.  (The seeding
    margin is reported beside them, not among them: see first_appearance_order.)"""
    reasons = []
    if not (r64["p_star"] == r32["p_star"] and r64["k"] == r32["k"] and np.array_equal(r64["labels"], r32["labels"])):
        reasons.append("the float64 and float32 oracle runs disagree")
    if not r64["gap_margin"] >= 10 * bar(n):
        reasons.append(f"gap margin {r64['gap_margin']:.3g} < {10 * bar(n):.3g}")
    if not r64["ratio_margin"] >= 10 * (2 * bar(n) / float(r64["gap"])):
        reasons.append(f"ratio margin {r64['ratio_margin']:.3g} < {10 * 2 * bar(n) / float(r64['gap']):.3g}")
    if not r64["kmeans_margin"] >= 10 * bar(n):
        reasons.append(f"k-means margin {r64['kmeans_margin']:.3g} < {10 * bar(n):.3g}")
    return reasons


def first_appearance_order(labels):
    """True when label c first occurs before label c + 1.  Where p* cuts the graph into its k components the spectral rows
    of a cluster coincide and two rows of different clusters are at distance 2 EXACTLY (orthonormal rows), so every step of
    the farthest-point seeding is an exact tie between the clusters not yet taken: the first point wins, and the labels
    come out in order of first appearance.  A LAPACK basis of the k-fold eigenvalue 0 is an arbitrary rotation of that
    frame, its distances are 2 +- rounding, and the tie falls wherever the rounding puts it; the cases of the GPU test
    are seeds at which it falls on the exact answer (chosen with the oracle alone, on the CPU)."""
    seen = []
    for lb in labels:
        if lb not in seen:
            seen.append(lb)
    return seen == sorted(seen)


def gaussian_clusters(seed, speakers, per, dim, noise):
    """centres ~ N(0, I), points = centre + noise * N(0, I), rows shuffled -> f32 [sum of per, dim]; `per` is the size
    of every cluster or a list of sizes"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((speakers, dim))
    sizes = [per] * speakers if isinstance(per, int) else list(per)
    pts = np.concatenate([centres[s] + noise * rng.standard_normal((sizes[s], dim)) for s in range(speakers)], 0)
    return pts[rng.permutation(len(pts))].astype(F)


def cluster_emb(centers, per, dim):
    """the reference's test helper (:736-747)"""
    out = []
    for ci, c in enumerate(centers):
        for p in range(per):
            v = np.zeros(dim, F)
            v[c] = F(1)
            v[dim - 1] = v[dim - 1] + (F(0.01) * (F(ci) + F(1)) + F(0.001) * F(p))
            out.append(v)
    return np.array(out, F)


# ---- host glue ------------------------------------------------------------------------------------------------------
WHITE_SPACE = "".join(map(chr, [9, 10, 11, 12, 13, 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F,
                                 0x205F, 0x3000]))


def rust_trim(s):
    return s.strip(WHITE_SPACE)


def chunk_plan(segments, sample_rate=16000):
    out = []
    for si, (start, end, ns) in enumerate(segments):
        dur = end - start
        if dur > 4.0:
            chunks = int(math.ceil(dur / 4.0))
            cs = ns // chunks
            for i in range(chunks):
                a = i * cs
                b = ns if i == chunks - 1 else (i + 1) * cs
                out.append((start + a / sample_rate, start + b / sample_rate, si, a, b - a))
        else:
            out.append((start, end, si, 0, ns))
    return out


def speaker_segments(starts, ends, labels, merge_gap):
    order = []
    for lb in labels:
        if lb not in order:
            order.append(lb)
    segs = [(s, e, order.index(lb) + 1) for s, e, lb in zip(starts, ends, labels)]
    segs.sort(key=lambda x: x[0])            # stable
    merged = []
    for s, e, w in segs:
        if merged:
            ls, le, lw = merged[-1]
            if lw == w and max(s - le, 0.0) <= merge_gap:
                merged[-1] = (ls, max(e, le), lw)
                continue
        merged.append((s, e, w))
    return merged


def find_speaker(time, segments):
    for s, e, w in segments:
        if s <= time <= e:
            return w
    closest, best = 0, math.inf
    for s, e, w in segments:
        d = s - time if time < s else time - e
        if d < best:
            best, closest = d, w
    return closest


def speaker_name(w):
    return "Speaker ?" if w == 0 else f"Speaker {w}"


def format_diarized_text(words, segments):
    if not segments or not words:
        return " ".join(t for _, _, t in words)
    lines, cur, current = [], [], None
    for t0, t1, text in words:
        t = rust_trim(text)
        if not t:
            continue
        w = find_speaker((t0 + t1) / 2.0, segments)
        if w != current:
            if cur:
                lines.append(" ".join(cur))
                cur = []
            current = w
            lines.append("\n[%s|%s]" % (speaker_name(w), format(t0, ".1f")))
        cur.append(t)
    if cur:
        lines.append(" ".join(cur))
    return rust_trim("\n".join(lines))

"""Timing of the speaker clustering (crispy_diar_*, include/crispy_hip.h) on the MI355X, for NOTEBOOK and the README row:

  * one recording of n = 256, 1024 and 2048 chunks (dim 192, 4 speakers, max_speakers 8), wall time of crispy_diar_cluster;
  * 16 recordings of n = 256 in one call;
  * the stages of one recording through the stage entry points (each returns when its work is complete);
  * the comparison: the same sweep through numpy.linalg.eigvalsh in float32 on this machine's host -- a STAND-IN for the
    reference's nalgebra SymmetricEigen, which cannot be built here -- on the Laplacians the device produced.  Its
    eigenvalues also give the p* and k that the device's decision is checked against (the n = 2048 correctness run).

    python tools/diar_timing.py [--sizes 256,1024,2048] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import nme_sc_oracle as O      # noqa: E402


def wall(fn, reps=1):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from crispy_amd.diarize import Diarizer

    d = Diarizer(0)
    res = {"device": torch.cuda.get_device_name(0), "host_threads": os.environ.get("OMP_NUM_THREADS", "?"), "runs": []}
    warm = O.gaussian_clusters(1, 4, 16, 192, 0.6)
    d.cluster([warm], 8)
    for n in [int(x) for x in a.sizes.split(",")]:
        emb = O.gaussian_clusters(7, 4, n // 4, 192, 0.6)
        reps = 3 if n <= 256 else 1
        t_call, (labels, info) = wall(lambda: d.cluster([emb], 8), reps)
        run = {"n": n, "p_max": info[0]["p_max"], "p_star": info[0]["p_star"], "k": info[0]["k"], "cluster_ms": 1e3 * t_call}
        print(f"n={n}: crispy_diar_cluster {1e3 * t_call:.1f} ms  p_max={info[0]['p_max']} p*={info[0]['p_star']} k={info[0]['k']}", flush=True)
        # stages
        d_emb = torch.from_numpy(emb).cuda()
        t_aff, d_aff = wall(lambda: d.affinity(d_emb), reps)
        t_lap, laps = wall(lambda: torch.stack([d.laplacian(d_aff, p) for p in range(1, info[0]["p_max"] + 1)]))
        t_eig, (ev, _) = wall(lambda: d.eigh(laps, False))
        t_vec, _ = wall(lambda: d.eigh(laps[info[0]["p_star"] - 1:info[0]["p_star"]], True))
        run.update(affinity_ms=1e3 * t_aff, laplacians_ms=1e3 * t_lap, eigvals_sweep_ms=1e3 * t_eig, eigvecs_pstar_ms=1e3 * t_vec)
        print(f"   stages: affinity {1e3 * t_aff:.2f} ms, ranking + Laplacian x {info[0]['p_max']} (one call per p) {1e3 * t_lap:.1f} ms, "
              f"eigenvalues of the sweep {1e3 * t_eig:.1f} ms, vectors at p* {1e3 * t_vec:.1f} ms", flush=True)
        # stand-in host sweep on the same Laplacians, and the decision it leads to
        host_laps = laps.cpu().numpy()
        kmax = min(8, n - 1)

        def host_sweep():
            best = None
            for p in range(1, host_laps.shape[0] + 1):
                w = np.linalg.eigvalsh(host_laps[p - 1])
                k, gap = O.max_eigengap(w.astype(np.float32), kmax)
                ratio = np.float32(np.float32(p) / np.float32(n)) / max(gap, np.float32(1e-6))
                if best is None or ratio < best[0]:
                    best = (ratio, p, k)
            np.linalg.eigh(host_laps[best[1] - 1])
            return best
        t_host, best = wall(host_sweep)
        run.update(host_eigvalsh_f32_ms=1e3 * t_host, host_p_star=int(best[1]), host_k=int(best[2]))
        err = float(np.abs(np.sort(ev[best[1] - 1].cpu().numpy().astype(np.float64)) - np.linalg.eigvalsh(host_laps[best[1] - 1].astype(np.float64))).max())
        run["eigenvalue_error_at_pstar"] = err
        run["bar"] = O.bar(n)
        ok = (best[1], min(max(best[2], 1), kmax)) == (info[0]["p_star"], info[0]["k"])
        run["decision_equals_host"] = bool(ok)
        print(f"   host stand-in (numpy eigvalsh f32, same Laplacians): {1e3 * t_host:.0f} ms -> p*={best[1]} k={best[2]}  "
              f"{'EQUAL' if ok else 'DIFFERENT'}; eigenvalue error at p* {err:.3g} (bar {O.bar(n):.3g}); labels used: {sorted(set(labels[0].tolist()))}", flush=True)
        res["runs"].append(run)
    recs = [O.gaussian_clusters(20 + i, 4, 64, 192, 0.6) for i in range(16)]
    t16, (l16, i16) = wall(lambda: d.cluster(recs, 8), 3)
    t1, (l1, _) = wall(lambda: d.cluster(recs[:1], 8), 3)
    res["batch16_n256_ms"] = 1e3 * t16
    res["batch16_single_ms"] = 1e3 * t1
    res["batch16_first_equals_solo"] = bool(l16[0].tobytes() == l1[0].tobytes())
    print(f"16 recordings of n=256 in one call: {1e3 * t16:.1f} ms ({1e3 * t16 / 16:.1f} ms each; one alone {1e3 * t1:.1f} ms); "
          f"k = {[x['k'] for x in i16]}", flush=True)
    d.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

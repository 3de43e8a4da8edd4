"""Times of the marginal covariances (HipSolver.covariance / cuba_hip_compute_covariance) on the BASELINE shapes.

    python scripts/covariance_times.py kitti00 s2m g4m [--reps 5] [--iters 3] [--out file.json]

Per shape, after `iters` LM iterations: the selected inversion's plan (levels, factor tiles, gather entries, tile products, bytes of the
Sigma tiles and of the factor they sit beside), then for poses only and for poses + landmarks the device time of one computation
(median of `reps` repeats after one warm-up call that builds the plan and allocates; the handle's "covariance_ns" counter: from the
first launch to the stream synchronisation, before the results are copied out) and the wall time of the whole call; as context, the
time numpy takes for a dense inverse of the reduced matrix where it fits (<= 12 000 unknowns)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cuba_amd.capi import HipSolver, selinv_plan, sparse_plan  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_named  # noqa: E402

RK_HUBER = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))


def one(name, reps, iters):
    t0 = time.time()
    fp = flatten(synth_named(name))
    h = HipSolver(fp, RK_HUBER)
    h.optimize(iters)
    rp, ci = h.hsc_structure()
    plan = sparse_plan(rp, ci)
    sel = selinv_plan(rp, ci)
    out = dict(shape=name, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, hsc_blocks=len(ci), levels=plan["nLevels"], tiles=plan["nTiles"],
               tile_columns=plan["T"], factor_gather_entries=plan["entries"], selinv_gather_entries=sel["entries"],
               selinv_tile_products=sel["products"], sigma_bytes=8 * 1024 * plan["nTiles"], factor_bytes=8 * 1024 * (2 * plan["nTiles"] + 1))
    for label, lm in (("poses_only", False), ("poses_and_landmarks", True)):
        h.covariance(landmarks=lm)                              # warm-up: plan, allocations
        dev, wall = [], []
        for _ in range(reps):
            w0 = time.perf_counter()
            c = h.covariance(landmarks=lm)
            wall.append(time.perf_counter() - w0)
            dev.append(h.counter("covariance_ns") * 1e-9)
            assert not c["not_positive_definite"]
        out[label] = dict(device_ms_median=1e3 * float(np.median(dev)), device_ms_min=1e3 * float(np.min(dev)),
                          wall_ms_median=1e3 * float(np.median(wall)))
    n = 6 * fp.Pf
    if n <= 12000:
        rp2, ci2, v = h.hsc()
        S = np.zeros((n, n))
        for i in range(fp.Pf):
            for k in range(rp2[i], rp2[i + 1]):
                j = ci2[k]
                S[6 * i:6 * i + 6, 6 * j:6 * j + 6] = v[k]
                S[6 * j:6 * j + 6, 6 * i:6 * i + 6] = v[k].T
        w0 = time.perf_counter()
        np.linalg.inv(S)
        out["numpy_dense_inverse_ms"] = 1e3 * (time.perf_counter() - w0)
    out["script_seconds"] = time.time() - t0
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="+")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = []
    for s in a.shapes:
        r = one(s, a.reps, a.iters)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

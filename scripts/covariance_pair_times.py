"""Times of the covariance pairs (HipSolver.covariance_pairs / cuba_hip_compute_covariance_pairs) on the BASELINE shapes.

    python scripts/covariance_pair_times.py kitti00 g4m [--reps 5] [--iters 3] [--out file.json] [--requests name ...] [--pause s]

Per shape, after `iters` LM iterations, for three requests -- the first pose against every free pose, 100 random pose pairs, 1000 random
landmark-landmark pairs -- the time of one call, median of `reps` repeats after one warm-up call:
  call_ms   the handle's "covariance_pairs_ns" counter: the HOST-side time of the whole call, from after the argument checks to the results
            on the host (symbolic phase, linearisation, factorisation, solves, extraction, download) -- not a device-only time;
  wall_ms   the Python call around it.
Also the chunks it ran in and, as context, covariance() poses-only on the same handle ("covariance_ns", likewise host-side).
--pause s sleeps s seconds after the LM iterations and before every call, so that a kernel trace of the run (rocprofv3 --kernel-trace)
can be cut into calls at the gaps; --requests restricts the run to the named requests."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cuba_amd.capi import HipSolver, sparse_plan  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_named  # noqa: E402

RK_HUBER = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))


def one(name, reps, iters, only=None, pause=0.0):
    t0 = time.time()
    fp = flatten(synth_named(name))
    h = HipSolver(fp, RK_HUBER)
    h.optimize(iters)
    rp, ci = h.hsc_structure()
    plan = sparse_plan(rp, ci)
    out = dict(shape=name, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, levels=plan["nLevels"], tiles=plan["nTiles"], tile_columns=plan["T"])
    rng = np.random.default_rng(0)
    requests = {
        "first_pose_vs_all": [("pose", 0, "pose", j) for j in range(fp.Pf)],
        "random_pose_pairs_100": [("pose", int(a), "pose", int(b)) for a, b in rng.integers(0, fp.Pf, size=(100, 2))],
        "random_landmark_pairs_1000": [("landmark", int(a), "landmark", int(b)) for a, b in rng.integers(0, fp.Lf, size=(1000, 2))],
    }
    for label, pairs in requests.items():
        if only and label not in only:
            continue
        time.sleep(pause)
        h.covariance_pairs(pairs)                               # warm-up: plan, allocations
        call, wall = [], []
        for _ in range(reps):
            time.sleep(pause)
            w0 = time.perf_counter()
            _, bad = h.covariance_pairs(pairs)
            wall.append(time.perf_counter() - w0)
            call.append(h.counter("covariance_pairs_ns") * 1e-9)
            assert not bad
        out[label] = dict(call_ms_median=1e3 * float(np.median(call)), call_ms_min=1e3 * float(np.min(call)),
                          wall_ms_median=1e3 * float(np.median(wall)), chunks=h.counter("covariance_pairs_chunks"))
    if not only:
        h.covariance(landmarks=False)
        ref = []
        for _ in range(reps):
            h.covariance(landmarks=False)
            ref.append(h.counter("covariance_ns") * 1e-9)
        out["covariance_poses_only_call_ms_median"] = 1e3 * float(np.median(ref))
    out["script_seconds"] = time.time() - t0
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="+")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--requests", nargs="*")
    ap.add_argument("--pause", type=float, default=0.0)
    a = ap.parse_args()
    res = []
    for s in a.shapes:
        r = one(s, a.reps, a.iters, a.requests, a.pause)
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

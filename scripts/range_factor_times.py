"""What range factors on the poses (HipSolver.set_range_factors / cuba_hip_set_range_factors) add to an LM run.

    python scripts/range_factor_times.py [--shape kitti00] [--iters 10] [--reps 10] [--out file.json]

Three variants of one shape, each on a handle of its own: no factors, a factor on every free pose, a factor on every tenth (four anchors
at the corners of a tetrahedron about the trajectory, taken in turn; ranges 5 cm off the antenna's distance at the start, lever arm
0.1 -0.2 0.5 m, information of a decimetre-level range, Cauchy kernel).  Per repeat the variants run in turn (every run starts from the
same estimate, restored with set_state) and the wall time of optimize(iters) is taken; the script reports medians and minima per variant
and the ratio of each factor variant's median to the no-factor median."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_named  # noqa: E402

RK_HUBER = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))
ARM = np.array([0.1, -0.2, 0.5])
CORNERS = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])


def rotations(q):
    """[n, 3, 3] rotation matrices of (x, y, z, w) unit quaternions"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def factors_on(fp, poses, seed=0):
    rng = np.random.default_rng(seed)
    poses = np.asarray(poses, dtype=np.int32)
    q, t = np.asarray(fp.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp.t, dtype=np.float64).reshape(-1, 3)
    antennas = np.einsum("nji,nj->ni", rotations(q), ARM - t)          # R^T (a - t) of every pose
    reach = np.abs(antennas - antennas.mean(axis=0)).max()
    anchors = (antennas.mean(axis=0) + reach * CORNERS)[np.arange(len(poses)) % 4]
    ranges = np.abs(np.linalg.norm(antennas[poses] - anchors, axis=1) + 0.05 * rng.normal(size=len(poses)))
    return poses, anchors, ranges, np.full(len(poses), 1e2), np.tile(ARM, (len(poses), 1)), np.full(len(poses), 3, dtype=np.int32), np.full(len(poses), 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = flatten(synth_named(a.shape))
    free = np.arange(fp.Pf)
    variants = {"no_factors": None, "every_pose": factors_on(fp, free), "every_tenth_pose": factors_on(fp, free[::10])}
    handles = {}
    for name, fac in variants.items():
        h = HipSolver(fp, RK_HUBER)
        if fac is not None:
            h.set_range_factors(*fac)
        handles[name] = h
    start = handles["no_factors"].state()
    times = {name: [] for name in variants}
    chi2 = {}
    for rep in range(a.reps + 1):                 # (repeat 0 is the warm-up: structure, allocations, coarse inverse memory)
        for name, h in handles.items():
            h.set_state(*start)
            t0 = time.perf_counter()
            c = h.optimize(a.iters)["chi2"]
            dt = time.perf_counter() - t0
            if rep > 0:
                times[name].append(dt)
            chi2[name] = float(c[-1])
    base = float(np.median(times["no_factors"]))
    out = dict(shape=a.shape, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, iterations=a.iters, reps=a.reps)
    for name in variants:
        med = float(np.median(times[name]))
        out[name] = dict(ms_median=1e3 * med, ms_min=1e3 * float(np.min(times[name])), ratio_to_no_factors=med / base,
                         final_chi2=chi2[name], factors=0 if variants[name] is None else len(variants[name][0]))
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)
    for h in handles.values():
        h.close()


if __name__ == "__main__":
    main()

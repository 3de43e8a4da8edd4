"""What range factors between two poses (HipSolver.set_pose_range_factors / cuba_hip_set_pose_range_factors) add to an LM run, next to
relative-pose edges on the same pairs.

    python scripts/pose_range_factor_times.py [--shape kitti00] [--iters 10] [--reps 10] [--out file.json]

Five variants of one shape, each on a handle of its own, three handles alive at a time: no factors; a range factor on every
consecutive pair of free poses and on every tenth (an odometer: the distance of the wheel points, lever arm 0 / 0.3 / -0.2 m, 2 cm off the distance at the start, information of a
2 cm distance, no kernel); a relative-pose edge on the same pairs (the relative pose at the start, information of a degree and of
2 cm).  Per repeat the variants run in turn (every run starts from the same estimate, restored with set_state) and the wall time of
optimize(iters) is taken; the script reports medians and minima per variant and the ratio of each variant's median to the no-factor
median.  The block pattern is the same in every variant only where the consecutive poses share landmarks."""
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
ARM = np.array([0.0, 0.3, -0.2])
SIGMA = 0.02


def rotations(q):
    """[n, 3, 3] rotation matrices of (x, y, z, w) unit quaternions"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions, row by row"""
    av, aw, bv, bw = a[:, :3], a[:, 3:], b[:, :3], b[:, 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(axis=1, keepdims=True)], axis=1)


def ranges_on(fp, pi, seed=0):
    rng = np.random.default_rng(seed)
    pi = np.asarray(pi, dtype=np.int32)
    pj = pi + 1
    q, t = np.asarray(fp.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp.t, dtype=np.float64).reshape(-1, 3)
    wheels = np.einsum("nji,nj->ni", rotations(q), ARM - t)          # R^T (a - t) of every pose
    d = np.abs(np.linalg.norm(wheels[pi] - wheels[pj], axis=1) + SIGMA * rng.normal(size=len(pi)))
    arms = np.tile(ARM, (len(pi), 1))
    return pi, pj, d, np.full(len(pi), 1 / SIGMA ** 2), arms, arms


def edges_on(fp, pi):
    """Z = T_j T_i^-1 at the start: q_z = q_j q_i^-1, t_z = t_j - R_z t_i"""
    pi = np.asarray(pi, dtype=np.int32)
    pj = pi + 1
    q, t = np.asarray(fp.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp.t, dtype=np.float64).reshape(-1, 3)
    qz = quat_mul(q[pj], q[pi] * np.array([-1.0, -1.0, -1.0, 1.0]))
    qz /= np.linalg.norm(qz, axis=1, keepdims=True)
    tz = t[pj] - np.einsum("nij,nj->ni", rotations(qz), t[pi])
    info = np.tile(np.diag([3.3e3] * 3 + [1 / SIGMA ** 2] * 3), (len(pi), 1, 1))
    return pi, pj, qz, tz, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = flatten(synth_named(a.shape))
    first = np.arange(fp.Pf - 1)
    variants = {"no_factors": None, "range_every_pair": ("range", ranges_on(fp, first)), "range_every_tenth_pair": ("range", ranges_on(fp, first[::10])),
                "relative_every_pair": ("relative", edges_on(fp, first)), "relative_every_tenth_pair": ("relative", edges_on(fp, first[::10]))}
    times = {name: [] for name in variants}
    chi2, blocks = {}, {}
    # two groups of three handles, one after the other (more live handles than hardware queues slow each other down): the no-factor
    # variant runs in both and reports the first group's times
    for group in (("no_factors", "range_every_pair", "range_every_tenth_pair"), ("no_factors", "relative_every_pair", "relative_every_tenth_pair")):
        handles = {}
        for name in group:
            h = HipSolver(fp, RK_HUBER)
            if variants[name] is not None and variants[name][0] == "range":
                h.set_pose_range_factors(*variants[name][1])
            elif variants[name] is not None:
                h.set_relative_pose_edges(*variants[name][1])
            handles[name] = h
        start = handles["no_factors"].state()
        second = "no_factors_again" if times["no_factors"] else None
        for rep in range(a.reps + 1):                 # (repeat 0 is the warm-up: structure, allocations, coarse inverse memory)
            for name, h in handles.items():
                h.set_state(*start)
                t0 = time.perf_counter()
                c = h.optimize(a.iters)["chi2"]
                dt = time.perf_counter() - t0
                key = second if (second and name == "no_factors") else name
                if rep > 0:
                    times.setdefault(key, []).append(dt)
                chi2[key] = float(c[-1])
                blocks[key] = int(h.counters()["hsc_blocks"])
        for h in handles.values():
            h.close()
    variants["no_factors_again"] = None
    base = float(np.median(times["no_factors"]))
    out = dict(shape=a.shape, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, iterations=a.iters, reps=a.reps)
    for name in variants:
        med = float(np.median(times[name]))
        out[name] = dict(ms_median=1e3 * med, ms_min=1e3 * float(np.min(times[name])), ratio_to_no_factors=med / base,
                         final_chi2=chi2[name], hsc_blocks=blocks[name], factors=0 if variants[name] is None else len(variants[name][1][0]))
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

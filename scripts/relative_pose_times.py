"""What SE(3) relative-pose edges (HipSolver.set_relative_pose_edges / cuba_hip_set_relative_pose_edges) add to an LM run.

    python scripts/relative_pose_times.py [--shape kitti00] [--iters 10] [--reps 10] [--closures 20] [--out file.json]

Four variants of one shape, each on a handle of its own: (a) no relative-pose edges, (b) odometry edges on every consecutive pose pair,
(c) (b) plus `closures` long-range loop closures between poses that share no landmark, (d) (c) with robust kernels
(set_pose_factor_robust_kernels): Huber on every odometry edge, Cauchy on the closures, delta^2 = 12.592.  The measurements are the
relative poses of the start, a few centimetres / tenths of a degree off.  Per repeat the variants run in turn (every run starts from the same estimate, restored
with set_state) and the wall time of optimize(iters) is taken; the script reports medians, minima and the spread per variant, the ratio of
each variant's median to (a)'s, and -- to tell the cost of the launches from that of the graph -- the PCG iterations and the blocks of the
reduced matrix of each variant.  (d) is timed in a second round against (c) alone, after (b)'s handle is closed -- at most three handles
(streams) are alive at a time, as in the first round: a fourth one slows every variant down -- and reported with its ratio to (c) of
that round."""
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


def quat_mul(a, b):
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    v = aw * bv + bw * av + np.cross(av, bv)
    return np.array([v[0], v[1], v[2], aw * bw - av @ bv])


def quat_rot(q, v):
    a = 2 * np.cross(q[:3], v)
    return v + q[3] * a + np.cross(q[:3], a)


def edges_on(fp, pairs, seed=0):
    """measurement T_j T_i^-1 of the start, shifted by a few centimetres"""
    rng = np.random.default_rng(seed)
    q, t = np.asarray(fp.q).reshape(-1, 4), np.asarray(fp.t).reshape(-1, 3)
    qz, tz = [], []
    for i, j in pairs:
        qi = q[i] * np.array([-1, -1, -1, 1.0])
        qm = quat_mul(q[j], qi)
        qz.append(qm / np.linalg.norm(qm))
        tz.append(t[j] - quat_rot(qz[-1], t[i]) + 0.03 * rng.normal(size=3))
    info = np.tile(np.diag([1e4] * 3 + [1e2] * 3), (len(pairs), 1, 1))
    return (np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32), np.array(qz), np.array(tz), info)


def run_rounds(a, handles, start, times, info):
    """reps + 1 rounds over the handles in turn, every run from `start`; round 0 is the warm-up (structure, allocations, coarse inverse
    memory)"""
    for rep in range(a.reps + 1):
        for name, h in handles.items():
            h.set_state(*start)
            before = h.counters()["pcg_iterations"]
            t0 = time.perf_counter()
            c = h.optimize(a.iters)["chi2"]
            dt = time.perf_counter() - t0
            if rep > 0:
                times[name].append(dt)
            cnt = h.counters()
            info[name] = dict(final_chi2=float(c[-1]), pcg_iterations=cnt["pcg_iterations"] - before, hsc_blocks=cnt["hsc_blocks"],
                              exact_solves=h.counter("exact_solve_fallbacks"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--closures", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    g = synth_named(a.shape)
    fp = flatten(g)
    row_to_solver = np.full(g.nposes, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(fp.Pt)
    odometry = [(int(row_to_solver[r]), int(row_to_solver[r + 1])) for r in range(g.nposes - 1) if row_to_solver[r] >= 0 and row_to_solver[r + 1] >= 0]
    plain = HipSolver(fp, RK_HUBER)
    rp, ci = plain.hsc_structure()
    have = {(r, int(c)) for r in range(fp.Pf) for c in ci[rp[r]:rp[r + 1]]}
    rng = np.random.default_rng(1)
    closures = []
    while len(closures) < a.closures:
        x, y = sorted(int(v) for v in rng.integers(0, fp.Pf, 2))
        if y - x > max(24, fp.Pf // 8) and (x, y) not in have and (x, y) not in closures:
            closures.append((x, y))
    variants = {"none": None, "odometry": edges_on(fp, odometry), "odometry_and_closures": edges_on(fp, odometry + closures)}
    handles = {"none": plain}
    for name, rel in variants.items():
        if rel is not None:
            handles[name] = HipSolver(fp, RK_HUBER)
            handles[name].set_relative_pose_edges(*rel)
    start = plain.state()
    times = {name: [] for name in variants}
    info = {}
    run_rounds(a, handles, start, times, info)
    # second round: (d) against (c)
    handles.pop("odometry").close()
    variants["robust"] = variants["odometry_and_closures"]
    robust = HipSolver(fp, RK_HUBER)
    robust.set_relative_pose_edges(*variants["robust"])
    robust.set_pose_factor_robust_kernels(1, [1] * len(odometry) + [3] * len(closures), float(np.sqrt(12.592)))
    second = {"odometry_and_closures": handles["odometry_and_closures"], "robust": robust}
    times2 = {name: [] for name in second}
    run_rounds(a, second, start, times2, info)
    times["robust"] = times2["robust"]
    handles["robust"] = robust
    base = float(np.median(times["none"]))
    out = dict(shape=a.shape, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, iterations=a.iters, reps=a.reps)
    for name in variants:
        ts = 1e3 * np.array(times[name])
        out[name] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()), ratio_to_none=float(np.median(ts)) / (1e3 * base),
                         relative_pose_edges=0 if variants[name] is None else len(variants[name][0]), **info[name])
    out["robust"]["ratio_to_odometry_and_closures"] = float(np.median(times2["robust"]) / np.median(times2["odometry_and_closures"]))
    out["robust"]["odometry_and_closures_ms_median_same_round"] = 1e3 * float(np.median(times2["odometry_and_closures"]))
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)
    for h in handles.values():
        h.close()


if __name__ == "__main__":
    main()

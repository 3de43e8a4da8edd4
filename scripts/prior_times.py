"""What SE(3) pose priors (HipSolver.set_pose_priors / cuba_hip_set_pose_priors) add to an LM run.

    python scripts/prior_times.py [--shape kitti00] [--iters 10] [--reps 10] [--out file.json]

Three variants of one shape, each on a handle of its own: no priors, a prior on every free pose, a prior on every tenth free pose (priors
a few centimetres / tenths of a degree off the start, information of a GPS / INS reading).  Per repeat the variants run in turn (every
run starts from the same estimate, restored with set_state) and the wall time of optimize(iters) is taken; the script reports medians
and minima per variant and the ratio of each prior variant's median to the no-prior median."""
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


def priors_on(fp, poses, seed=0):
    rng = np.random.default_rng(seed)
    q = np.asarray(fp.q).reshape(-1, 4)[poses].copy()
    t = np.asarray(fp.t).reshape(-1, 3)[poses] + 0.05 * rng.normal(size=(len(poses), 3))
    info = np.tile(np.diag([1e4] * 3 + [1e2] * 3), (len(poses), 1, 1))
    return np.asarray(poses, dtype=np.int32), q, t, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = flatten(synth_named(a.shape))
    variants = {"no_priors": None, "every_pose": priors_on(fp, np.arange(fp.Pf)), "every_tenth_pose": priors_on(fp, np.arange(0, fp.Pf, 10))}
    handles = {}
    for name, pri in variants.items():
        h = HipSolver(fp, RK_HUBER)
        if pri is not None:
            h.set_pose_priors(*pri)
        handles[name] = h
    start = handles["no_priors"].state()
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
    base = float(np.median(times["no_priors"]))
    out = dict(shape=a.shape, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, iterations=a.iters, reps=a.reps)
    for name in variants:
        med = float(np.median(times[name]))
        out[name] = dict(ms_median=1e3 * med, ms_min=1e3 * float(np.min(times[name])), ratio_to_no_priors=med / base,
                         final_chi2=chi2[name], priors=0 if variants[name] is None else len(variants[name][0]))
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)
    for h in handles.values():
        h.close()


if __name__ == "__main__":
    main()

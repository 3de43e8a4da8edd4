"""What landmark position priors (HipSolver.set_landmark_priors / cuba_hip_set_landmark_priors) add to an LM run.

    python scripts/landmark_prior_times.py [--shape kitti00] [--iters 10] [--reps 10] [--out file.json]

Three variants of one shape, each on a handle of its own: no priors, a prior on every free (observed) landmark, a prior on every tenth
(priors a few centimetres off the start, information of a decimetre-level survey, Huber kernel).  Per repeat the variants run in turn (every
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


def priors_on(fp, landmarks, seed=0):
    rng = np.random.default_rng(seed)
    xyz = np.asarray(fp.Xw).reshape(-1, 3)[landmarks] + 0.05 * rng.normal(size=(len(landmarks), 3))
    info = np.tile(1e2 * np.eye(3), (len(landmarks), 1, 1))
    return np.asarray(landmarks, dtype=np.int32), xyz, info, np.full(len(landmarks), 1, dtype=np.int32), np.full(len(landmarks), 2.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = flatten(synth_named(a.shape))
    observed = np.nonzero(np.bincount(fp.eL, minlength=fp.Lt)[:fp.Lf] > 0)[0]
    variants = {"no_priors": None, "every_landmark": priors_on(fp, observed), "every_tenth_landmark": priors_on(fp, observed[::10])}
    handles = {}
    for name, pri in variants.items():
        h = HipSolver(fp, RK_HUBER)
        if pri is not None:
            h.set_landmark_priors(*pri)
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

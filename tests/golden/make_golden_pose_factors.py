"""Generates tests/golden/pose_factors_bits.json: the exact bits of what the solver computes with pose priors and relative-pose edges
(the assembled system, the objective, the per-factor chi2, LM trajectories and final states), on the fp64 and the fp32 library.  Doubles
are stored as float.hex() strings, arrays as the sha256 of their bytes plus their length.  tests/test_gpu_pose_factor_bits.py recomputes
every entry through record() below and asserts equality: the fixture pins a change that must leave the results alone (a refactor of the
factor code) to the commit it was recorded at.  Needs the GPU; re-record when the toolchain changes (the fixture names the hipcc it was
built with).  Run from the repo root: `python tests/golden/make_golden_pose_factors.py`."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import RK_HUBER  # noqa: E402
from test_gpu_configs import shuffled_pose_ids  # noqa: E402
from test_gpu_pose_priors import make_priors  # noqa: E402
from test_gpu_relative_pose import make_rel, split_pairs  # noqa: E402

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "pose_factors_bits.json")
PRECISIONS = ("f64", "f32")


def arr(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "len": int(a.size)}


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def factors(fp):
    """priors: two on one pose, one on the fixed pose; edges: the pair list of
    test_gpu_relative_pose.py::test_assembled_system_is_the_plain_one_plus_the_edge_terms"""
    fixed = fp.Pt - 1
    assert fixed >= fp.Pf
    near, far = split_pairs(fp, 2, 2)
    pairs = [near[0], far[0], far[0], (far[1][1], far[1][0]), (near[1][1], near[1][0]), (5, fixed), (fixed, 9)]
    return make_priors(fp, [3, 3, 17, fixed], seed=0), make_rel(fp, pairs, seed=2)


def handle(fp, precision, priors, rel, **opts):
    h = HipSolver(fp, RK_HUBER, precision=precision, **opts)
    if priors is not None:
        h.set_pose_priors(*priors)
    if rel is not None:
        h.set_relative_pose_edges(*rel)
    return h


def lm(fp, precision, priors, rel, **opts):
    return hexes(handle(fp, precision, priors, rel, **opts).optimize(10)["chi2"])


def record_g40(precision):
    fp = flatten(synth_ba(40, 600, 2400, seed=1))
    pri, rel = factors(fp)
    out = {}
    h = handle(fp, precision, pri, rel)
    h.set_lambda(0.0)
    h.schur()
    out["hsc"] = arr(h.hsc()[2])
    out["bp"] = arr(h.array("bp"))
    out["bsc"] = arr(h.array("bsc"))
    out["compute_errors"] = float(h.compute_errors()).hex()
    out["prior_chi_squares"] = hexes(h.prior_chi_squares())
    out["relative_pose_chi_squares"] = hexes(h.relative_pose_chi_squares())
    h = handle(fp, precision, pri, rel)
    out["optimize"] = hexes(h.optimize(10)["chi2"])
    q, t, X = h.state()
    out["q"], out["t"], out["Xw"] = arr(q), arr(t), arr(X)
    out["optimize_host_loop"] = lm(fp, precision, pri, rel, profile=1)
    out["optimize_priors_only"] = lm(fp, precision, pri, None)
    out["optimize_edges_only"] = lm(fp, precision, None, rel)
    return out


def record_shuffled(precision):
    fp = flatten(shuffled_pose_ids(synth_ba(60, 900, 3600, seed=2), seed=1))
    pri, rel = factors(fp)
    return {"optimize": lm(fp, precision, pri, rel)}


def record(precision):
    return {"g40": record_g40(precision), "shuffled60": record_shuffled(precision)}


if __name__ == "__main__":
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_pose_factors.py", "hipcc_version": hipcc, "iterations": 10}
    for precision in PRECISIONS:
        out[precision] = record(precision)
        print(precision, out[precision]["g40"]["optimize"][-1], out[precision]["shuffled60"]["optimize"][-1], flush=True)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1)

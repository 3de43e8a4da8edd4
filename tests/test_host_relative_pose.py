"""The relative-pose edges of the C++ host layer (cuba::addRelativePoseEdge / relativePoseChiSquared) through
host/samples/loop_closure.cpp: on the GPU the sample's objective per iteration, its edges' chi2 and the last pose's covariance are those
of the same flow driven through the C ABI (HipSolver), as tests/test_host_priors.py does for pose_priors.  (That the sample builds
without a GPU is checked in tests/test_relative_pose_reference.py.)"""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import relative_pose_reference as rr
from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "loop_closure")


def _python_flow(path, iters):
    """the sample's flow through the C ABI: every pose free but the first, odometry edges between consecutive poses, a first run, then
    the closure between the first and the last pose and a second run from the first one's estimate"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    g = Graph.from_json(path)
    g.pose_fixed[:] = False
    g.pose_fixed[0] = True
    fp = flatten(g)
    assert fp.Pt == g.nposes
    row_to_solver = np.empty(g.nposes, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(g.nposes)
    q0, t0 = np.asarray(g.pose_q), np.asarray(g.pose_t)
    rows = [(r, r + 1) for r in range(g.nposes - 1)] + [(0, g.nposes - 1)]
    z = [rr.measurement(q0, t0, i, j) for i, j in rows]
    info = [np.diag([1e4] * 3 + [1e2] * 3)] * (g.nposes - 1) + [np.diag([1e5] * 3 + [1e3] * 3)]
    pi, pj = row_to_solver[[r[0] for r in rows]], row_to_solver[[r[1] for r in rows]]
    qz, tz, info = np.array([a[0] for a in z]), np.array([a[1] for a in z]), np.array(info)
    h = HipSolver(fp, RK_HUBER)
    h.set_relative_pose_edges(pi[:-1], pj[:-1], qz[:-1], tz[:-1], info[:-1])
    h.optimize(iters)
    q, t, X = h.state()
    h2 = HipSolver(dataclasses.replace(fp, q=q, t=t, Xw=X), RK_HUBER)
    h2.set_relative_pose_edges(pi, pj, qz, tz, info)
    chi2 = h2.optimize(iters)["chi2"]
    cov = h2.covariance(landmarks=False)["pose"][row_to_solver[g.nposes - 1]]
    ids = np.asarray(g.pose_ids)
    return chi2, h2.relative_pose_chi_squares(), cov, [(int(ids[i]), int(ids[j])) for i, j in rows]


@pytest.mark.gpu
def test_loop_closure_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(80, 3000, 12000, seed=5, loop_closure=False).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got_chi2 = np.array([float(m) for m in re.findall(r"iter:\s*\d+, chi2: ([0-9.eE+-]+)", out.stdout)])
    got_rel = [(int(a), int(b), float(c)) for a, b, c in re.findall(r"relative (\d+) (\d+) chi2 ([0-9.eE+-]+)", out.stdout)]
    lines = out.stdout.split("covariance\n", 1)[1].split()
    got_cov = np.array([float(v) for v in lines[:36]]).reshape(6, 6).T
    assert re.search(r"gate mahalanobis2 [0-9.eE+-]+", out.stdout)
    before = np.array(re.search(r"last pose sigma before (.*)", out.stdout).group(1).split(), dtype=float)
    after = np.array(re.search(r"last pose sigma after (.*)", out.stdout).group(1).split(), dtype=float)
    assert np.all(after < before)          # the closure ties the end of the open trajectory down
    want_chi2, want_rel, want_cov, ids = _python_flow(path, 10)
    assert len(got_chi2) == len(want_chi2)
    assert np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
    assert [(a, b) for a, b, _ in got_rel] == ids
    for (_, _, c), w in zip(got_rel, want_rel):
        assert abs(c - w) <= 1e-8 * max(w, 1e-6)
    assert np.abs(got_cov - want_cov).max() <= 1e-8 * np.abs(want_cov).max()

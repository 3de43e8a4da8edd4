"""The landmark priors of the C++ host layer (cuba::addLandmarkPrior / landmarkPriorChiSquared) through
host/samples/ground_control_points.cpp: the sample builds without a GPU, and on the GPU its objective per iteration, its control points'
chi2, estimates and covariances are those of the same flow driven through the C ABI (HipSolver), as tests/test_host_priors.py does for
the pose priors."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "ground_control_points")


def test_ground_control_points_sample_builds_without_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/ground_control_points"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout


def _python_flow(path, iters, points, kernel, delta):
    """the sample's flow through the C ABI: every vertex free, `points` control points spread over the observed landmarks (file order) at
    their initial positions with information 1e4 I, the second one 5, -3, 4 m off"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    g = Graph.from_json(path)
    g.pose_fixed[:] = False
    g.lm_fixed[:] = False
    fp = flatten(g)
    row_to_solver = np.full(g.nlandmarks, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.lm_src)] = np.arange(len(fp.lm_src))
    seen = np.zeros(int(g.lm_ids.max()) + 1, dtype=bool)
    seen[np.concatenate([g.mono_vl, g.stereo_vl])] = True
    observed = np.nonzero(seen[g.lm_ids])[0]
    rows = observed[[j * len(observed) // points for j in range(points)]]
    xyz = np.asarray(g.lm_X)[rows].copy()
    xyz[1] += [5.0, -3.0, 4.0]
    info = np.tile(1e4 * np.eye(3), (points, 1, 1))
    h = HipSolver(fp, RK_HUBER)
    h.set_landmark_priors(row_to_solver[rows], xyz, info, kernel if kernel else None, delta if kernel else None)
    chi2 = h.optimize(iters)["chi2"]
    e = h.landmark_prior_chi_squares()
    X = h.state()[2][row_to_solver[rows]]
    cov = h.covariance()["landmark"][row_to_solver[rows]]
    return chi2, e, X, cov, np.asarray(g.lm_ids)[rows]


@pytest.mark.gpu
def test_ground_control_points_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=5).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "6", "3", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got_chi2 = np.array([float(m) for m in re.findall(r"iter:\s*\d+, chi2: ([0-9.eE+-]+)", out.stdout)])
    got_e = {int(a): float(b) for a, b in re.findall(r"control point (\d+) chi2 ([0-9.eE+-]+)", out.stdout)}
    got_X = {int(m[0]): np.array([float(v) for v in m[1:]]) for m in re.findall(r"control point (\d+) estimate (\S+) (\S+) (\S+)", out.stdout)}
    got_cov = {int(m[0]): np.array([float(v) for v in m[1].split()]).reshape(3, 3).T
               for m in re.findall(r"control point (\d+) covariance\n((?:\S+ \S+ \S+\n){3})", out.stdout)}
    want_chi2, want_e, want_X, want_cov, ids = _python_flow(path, 10, 6, 3, 3.0)
    assert len(got_chi2) == len(want_chi2)
    assert np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
    assert sorted(got_e) == sorted(int(i) for i in ids) == sorted(got_X) == sorted(got_cov)
    for k, i in enumerate(int(i) for i in ids):
        assert abs(got_e[i] - want_e[k]) <= 1e-8 * max(want_e[k], 1e-6)
        assert np.abs(got_X[i] - want_X[k]).max() <= 1e-9 * np.abs(want_X[k]).max()
        assert np.abs(got_cov[i] - want_cov[k]).max() <= 1e-8 * np.abs(want_cov[k]).max()
    # Cauchy rejects the gross survey: its chi2 stays far above every other control point's
    e = np.array([got_e[int(i)] for i in ids])
    assert e[1] > 100 * np.delete(e, 1).max()

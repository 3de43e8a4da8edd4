"""The position factors of the C++ host layer (cuba::addPositionFactor / positionFactorChiSquared) through
host/samples/gnss_positions.cpp: the sample builds without a GPU, and on the GPU its objective per iteration, its fixes' chi2, the camera
centres and the pose covariances are those of the same flow driven through the C ABI (HipSolver), as tests/test_host_landmark_priors.py
does for the landmark priors."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "gnss_positions")
ARM = np.array([0.1, -0.2, 0.5])


def test_gnss_positions_sample_builds_without_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/gnss_positions"])
    assert os.access(SAMPLE, os.X_OK)          # (what it prints without arguments: tests/test_position_factor_reference.py)


def _python_flow(path, iters, stride, kernel, delta):
    """the sample's flow through the C ABI: every vertex free, a fix on every stride-th pose with an edge (file order) at the antenna's
    initial position with information 1e4 I, the second one 5, -3, 4 m off"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    from oracle import oracle
    g = Graph.from_json(path)
    g.pose_fixed[:] = False
    g.lm_fixed[:] = False
    fp = flatten(g)
    row_to_solver = np.full(g.nposes, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(len(fp.pose_src))
    seen = np.zeros(int(g.pose_ids.max()) + 1, dtype=bool)
    seen[np.concatenate([g.mono_vp, g.stereo_vp])] = True
    observed = np.nonzero(seen[g.pose_ids])[0]
    rows = observed[::stride]
    n = len(rows)
    q0, t0 = np.asarray(g.pose_q, dtype=np.float64)[rows], np.asarray(g.pose_t, dtype=np.float64)[rows]
    z = np.array([oracle.quat_to_rot(q0[k]).T @ (ARM - t0[k]) for k in range(n)])
    z[1] += [5.0, -3.0, 4.0]
    info = np.tile(1e4 * np.eye(3), (n, 1, 1))
    poses = row_to_solver[rows]
    h = HipSolver(fp, RK_HUBER)
    h.set_position_factors(poses, z, info, np.tile(ARM, (n, 1)), kernel if kernel else None, delta if kernel else None)
    chi2 = h.optimize(iters)["chi2"]
    e = h.position_factor_chi_squares()
    q, t, _ = h.state()
    centres = np.array([-oracle.quat_to_rot(q[p]).T @ t[p] for p in poses])
    cov = h.covariance(landmarks=False)["pose"][poses]
    return chi2, e, centres, cov, np.asarray(g.pose_ids)[rows]


@pytest.mark.gpu
def test_gnss_positions_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=5).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "5", "3", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got_chi2 = np.array([float(m) for m in re.findall(r"iter:\s*\d+, chi2: ([0-9.eE+-]+)", out.stdout)])
    got_e = {int(a): float(b) for a, b in re.findall(r"fix (\d+) chi2 ([0-9.eE+-]+)", out.stdout)}
    got_X = {int(m[0]): np.array([float(v) for v in m[1:]]) for m in re.findall(r"fix (\d+) position (\S+) (\S+) (\S+)", out.stdout)}
    got_cov = {int(m[0]): np.array([float(v) for v in m[1].split()]).reshape(6, 6).T
               for m in re.findall(r"fix (\d+) covariance\n((?:\S+ \S+ \S+ \S+ \S+ \S+\n){6})", out.stdout)}
    want_chi2, want_e, want_X, want_cov, ids = _python_flow(path, 10, 5, 3, 3.0)
    assert len(ids) == 8
    assert len(got_chi2) == len(want_chi2)
    assert np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
    assert sorted(got_e) == sorted(int(i) for i in ids) == sorted(got_X) == sorted(got_cov)
    for k, i in enumerate(int(i) for i in ids):
        assert abs(got_e[i] - want_e[k]) <= 1e-8 * max(want_e[k], 1e-6)
        assert np.abs(got_X[i] - want_X[k]).max() <= 1e-9 * np.abs(want_X[k]).max()
        assert np.abs(got_cov[i] - want_cov[k]).max() <= 1e-8 * np.abs(want_cov[k]).max()
    # Cauchy rejects the gross fix: its chi2 stays far above every other fix's
    e = np.array([got_e[int(i)] for i in ids])
    assert e[1] > 100 * np.delete(e, 1).max()

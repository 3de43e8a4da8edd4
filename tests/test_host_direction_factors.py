"""The direction factors of the C++ host layer (cuba::addDirectionFactor / directionFactorChiSquared) through
host/samples/gravity_aligned.cpp: the sample builds without a GPU, and on the GPU its objective per iteration, its readings' chi2, the
tilt errors and the pose covariances are those of the same flow driven through the C ABI (HipSolver), as
tests/test_host_position_factors.py does for the position factors."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "gravity_aligned")
DOWN = np.array([0.0, 0.0, -1.0])
SIGMA = 0.01


def test_gravity_aligned_sample_builds_without_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/gravity_aligned"])
    assert os.access(SAMPLE, os.X_OK)          # (what it prints without arguments: tests/test_direction_factor_reference.py)


def _angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b))


def _python_flow(path, iters, stride, kernel, delta):
    """the sample's flow through the C ABI: every vertex free, fixes with information 1e4 I on the camera centres of the first and the
    last pose with an edge (file order), a gravity reading m = R d, d = (0, 0, -1), with information (I - m m^T) / 0.01^2 on every
    stride-th such pose, the second one normalised(m + (0.5, -0.3, 0.4))"""
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
    q0, t0 = np.asarray(g.pose_q, dtype=np.float64), np.asarray(g.pose_t, dtype=np.float64)
    ends = observed[[0, -1]]
    z = np.array([-oracle.quat_to_rot(q0[r]).T @ t0[r] for r in ends])
    rows = observed[::stride]
    n = len(rows)
    clean = np.array([oracle.quat_to_rot(q0[r]) @ DOWN for r in rows])
    m = clean.copy()
    m[1] = m[1] + [0.5, -0.3, 0.4]
    m[1] /= np.linalg.norm(m[1])
    info = np.array([(np.eye(3) - np.outer(x, x)) / SIGMA ** 2 for x in m])
    poses = row_to_solver[rows]
    h = HipSolver(fp, RK_HUBER)
    h.set_position_factors(row_to_solver[ends], z, np.tile(1e4 * np.eye(3), (2, 1, 1)))
    h.set_direction_factors(poses, np.tile(DOWN, (n, 1)), m, info, kernel if kernel else None, delta if kernel else None)
    chi2 = h.optimize(iters)["chi2"]
    e = h.direction_factor_chi_squares()
    q = h.state()[0]
    tilt = np.array([_angle(oracle.quat_to_rot(q[p]) @ DOWN, clean[k]) for k, p in enumerate(poses)])
    cov = h.covariance(landmarks=False)
    assert not cov["not_positive_definite"]
    return chi2, e, tilt, cov["pose"][poses], np.asarray(g.pose_ids)[rows]


@pytest.mark.gpu
def test_gravity_aligned_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=5).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "5", "3", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got_chi2 = np.array([float(m) for m in re.findall(r"iter:\s*\d+, chi2: ([0-9.eE+-]+)", out.stdout)])
    got_e = {int(a): float(b) for a, b in re.findall(r"gravity (\d+) chi2 ([0-9.eE+-]+)", out.stdout)}
    got_tilt = {int(a): float(b) for a, b in re.findall(r"gravity (\d+) tilt ([0-9.eE+-]+)", out.stdout)}
    got_cov = {int(m[0]): np.array([float(v) for v in m[1].split()]).reshape(6, 6).T
               for m in re.findall(r"gravity (\d+) covariance\n((?:\S+ \S+ \S+ \S+ \S+ \S+\n){6})", out.stdout)}
    want_chi2, want_e, want_tilt, want_cov, ids = _python_flow(path, 10, 5, 3, 3.0)
    assert len(ids) == 8
    assert len(got_chi2) == len(want_chi2)
    assert np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
    assert sorted(got_e) == sorted(int(i) for i in ids) == sorted(got_tilt) == sorted(got_cov)
    for k, i in enumerate(int(i) for i in ids):
        assert abs(got_e[i] - want_e[k]) <= 1e-8 * max(want_e[k], 1e-6)
        # (an angle of ~1e-3 from atan2 of 17-digit quaternions: absolute, 1e-9 of the unit vectors it is taken between)
        assert abs(got_tilt[i] - want_tilt[k]) <= 1e-9
        assert np.abs(got_cov[i] - want_cov[k]).max() <= 1e-8 * np.abs(want_cov[k]).max()
    # Cauchy rejects the gross reading: its chi2 stays far above every other reading's
    e = np.array([got_e[int(i)] for i in ids])
    assert e[1] > 100 * np.delete(e, 1).max()

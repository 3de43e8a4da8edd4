"""The pose priors of the C++ host layer (cuba::addPosePrior / priorChiSquared) through host/samples/pose_priors.cpp: the sample
builds without a GPU, and on the GPU its objective per iteration, its priors' chi2 and the last pose's covariance are those of the same
flow driven through the C ABI (HipSolver), as tests/test_host_cpp.py does for local_ba_flow."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "pose_priors")


def test_pose_priors_sample_builds_without_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/pose_priors"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout


def _python_flow(path, iters, every):
    """the sample's flow through the C ABI: every pose free, a strong prior on the first pose, loose ones on every k-th"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    g = Graph.from_json(path)
    g.pose_fixed[:] = False
    fp = flatten(g)
    row_to_solver = np.empty(len(fp.pose_src), dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(len(fp.pose_src))
    rows = np.arange(0, g.nposes, every)
    info = [np.diag([1e8] * 6) if r == 0 else np.diag([1e2] * 3 + [1.0] * 3) for r in rows]
    h = HipSolver(fp, RK_HUBER)
    h.set_pose_priors(row_to_solver[rows], np.asarray(g.pose_q)[rows], np.asarray(g.pose_t)[rows], np.array(info))
    chi2 = h.optimize(iters)["chi2"]
    prior_chi = h.prior_chi_squares()
    cov = h.covariance(landmarks=False)["pose"][row_to_solver[g.nposes - 1]]
    return chi2, prior_chi, cov, np.asarray(g.pose_ids)[rows]


@pytest.mark.gpu
def test_pose_priors_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(80, 3000, 12000, seed=5).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "5", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got_chi2 = np.array([float(m) for m in re.findall(r"iter:\s*\d+, chi2: ([0-9.eE+-]+)", out.stdout)])
    got_prior = {int(a): float(b) for a, b in re.findall(r"prior (\d+) chi2 ([0-9.eE+-]+)", out.stdout)}
    lines = out.stdout.split("covariance\n", 1)[1].split()
    got_cov = np.array([float(v) for v in lines[:36]]).reshape(6, 6).T
    want_chi2, want_prior, want_cov, ids = _python_flow(path, 10, 5)
    assert len(got_chi2) == len(want_chi2)
    assert np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
    assert sorted(got_prior) == sorted(int(i) for i in ids)
    for i, w in zip(ids, want_prior):
        assert abs(got_prior[int(i)] - w) <= 1e-8 * max(w, 1e-6)
    assert np.abs(got_cov - want_cov).max() <= 1e-8 * np.abs(want_cov).max()

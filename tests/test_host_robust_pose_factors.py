"""The robust kernels of the C++ host layer (cuba::PoseFactorKernel on cuba::RelativePoseEdge) through host/samples/robust_loop_closure.cpp:
on the GPU the sample's objective per iteration, its edges' chi2 and the distances of its results from the run without the false closure
are those of the same flow driven through the C ABI (HipSolver), as tests/test_host_relative_pose.py does for loop_closure.  (That the
sample builds without a GPU is checked in tests/test_robust_pose_factor_reference.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import relative_pose_reference as rr
from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "robust_loop_closure")
CAUCHY = 3


def _python_flow(path, iters):
    """the sample's three runs through the C ABI, each from the initial estimate: every pose free but the first, odometry between
    consecutive poses, the closure first -> last, then the false closure, then Cauchy on both closures"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    g = Graph.from_json(path)
    g.pose_fixed[:] = False
    g.pose_fixed[0] = True
    fp = flatten(g)
    P = g.nposes
    assert fp.Pt == P
    row_to_solver = np.empty(P, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(P)
    q0, t0 = np.asarray(g.pose_q), np.asarray(g.pose_t)
    rows = [(r, r + 1) for r in range(P - 1)] + [(0, P - 1), (P // 4, 3 * P // 4)]
    z = [rr.measurement(q0, t0, i, j) for i, j in rows]
    z[-1] = rr.pose_mul((np.array([0.0, np.sin(0.1), 0.0, np.cos(0.1)]), np.array([0.5, 0.0, 1.0])), z[-1])
    info = [np.diag([1e4] * 3 + [1e2] * 3)] * (P - 1) + [np.diag([1e5] * 3 + [1e3] * 3)] * 2
    pi, pj = row_to_solver[[r[0] for r in rows]], row_to_solver[[r[1] for r in rows]]
    qz, tz, info = np.array([a[0] for a in z]), np.array([a[1] for a in z]), np.array(info)
    ids = np.asarray(g.pose_ids)
    runs, reference = {}, None
    for name, n, kernel in (("reference", P, False), ("plain", P + 1, False), ("cauchy", P + 1, True)):
        h = HipSolver(fp, RK_HUBER)
        h.set_relative_pose_edges(pi[:n], pj[:n], qz[:n], tz[:n], info[:n])
        if kernel:
            h.set_pose_factor_robust_kernels(1, [0] * (P - 1) + [CAUCHY] * 2, [0.0] * (P - 1) + [float(np.sqrt(12.592))] * 2)
        chi2 = h.optimize(iters)["chi2"]
        t = h.state()[1]
        reference = t if reference is None else reference
        runs[name] = (chi2, h.relative_pose_chi_squares(), float(np.abs(t - reference).max()), [(int(ids[i]), int(ids[j])) for i, j in rows[:n]])
    return runs


@pytest.mark.gpu
def test_robust_loop_closure_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(60, 1500, 6000, seed=5, loop_closure=False).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    sections = {s.split("\n", 1)[0].strip(): s for s in out.stdout.split("run ")[1:]}
    assert sorted(sections) == ["cauchy", "plain", "reference"]
    want = _python_flow(path, 10)
    dist = {}
    for name, text in sections.items():
        got_chi2 = np.array([float(m) for m in re.findall(r"iter:\s*\d+, chi2: ([0-9.eE+-]+)", text)])
        got_rel = [(int(a), int(b), float(c)) for a, b, c in re.findall(r"relative (\d+) (\d+) chi2 ([0-9.eE+-]+)", text)]
        want_chi2, want_rel, want_dist, ids = want[name]
        assert len(got_chi2) == len(want_chi2)
        assert np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
        assert [(a, b) for a, b, _ in got_rel] == ids
        for (_, _, c), w in zip(got_rel, want_rel):
            assert abs(c - w) <= 1e-8 * max(w, 1e-6)
        if name != "reference":
            dist[name] = float(re.search(r"distance %s ([0-9.eE+-]+)" % name, text).group(1))
            assert abs(dist[name] - want_dist) <= 1e-8 * max(want_dist, 1e-6)
    print("distance from the run without the false closure: no kernel %.4g m, Cauchy %.4g m" % (dist["plain"], dist["cauchy"]))
    assert dist["cauchy"] < 0.1 * dist["plain"]          # what the kernel is for

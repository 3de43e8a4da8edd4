"""The range factors between two poses of the C++ host layer (cuba::addPoseRangeFactor / removePoseRangeFactor /
poseRangeFactorChiSquared) through host/samples/odometer_scale.cpp: the sample builds without a GPU, and on the GPU its objective per
iteration, the recovered scale, its factors' chi2 and the gated outlier -- in the first run, in the run after the gated factor was removed
(removePoseRangeFactor) and in the run after the last keyframe was removed (removePoseVertex, which drops the factors touching the pose: a
factor left behind on a vertex that is no longer part of the graph would make initialize() throw) -- are those of the same flow driven
through the C ABI (HipSolver), as tests/test_host_range_factors.py does for the range factors.  That addPoseRangeFactor refuses a factor
without two different vertices is part of host/host_selftest.cpp (tests/test_host_cpp.py)."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER
from test_pose_range_factor_reference import monocular

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "odometer_scale")
ARM = np.array([0.0, 0.3, -0.2])
SIGMA = 0.02


def test_odometer_scale_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/odometer_scale"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout


def spread(c):
    return float(np.sqrt(((c - c.mean(axis=0)) ** 2).sum()))


def _python_flow(path, iters, kernel, delta, scale0, gate):
    """the sample's flow through the C ABI: monocular edges only, the first pose with an edge fixed and every other vertex free, an
    odometer factor (information 1 / 0.02^2, arms 0 / 0.3 / -0.2) on every consecutive pair of poses with edges, a peer range from the
    middle pose to the second, 5 m long, under the kernel; the start blown up by scale0 about the fixed pose's camera centre; then the run
    without the factors whose chi2 exceeds the gate; then, from there, the graph without the last pose, its edges and its factors"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten, write_back
    from oracle import oracle
    g = monocular(Graph.from_json(path))
    q0, t0 = np.asarray(g.pose_q, dtype=np.float64), np.asarray(g.pose_t, dtype=np.float64)
    seen = np.zeros(int(g.pose_ids.max()) + 1, dtype=bool)
    seen[g.mono_vp] = True
    observed = np.nonzero(seen[g.pose_ids])[0]
    fixed = np.zeros_like(g.pose_fixed)
    fixed[observed[0]] = True
    g = dataclasses.replace(g, pose_fixed=fixed, lm_fixed=np.zeros_like(g.lm_fixed))
    R = [oracle.quat_to_rot(q0[r]) for r in range(g.nposes)]
    world = lambda r, a: R[r].T @ (a - t0[r])  # noqa: E731
    file_centres = np.array([world(r, np.zeros(3)) for r in observed])
    rows_i = np.concatenate([observed[:-1], [observed[len(observed) // 2]]])
    rows_j = np.concatenate([observed[1:], [observed[1]]])
    n = len(rows_i)
    rng = np.array([np.linalg.norm(world(i, ARM) - world(j, ARM)) for i, j in zip(rows_i, rows_j)])
    rng[-1] += 5.0
    kinds = np.zeros(n, dtype=np.int32)
    kinds[-1] = kernel
    deltas = np.where(kinds != 0, delta, 0.0) if kernel else None
    c0 = file_centres[0]
    centres = np.array([world(r, np.zeros(3)) for r in range(g.nposes)])
    t1 = np.array([t0[r] if r == observed[0] else -R[r] @ (c0 + scale0 * (centres[r] - c0)) for r in range(g.nposes)])
    g = dataclasses.replace(g, pose_t=t1, lm_X=c0 + scale0 * (np.asarray(g.lm_X, dtype=np.float64) - c0))
    fp = flatten(g)
    row_to_solver = np.full(g.nposes, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(len(fp.pose_src))
    ids_i, ids_j = np.asarray(g.pose_ids)[rows_i], np.asarray(g.pose_ids)[rows_j]

    def scale_of(h):
        q, t, _ = h.state()
        c = np.array([-oracle.quat_to_rot(q[p]).T @ t[p] for p in row_to_solver[observed]])
        return spread(c) / spread(file_centres)

    def set_factors(h, k, to_solver, ri, rj):
        robust = kernel and kinds[k].any()
        h.set_pose_range_factors(to_solver[ri], to_solver[rj], rng[k], np.full(len(k), 1 / SIGMA ** 2), np.tile(ARM, (len(k), 1)),
                                 np.tile(ARM, (len(k), 1)), kinds[k] if robust else None, deltas[k] if robust else None)

    h = HipSolver(fp, RK_HUBER)
    keep = np.ones(n, dtype=bool)
    out = []
    for _ in range(2):
        k = np.nonzero(keep)[0]
        set_factors(h, k, row_to_solver, rows_i[k], rows_j[k])
        chi2 = h.optimize(iters)["chi2"]
        e = np.zeros(n)
        e[k] = h.pose_range_factor_chi_squares()
        out.append((chi2, scale_of(h), e))
        keep = keep & (e <= gate)
    # the last keyframe leaves: the estimates of the second run go back into the graph, the pose's row and its edges go
    write_back(g, fp, *h.state())
    gone = observed[-1]
    gone_id = int(np.asarray(g.pose_ids)[gone])
    stays = g.mono_vp != g.pose_ids[gone]
    rest = np.arange(g.nposes) != gone
    g = dataclasses.replace(g, pose_ids=g.pose_ids[rest], pose_fixed=g.pose_fixed[rest], pose_q=np.asarray(g.pose_q)[rest],
                            pose_t=np.asarray(g.pose_t)[rest], pose_cam=np.asarray(g.pose_cam)[rest], mono_vp=g.mono_vp[stays],
                            mono_vl=g.mono_vl[stays], mono_meas=g.mono_meas[stays], mono_info=g.mono_info[stays])
    fp = flatten(g)
    row_to_solver = np.full(g.nposes, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(len(fp.pose_src))
    k = np.nonzero(keep & (rows_i != gone) & (rows_j != gone))[0]
    h = HipSolver(fp, RK_HUBER)
    set_factors(h, k, row_to_solver, rows_i[k] - (rows_i[k] > gone), rows_j[k] - (rows_j[k] > gone))
    chi2 = h.optimize(iters)["chi2"]
    e = np.zeros(n)
    e[k] = h.pose_range_factor_chi_squares()
    out.append((chi2, None, e))
    return out, ids_i, ids_j, gone_id


@pytest.mark.gpu
def test_odometer_scale_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=5).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "3", "3", "1.05", "25"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    text = out.stdout
    start = float(re.search(r"^start scale ([0-9.eE+-]+)", text, re.M).group(1))
    assert abs(start - 1.05) <= 1e-12
    (first, refit, dropped), ids_i, ids_j, gone_id = _python_flow(path, 10, 3, 3.0, 1.05, 25.0)
    keys = list(zip((int(i) for i in ids_i), (int(j) for j in ids_j)))
    assert len(keys) == 40 and len(set(keys)) == 40
    gated = [(int(a), int(b)) for a, b in re.findall(r"^gated (\d+) (\d+)", text, re.M)]
    for prefix, (want_chi2, want_scale, want_e) in (("", first), ("refit ", refit), ("dropped ", dropped)):
        got_chi2 = np.array([float(m) for m in re.findall(r"^%siter:\s*\d+, chi2: ([0-9.eE+-]+)" % prefix, text, re.M)])
        got_scale = float(re.search(r"^%sscale ([0-9.eE+-]+)" % prefix, text, re.M).group(1)) if want_scale is not None else float("nan")
        got_e = {(int(a), int(b)): float(c) for a, b, c in re.findall(r"^%srange (\d+) (\d+) chi2 ([0-9.eE+-]+)" % prefix, text, re.M)}
        print("%sscale %.9g (C ABI flow %.9g), chi2 %.6g -> %.6g, largest factor chi2 %.4g, the others' %.4g"
              % (prefix, got_scale, float("nan") if want_scale is None else want_scale, got_chi2[0], got_chi2[-1], max(got_e.values()), sorted(got_e.values())[-2]))
        assert len(got_chi2) == len(want_chi2) and np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
        assert want_scale is None or abs(got_scale - want_scale) <= 1e-9
        assert sorted(got_e) == sorted(keys)
        # (e = Omega r^2 with r the difference of two distances of metres: the two flows may differ by a nanometre of distance -- as the
        # scale's bar above -- which moves e by 2 sqrt(Omega e) dr + Omega dr^2, not by a fraction of e)
        dr = 1e-9
        for k, key in enumerate(keys):
            assert abs(got_e[key] - want_e[k]) <= 2 * np.sqrt(want_e[k] / SIGMA ** 2) * dr + dr ** 2 / SIGMA ** 2
        # the odometer gives the monocular graph its scale back: at least four fifths of the 5 % the start was off by.  (The minimum itself
        # is not at 1: the file's estimate, at which the distances were measured, is a perturbed one and the reprojection edges have their
        # say -- the dense CPU model of the same flow, tests/pose_range_factor_reference.py, stands at 1.0082025 after ten iterations and
        # converges to 1.00802 in forty)
        assert want_scale is None or abs(got_scale - 1) <= 1e-2
    # Cauchy weights the gross range down: its chi2 stays far above every other's, the gate rejects it alone, and once removed it reports 0
    e = first[2]
    assert e[-1] > 100 * e[:-1].max() and e[:-1].max() <= 25.0
    assert gated == [keys[-1]]
    assert refit[2][-1] == 0.0 and float(re.search(r"^refit range %d %d chi2 ([0-9.eE+-]+)" % gated[0], text, re.M).group(1)) == 0.0
    assert refit[2][:-1].min() > 0
    # the pose that left took the factor touching it along: it reports 0, every other factor that was left still has its chi2
    assert int(re.search(r"^dropped (\d+)$", text, re.M).group(1)) == gone_id
    went = (ids_i == gone_id) | (ids_j == gone_id)
    assert went.sum() == 1 and not dropped[2][went].any() and (dropped[2][~went][:-1] > 0).all()
    for i, j in zip(ids_i[went], ids_j[went]):
        assert float(re.search(r"^dropped range %d %d chi2 ([0-9.eE+-]+)" % (i, j), text, re.M).group(1)) == 0.0

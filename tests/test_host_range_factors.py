"""The range factors of the C++ host layer (cuba::addRangeFactor / removeRangeFactor / rangeFactorChiSquared) through
host/samples/uwb_ranges.cpp: the sample builds without a GPU, and on the GPU its objective per iteration, the recovered scale, its
ranges' chi2 and the gated outlier -- in the first run, in the run after the gated factor was removed (removeRangeFactor) and in the
run after the last ranged pose was removed (removePoseVertex, which drops the pose's range factors: a factor left behind on a vertex
that is no longer part of the graph would make initialize() throw) -- are those of the same flow driven through the C ABI (HipSolver),
as tests/test_host_direction_factors.py does for the direction factors.  That addRangeFactor refuses a factor without a vertex is part
of host/host_selftest.cpp (tests/test_host_cpp.py)."""
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "uwb_ranges")
ARM = np.array([0.1, -0.2, 0.5])
SIGMA = 0.05
CORNERS = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])


def test_uwb_ranges_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/uwb_ranges"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout


def monocular(g):
    """the graph with every stereo edge as a monocular one (u, v), behind the monocular edges, every vertex free"""
    g = dataclasses.replace(g, mono_vp=np.concatenate([g.mono_vp, g.stereo_vp]), mono_vl=np.concatenate([g.mono_vl, g.stereo_vl]),
                            mono_meas=np.concatenate([np.asarray(g.mono_meas).reshape(-1, 2), np.asarray(g.stereo_meas).reshape(-1, 3)[:, :2]]),
                            mono_info=np.concatenate([g.mono_info, g.stereo_info]), stereo_vp=g.stereo_vp[:0], stereo_vl=g.stereo_vl[:0],
                            stereo_meas=np.asarray(g.stereo_meas).reshape(-1, 3)[:0], stereo_info=g.stereo_info[:0],
                            pose_fixed=np.zeros_like(g.pose_fixed), lm_fixed=np.zeros_like(g.lm_fixed))
    return g


def spread(c):
    return float(np.sqrt(((c - c.mean(axis=0)) ** 2).sum()))


def _python_flow(path, iters, stride, kernel, delta, scale0, gate):
    """the sample's flow through the C ABI: monocular edges only, every vertex free, four anchors at the corners of a tetrahedron about
    the camera centres, a range (information 1 / 0.05^2, arm 0.1 / -0.2 / 0.5) from each to every stride-th pose with an edge, the second
    5 m long, the start blown up by scale0; then the run without the ranges whose chi2 exceeds the gate; then, from there, the graph
    without the last ranged pose, its edges and its ranges"""
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten, write_back
    from oracle import oracle
    g = monocular(Graph.from_json(path))
    q0, t0 = np.asarray(g.pose_q, dtype=np.float64), np.asarray(g.pose_t, dtype=np.float64)
    seen = np.zeros(int(g.pose_ids.max()) + 1, dtype=bool)
    seen[g.mono_vp] = True
    observed = np.nonzero(seen[g.pose_ids])[0]
    world = lambda r, a, t: oracle.quat_to_rot(q0[r]).T @ (a - t)  # noqa: E731
    file_centres = np.array([world(r, np.zeros(3), t0[r]) for r in observed])
    reach = max(5.0, spread(file_centres) / np.sqrt(len(observed)))
    anchors = file_centres.mean(axis=0) + reach * CORNERS
    rows = np.repeat(observed[::stride], 4)
    which = np.tile(np.arange(4), len(rows) // 4)
    rng = np.array([np.linalg.norm(world(r, ARM, t0[r]) - anchors[k]) for r, k in zip(rows, which)])
    rng[1] += 5.0
    g = dataclasses.replace(g, pose_t=t0 * scale0, lm_X=np.asarray(g.lm_X, dtype=np.float64) * scale0)
    fp = flatten(g)
    row_to_solver = np.full(g.nposes, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(len(fp.pose_src))
    poses = row_to_solver[rows]
    n = len(rows)
    ids = np.asarray(g.pose_ids)[rows]

    def scale_of(h):
        q, t, _ = h.state()
        c = np.array([-oracle.quat_to_rot(q[p]).T @ t[p] for p in row_to_solver[observed]])
        return spread(c) / spread(file_centres)

    h = HipSolver(fp, RK_HUBER)
    keep = np.ones(n, dtype=bool)
    out = []
    for _ in range(2):
        k = np.nonzero(keep)[0]
        h.set_range_factors(poses[k], anchors[which[k]], rng[k], np.full(len(k), 1 / SIGMA ** 2), np.tile(ARM, (len(k), 1)),
                            kernel if kernel else None, delta if kernel else None)
        chi2 = h.optimize(iters)["chi2"]
        e = np.zeros(n)
        e[k] = h.range_factor_chi_squares()
        out.append((chi2, scale_of(h), e))
        keep = keep & (e <= gate)
    # the last ranged pose leaves: the estimates of the second run go back into the graph, the pose's row and its edges go
    write_back(g, fp, *h.state())
    gone = rows[-1]
    stays = g.mono_vp != g.pose_ids[gone]
    rest = np.arange(g.nposes) != gone
    g = dataclasses.replace(g, pose_ids=g.pose_ids[rest], pose_fixed=g.pose_fixed[rest], pose_q=np.asarray(g.pose_q)[rest],
                            pose_t=np.asarray(g.pose_t)[rest], pose_cam=np.asarray(g.pose_cam)[rest], mono_vp=g.mono_vp[stays],
                            mono_vl=g.mono_vl[stays], mono_meas=g.mono_meas[stays], mono_info=g.mono_info[stays])
    fp = flatten(g)
    row_to_solver = np.full(g.nposes, -1, dtype=np.int64)
    row_to_solver[np.asarray(fp.pose_src)] = np.arange(len(fp.pose_src))
    k = np.nonzero(keep & (rows != gone))[0]
    h = HipSolver(fp, RK_HUBER)
    h.set_range_factors(row_to_solver[rows[k] - (rows[k] > gone)], anchors[which[k]], rng[k], np.full(len(k), 1 / SIGMA ** 2),
                        np.tile(ARM, (len(k), 1)), kernel if kernel else None, delta if kernel else None)
    chi2 = h.optimize(iters)["chi2"]
    e = np.zeros(n)
    e[k] = h.range_factor_chi_squares()
    out.append((chi2, None, e))
    return out, ids, which


@pytest.mark.gpu
def test_uwb_ranges_sample_matches_the_c_abi_flow(tmp_path):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=5).to_json(path)
    out = subprocess.run([SAMPLE, path, "10", "5", "3", "3", "1.05", "25"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    text = out.stdout
    start = float(re.search(r"^start scale ([0-9.eE+-]+)", text, re.M).group(1))
    assert abs(start - 1.05) <= 1e-12
    (first, refit, dropped), ids, which = _python_flow(path, 10, 5, 3, 3.0, 1.05, 25.0)
    assert len(ids) == 32
    gated = [(int(a), int(b)) for a, b in re.findall(r"^gated (\d+) (\d+)", text, re.M)]
    for prefix, (want_chi2, want_scale, want_e) in (("", first), ("refit ", refit), ("dropped ", dropped)):
        got_chi2 = np.array([float(m) for m in re.findall(r"^%siter:\s*\d+, chi2: ([0-9.eE+-]+)" % prefix, text, re.M)])
        got_scale = float(re.search(r"^%sscale ([0-9.eE+-]+)" % prefix, text, re.M).group(1)) if want_scale is not None else float("nan")
        got_e = {(int(a), int(b)): float(c) for a, b, c in re.findall(r"^%srange (\d+) (\d+) chi2 ([0-9.eE+-]+)" % prefix, text, re.M)}
        print("%sscale %.9g (C ABI flow %.9g), chi2 %.6g -> %.6g, largest range chi2 %.4g, the others' %.4g"
              % (prefix, got_scale, float("nan") if want_scale is None else want_scale, got_chi2[0], got_chi2[-1], max(got_e.values()), sorted(got_e.values())[-2]))
        assert len(got_chi2) == len(want_chi2) and np.all(np.abs(got_chi2 - want_chi2) <= 1e-9 * want_chi2)
        assert want_scale is None or abs(got_scale - want_scale) <= 1e-9
        assert sorted(got_e) == sorted(zip((int(i) for i in ids), (int(k) for k in which)))
        # (e = Omega r^2 with r the difference of two ranges of ~10 m: the two flows may differ by a nanometre of range -- 1e-10 of it, as the
        # scale's bar above -- which moves e by 2 sqrt(Omega e) dr + Omega dr^2, not by a fraction of e: a range that fits to 0.1 mm has
        # e = 6e-6 and lost five digits to the subtraction.  Seen on the MI355X: 9e-13 m)
        dr = 1e-9
        for k, key in enumerate(zip((int(i) for i in ids), (int(k) for k in which))):
            assert abs(got_e[key] - want_e[k]) <= 2 * np.sqrt(want_e[k] / SIGMA ** 2) * dr + dr ** 2 / SIGMA ** 2
        # the ranges give the monocular graph its scale back: from 5 % off to within 0.5 % in ten iterations (0.25 % on the dense CPU model
        # of the same flow, still descending; the file's estimate is itself a perturbed one)
        assert want_scale is None or abs(got_scale - 1) <= 5e-3
    # Cauchy weights the gross range down: its chi2 stays far above every other's, the gate rejects it alone, and once removed it reports 0
    e = first[2]
    assert e[1] > 100 * np.delete(e, 1).max() and np.delete(e, 1).max() <= 25.0
    assert gated == [(int(ids[1]), int(which[1]))]
    assert refit[2][1] == 0.0 and float(re.search(r"^refit range %d %d chi2 ([0-9.eE+-]+)" % gated[0], text, re.M).group(1)) == 0.0
    assert np.delete(refit[2], 1).max() > 0
    # the pose that left took its four ranges with it: they report 0, every other range that was left still has its chi2
    assert int(re.search(r"^dropped (\d+)$", text, re.M).group(1)) == int(ids[-1])
    went = ids == ids[-1]
    assert went.sum() == 4 and not dropped[2][went].any() and (np.delete(dropped[2][~went], 1) > 0).all()
    for i, k in zip(ids[went], which[went]):
        assert float(re.search(r"^dropped range %d %d chi2 ([0-9.eE+-]+)" % (i, k), text, re.M).group(1)) == 0.0

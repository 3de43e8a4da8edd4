"""Pose localisation in the C++ host layer (cuba::localizePoses / poseLocalizationStatus), without a GPU.

host/test/localize_trace.cpp -- the host layer over the recording stand-ins for the device library -- shows what crosses the C ABI and
what the vertices hold after every step.  Its graph: four free poses of ids 7, 3, 9, 5, so the solver numbers them 3, 5, 7, 9 -> 0, 1, 2,
3; the program prints them in the order 7, 3, 9, 5.  The stand-in accepts the solver poses 0 and 3 (q = (0, 1, 0, 0), t = (1000 + p,
2000 + p, 3000 + p)), calls 1 FEW_INLIERS and 2 NO_SOLUTION."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
OK, NOT_SELECTED, NO_SOLUTION, FEW_INLIERS = 0, 1, 4, 5

_trace = []


def trace():
    if not _trace:
        subprocess.check_call(["make", "-C", HOST, "-s", "localize_trace"])
        out = subprocess.run([os.path.join(HOST, "localize_trace")], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        steps, name = {}, None
        for line in out.stdout.splitlines():
            if line.startswith("# ") and not re.match(r"# [a-z ]+: status|# counts|# foreign", line):
                name = line[2:]; steps[name] = []
            elif name is not None:
                steps[name].append(line)
        shown = {m.group(1): ([int(v) for v in m.group(2).split()], [float(v) for v in m.group(3).split()])
                 for m in re.finditer(r"^# ([a-z ]+): status ([0-9 ]+), qt ([-0-9.e+ ]+)$", out.stdout, re.M)}
        _trace.append((out.stdout, steps, shown))
    return _trace[0]


def calls(lines):
    """every cuba_hip_localize_poses line as (hypotheses, seed, chi2 mono, chi2 stereo, min_inliers, dry_run, mask or None, outputs)"""
    out = []
    for l in lines:
        if l.startswith("cuba_hip_localize_poses"):
            head, mask, outputs = l.split(" | ")
            f = head.split()[1:]
            out.append((int(f[0]), int(f[1]), float.fromhex(f[2]), float.fromhex(f[3]), int(f[4]), int(f[5]), None if mask == "null" else mask,
                        outputs.split()[1]))
    return out


HALF = [0.5, 0.5, 0.5, 0.5]
FOUND = [0, 1, 0, 0]


def poses(t7, t3, t9, t5, q3=HALF, q9=HALF):
    return HALF + t7 + q3 + t3 + q9 + t9 + HALF + t5


def test_calls_statuses_and_poses():
    text, steps, shown = trace()
    start = poses([7, 0, 0], [3, 0, 0], [9, 0, 0], [5, 0, 0])
    assert shown["before"] == ([NOT_SELECTED] * 4, start)               # NOT_SELECTED before any call
    # 1. all poses: the graph goes up first, then ONE call with the defaults (256 hypotheses, seed 0, 5.991 / 7.815, 10 inliers, no dry run,
    #    no mask); status, counts, q and t are asked for, inliers, cost, winner and edge_inlier are not
    first = steps["all poses with the default options"]
    assert [l.split()[0] for l in first if l.startswith(("cuba_hip_set_graph_begin", "cuba_hip_localize"))] == ["cuba_hip_set_graph_begin", "cuba_hip_localize_poses"]
    assert calls(first) == [(256, 0, 5.991, 7.815, 10, 0, None, "11000110")]
    assert "# counts 2 0 0 0 1 1" in first
    after_all = poses([7, 0, 0], [1000, 2000, 3000], [1003, 2003, 3003], [5, 0, 0], q3=FOUND, q9=FOUND)
    # (printed order 7, 3, 9, 5 = solver 2, 0, 3, 1) the OK poses land in their vertex objects, the others stay
    assert shown["all"] == ([NO_SOLUTION, OK, OK, FEW_INLIERS], after_all)
    # 2. a dry run on {9, 3, null}: the mask in SOLVER numbering (3 -> 0, 9 -> 3), the options as given (a seed above 2^63 too); no vertex changes
    dry = steps["a dry run on a subset with options of its own"]
    assert calls(dry) == [(77, 2 ** 64 - 59, 4.0, 6.0, 5, 1, "4 1 0 0 1", "11000110")]
    assert not any(l.startswith("cuba_hip_set_graph") for l in dry) and "# counts 2 2 0 0 0 0" in dry
    moved = poses([7, 0, 0], [1000, 2000, 3000], [-9, 0, 0], [5, 0, 0], q3=FOUND, q9=FOUND)       # (the caller moved pose 9 before the dry run)
    assert shown["dry run"] == ([NOT_SELECTED, OK, OK, NOT_SELECTED], moved)
    # 3. the same for real: pose 9 gets the stand-in's value again
    real = steps["the same subset for real"]
    assert calls(real) == [(77, 2 ** 64 - 59, 4.0, 6.0, 5, 0, "4 1 0 0 1", "11000110")]
    assert shown["subset"] == ([NOT_SELECTED, OK, OK, NOT_SELECTED], after_all)
    # 4. optimize afterwards: no new upload (the handle holds the poses), and the vertices keep them
    opt = steps["the next optimize starts from the new poses"]
    assert not any(l.startswith("cuba_hip_set_graph") for l in opt) and any(l.startswith("cuba_hip_optimize 1") for l in opt)
    assert shown["optimized"][1] == after_all
    # 5. clear() drops the statuses
    assert shown["cleared"][0] == [NOT_SELECTED] * 4


def test_options_out_of_range_are_refused_before_any_call():
    text, steps, shown = trace()
    lines = steps["options out of range are refused before any call"]
    assert lines[:9] == [f"std::invalid_argument {k}" for k in range(9)]
    assert not any(l.startswith("cuba_hip_") for l in lines)
    assert shown["refused"] == shown["subset"]


def test_an_object_of_another_library_is_refused():
    text, steps, _ = trace()
    lines = steps["an object of another library is refused"]
    assert lines[0] == "std::runtime_error: cuba::localizePoses: not an object of this library"
    assert calls(lines) == [] and f"# foreign status {NOT_SELECTED}" in text


def test_the_stand_in_files_define_the_same_handle():
    """fake_cuba_hip_localize.cpp repeats struct cuba_hip_solver of fake_cuba_hip.cpp (one type in one program): token for token"""
    def handle(name):
        text = open(os.path.join(HOST, "test", name)).read()
        m = re.search(r"^struct cuba_hip_solver\n\{.*?^\};", text, re.M | re.S)
        assert m, name
        return m.group(0).split()
    assert handle("fake_cuba_hip_localize.cpp") == handle("fake_cuba_hip.cpp")


SAMPLE = os.path.join(HOST, "samples", "relocalise_keyframes")
NAMES = ("ok", "not_selected", "fixed", "few_observations", "no_solution", "few_inliers")


def test_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/relocalise_keyframes"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout and "hypotheses" in out.stdout


@pytest.mark.gpu
def test_sample_matches_the_c_abi_flow(tmp_path):
    """every third free pose (file order, from the second pose on) loses its value (NaN) and is localised, refined and optimised: the counts
    and run B's objective are those of the same flow through the C ABI"""
    import numpy as np
    from conftest import RK_HUBER
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=1, perturb=False).to_json(path)
    out = subprocess.run([SAMPLE, path, "10"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    g = Graph.from_json(path)
    fp = flatten(g)
    solver = {int(r): i for i, r in enumerate(fp.pose_src)}
    lost = [r for r in range(1, g.nposes) if not g.pose_fixed[r]][::3]
    select = np.zeros(fp.Pt, bool)
    q, t = fp.q.copy(), fp.t.copy()
    for r in lost:
        select[solver[r]] = True
        q[solver[r]], t[solver[r]] = np.nan, np.nan
    h = HipSolver(fp, RK_HUBER)
    h.set_state(q, t, fp.Xw)
    got = h.localize_poses(select=select)
    h.refine_poses(select=select)
    want = h.optimize(10)["chi2"]
    m = re.search(r"^localised (\d+) of (\d+): (.*)$", out.stdout, re.M)
    counts = dict(zip(m.group(3).split()[::2], map(int, m.group(3).split()[1::2])))
    assert counts == {k: got[k] for k in NAMES} and int(m.group(1)) == got["ok"] >= 1 and int(m.group(2)) == select.sum() == len(lost) == 13
    runs = {tag: np.array([float(v) for v in re.findall(r"^%s iter:\s*\d+, chi2: ([0-9.eE+-]+)" % tag, out.stdout, re.M)]) for tag in "AB"}
    assert len(runs["B"]) == len(want) and np.all(np.abs(runs["B"] - want) <= 1e-9 * want)
    assert len(runs["A"]) == 10 and runs["A"][-1] < runs["A"][0]
    # (every lost pose came back: the distance to run A's poses is a number; how small it is depends on how far ten iterations converge)
    assert got["ok"] < 13 or np.isfinite(float(re.search(r"^largest distance .*: ([0-9.eE+-]+|inf)$", out.stdout, re.M).group(1)))

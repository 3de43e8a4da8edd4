"""Landmark triangulation in the C++ host layer (cuba::triangulateLandmarks / triangulationStatus), without a GPU.

host/test/triangulate_trace.cpp -- the host layer over the recording stand-ins for the device library -- shows what crosses the C ABI and
what the vertices hold after every step.  Its graph: landmark ids 7, 3, 9, 5 (free) and 1 (fixed), so the solver numbers them 3, 5, 7, 9 ->
0, 1, 2, 3 and 1 -> 4; the program prints them in the order 7, 3, 9, 5, 1.  The stand-in accepts the solver landmarks 0 and 3 (positions
(100 + l, 200 + l, 300 + l)), calls 1 and 4 CHI2 and 2 LOW_PARALLAX."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
OK, NOT_SELECTED, LOW_PARALLAX, CHI2 = 0, 1, 4, 7


def trace():
    subprocess.check_call(["make", "-C", HOST, "-s", "triangulate_trace"])
    out = subprocess.run([os.path.join(HOST, "triangulate_trace")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    steps, name = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("# ") and not re.match(r"# [a-z ]+: status|# counts|# foreign", line):
            name = line[2:]; steps[name] = []
        elif name is not None:
            steps[name].append(line)
    shown = {m.group(1): ([int(v) for v in m.group(2).split()], [float(v) for v in m.group(3).split()])
             for m in re.finditer(r"^# ([a-z ]+): status ([0-9 ]+), Xw ([-0-9.e+ ]+)$", out.stdout, re.M)}
    return out.stdout, steps, shown


def calls(lines):
    """every cuba_hip_triangulate_landmarks line as (iterations, min_parallax_deg, chi2 mono, chi2 stereo, dry_run, mask or None)"""
    out = []
    for l in lines:
        if l.startswith("cuba_hip_triangulate_landmarks"):
            head, mask = l.split(" | ")
            f = head.split()[1:]
            out.append((int(f[0]), float.fromhex(f[1]), float.fromhex(f[2]), float.fromhex(f[3]), int(f[4]), None if mask == "null" else mask))
    return out


def test_calls_statuses_and_positions():
    text, steps, shown = trace()
    start = [7, 0, 5, 3, 0, 5, 9, 0, 5, 5, 0, 5, 1, 0, 5]
    assert shown["before"] == ([NOT_SELECTED] * 5, start)
    # 1. all landmarks: the graph goes up first, then ONE call with the defaults (5 iterations, 1 degree, 5.991 / 7.815, no dry run, no mask)
    first = steps["all landmarks with the default options"]
    assert [l.split()[0] for l in first if l.startswith(("cuba_hip_set_graph_begin", "cuba_hip_triangulate"))] == ["cuba_hip_set_graph_begin", "cuba_hip_triangulate_landmarks"]
    assert calls(first) == [(5, 1.0, 5.991, 7.815, 0, None)]
    assert "# counts 2 0 0 0 1 0 0 2" in first
    after_all = start[:3] + [100, 200, 300, 103, 203, 303] + start[9:]
    assert shown["all"] == ([LOW_PARALLAX, OK, OK, CHI2, CHI2], after_all)          # the OK positions land in their vertex objects, the others stay
    # 2. a dry run on {9, 3, null}: the mask in SOLVER numbering (3 -> 0, 9 -> 3), the options as given; no vertex changes
    dry = steps["a dry run on a subset with options of its own"]
    assert calls(dry) == [(3, 0.5, 4.0, 6.0, 1, "5 1 0 0 1 0")]
    assert not any(l.startswith("cuba_hip_set_graph") for l in dry) and "# counts 2 3 0 0 0 0 0 0" in dry
    moved = after_all[:6] + [-9, 0, 5] + after_all[9:]                            # (the caller moved landmark 9 before the dry run)
    assert shown["dry run"] == ([NOT_SELECTED, OK, OK, NOT_SELECTED, NOT_SELECTED], moved)
    # 3. the same for real: landmark 9 gets the accepted position again
    real = steps["the same subset for real"]
    assert calls(real) == [(3, 0.5, 4.0, 6.0, 0, "5 1 0 0 1 0")]
    assert shown["subset"] == ([NOT_SELECTED, OK, OK, NOT_SELECTED, NOT_SELECTED], after_all)
    # 4. optimize afterwards: no new upload (the handle holds the positions), and the vertices keep them
    opt = steps["the next optimize starts from the accepted positions"]
    assert not any(l.startswith("cuba_hip_set_graph") for l in opt) and any(l.startswith("cuba_hip_optimize 1") for l in opt)
    assert shown["optimized"][1] == after_all
    # 5. clear() drops the statuses
    assert shown["cleared"][0] == [NOT_SELECTED] * 5


def test_an_object_of_another_library_is_refused():
    text, steps, _ = trace()
    lines = steps["an object of another library is refused"]
    assert lines[0] == "std::runtime_error: cuba::triangulateLandmarks: not an object of this library"
    assert calls(lines) == [] and f"# foreign status {NOT_SELECTED}" in text


def test_the_other_trace_programs_link_the_new_stand_in():
    for target in ("factor_trace", "gate_trace"):
        subprocess.check_call(["make", "-C", HOST, "-s", target])


def test_the_two_stand_in_files_define_the_same_handle():
    """fake_cuba_hip_triangulate.cpp repeats struct cuba_hip_solver of fake_cuba_hip.cpp (one type in one program): token for token"""
    def handle(name):
        text = open(os.path.join(HOST, "test", name)).read()
        m = re.search(r"^struct cuba_hip_solver\n\{.*?^\};", text, re.M | re.S)
        assert m, name
        return m.group(0).split()
    assert handle("fake_cuba_hip_triangulate.cpp") == handle("fake_cuba_hip.cpp")


SAMPLE = os.path.join(HOST, "samples", "triangulate_new_points")
NAMES = ("ok", "not_selected", "fixed", "few_observations", "low_parallax", "singular", "behind_camera", "chi2")


def test_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/triangulate_new_points"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout and "min_parallax_deg" in out.stdout


@pytest.mark.gpu
def test_sample_matches_the_c_abi_flow(tmp_path):
    """every third free landmark (file order) starts at zero and is triangulated: the counts and run B's objective are those of the same flow
    through the C ABI"""
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
    free_rows = [r for r in range(g.nlandmarks) if not g.lm_fixed[r]]
    solver = {int(r): i for i, r in enumerate(fp.lm_src)}
    select = np.zeros(fp.Lt, bool)
    select[[solver[r] for r in free_rows[::3] if r in solver]] = True
    h = HipSolver(fp, RK_HUBER)
    X = fp.Xw.copy(); X[select] = 0.0
    h.set_state(fp.q, fp.t, X)
    got = h.triangulate_landmarks(select=select)
    want = h.optimize(10)["chi2"]
    m = re.search(r"^triangulated (\d+) of (\d+): (.*)$", out.stdout, re.M)
    counts = dict(zip(m.group(3).split()[::2], map(int, m.group(3).split()[1::2])))
    assert counts == {k: got[k] for k in NAMES} and int(m.group(1)) == got["ok"] > 150 and int(m.group(2)) == select.sum() == 200
    runs = {tag: np.array([float(v) for v in re.findall(r"^%s iter:\s*\d+, chi2: ([0-9.eE+-]+)" % tag, out.stdout, re.M)]) for tag in "AB"}
    assert len(runs["B"]) == len(want) and np.all(np.abs(runs["B"] - want) <= 1e-9 * want)
    # (the rejected landmarks -- outliers among their few views -- still sit at zero in run B and weigh on its objective: 6.3e5 against run
    # A's 9.6e3 with 39 of the 200 rejected; a pipeline would cull them)
    assert len(runs["A"]) == 10 and runs["A"][-1] < runs["A"][0] and runs["B"][-1] <= runs["B"][0]

"""Edge gating in the C++ host layer (cuba::gateEdges / setEdgeActive / edgeActive / edgeGateChiSquared / activeObservations).

Without a GPU: host/samples/outlier_gating.cpp builds and prints its usage, and host/test/gate_trace.cpp -- the host layer over the
recording stand-in for the device library -- shows what crosses the C ABI and what the levels are after every step: nothing for an
object that never gates, the mask once per change and again after every upload of the graph, the levels of edges that stay in the graph
kept, those of edges that leave dropped, a null mask when the last edge is switched on again.

On the GPU: the sample's objective per iteration, its counts per classification and its landmarks left with fewer than two active
observations are those of the same flow through the C ABI (HipSolver), for the 5 + 10 flow and for the four-round re-admitting flow --
as tests/test_host_range_factors.py does for its sample."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, RK_HUBER

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "outlier_gating")
COUNTS = r"active (\d+) (\d+), gated by chi2 (\d+) (\d+), gated by depth (\d+), changed (\d+)"
NAMES = ("active_mono", "active_stereo", "gated_chi2_mono", "gated_chi2_stereo", "gated_depth", "changed")


def test_outlier_gating_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/outlier_gating"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout and "--rounds" in out.stdout


def test_levels_and_c_abi_traffic_of_the_host_layer():
    subprocess.check_call(["make", "-C", HOST, "-s", "gate_trace"])
    out = subprocess.run([os.path.join(HOST, "gate_trace")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    steps, name = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("# ") and not re.match(r"# [a-z0-9 ]+: active|# counts", line):
            name = line[2:]; steps[name] = []
        elif name is not None:
            steps[name].append(line)
    by = {k.split(":")[0].split(",")[0]: v for k, v in steps.items()}
    gate_calls = lambda lines: [l for l in lines if re.match(r"cuba_hip_(gate_edges|set_edge_active|get_edge_active|landmark_active_edges)", l)]  # noqa: E731
    levels = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"^# ([a-z0-9 ]+): active ([01 ]+), observations (\d+ \d+)$", out.stdout, re.M)}
    assert gate_calls(by["no gate"]) == [] and levels["plain"] == ("1 1 1 1", "2 2")
    assert levels["e10 off"] == ("1 0 1 1", "1 2")
    assert gate_calls(by["a level set by hand goes up with the next optimize"]) == ["cuba_hip_set_edge_active mask 1"]      # once for two runs
    g = gate_calls(by["gateEdges"])
    assert len(g) == 3 and g[0].endswith(" 1 2") and g[1].endswith(" 1 0") and g[2] == "cuba_hip_get_edge_active"
    assert levels["dry run"] == ("1 0 1 1", "1 2") and levels["classified"] == ("1 1 1 1", "2 2")
    assert "# counts 0 4 0 0 0 0, ungated chi2 0 1 2 3" in out.stdout
    # e01 and e11 switched off, e11 removed and added again: e01 keeps its level through both uploads, e11 comes back switched on
    assert gate_calls(by["the levels survive a change of the graph that keeps the edge; the level of an edge that leaves goes with it"]) == \
        ["cuba_hip_set_edge_active mask 1", "cuba_hip_set_edge_active mask 1"]
    assert levels["e11 removed"] == ("1 1 0 1", "2 0") and levels["e11 back"] == ("1 1 0 1", "2 1")
    assert gate_calls(by["the last level switched on again"]) == ["cuba_hip_set_edge_active null 0"]
    assert gate_calls(by["clear() drops all levels"]) == [] and levels["cleared"] == ("1 1 1 1", "0 0")


def _python_flow(path, iters1, iters2, rounds):
    from cuba_amd.capi import HipSolver
    from cuba_amd.graph import Graph, flatten
    fp = flatten(Graph.from_json(path))
    h = HipSolver(fp, RK_HUBER)
    runs, counts = [], []
    if rounds:
        for _ in range(rounds):
            runs.append(h.optimize(iters2)["chi2"])
            counts.append(h.gate_edges())
    else:
        runs.append(h.optimize(iters1)["chi2"])
        counts.append(h.gate_edges())
        runs.append(h.optimize(iters2)["chi2"])
    per_lm = h.landmark_active_edges()
    return runs, counts, int((~h.edge_active()).sum()), int((per_lm < 2).sum()), fp


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [0, 4])
def test_outlier_gating_sample_matches_the_c_abi_flow(tmp_path, rounds):
    from cuba_amd.synth import synth_ba
    path = str(tmp_path / "graph.json")
    synth_ba(40, 600, 2400, seed=1).to_json(path)
    out = subprocess.run([SAMPLE, path, "5", "10"] + (["--rounds", str(rounds)] if rounds else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    text = out.stdout
    runs, counts, off, weak, fp = _python_flow(path, 5, 10, rounds)
    prefixes = [f"round {r} " for r in range(rounds)] if rounds else ["stage1 ", "stage2 "]
    for prefix, want in zip(prefixes, runs):
        got = np.array([float(m) for m in re.findall(r"^%siter:\s*\d+, chi2: ([0-9.eE+-]+)" % prefix, text, re.M)])
        assert len(got) == len(want) and np.all(np.abs(got - want) <= 1e-9 * want), (prefix, got, want)
    got_counts = [dict(zip(NAMES, map(int, m))) for m in re.findall(r"^(?:gate|round) \d+: " + COUNTS, text, re.M)]
    assert got_counts == [{k: c[k] for k in NAMES} for c in counts]
    assert int(re.search(r"^switched off (\d+) of (\d+) edges", text, re.M).group(1)) == off
    assert int(re.search(r"^landmarks with fewer than two active observations: (\d+)", text, re.M).group(1)) == weak
    if not rounds:
        # the figures of the flow on this graph (tests/test_edge_gate_reference.py)
        assert got_counts[0] == dict(active_mono=328, active_stereo=1945, gated_chi2_mono=15, gated_chi2_stereo=112, gated_depth=0, changed=127)
        assert off == 127 and weak == 14 and abs(runs[1][0] - 4185.5) < 0.05 and abs(runs[1][-1] - 3884.7) < 0.05
    else:
        assert any(c["changed"] > 0 for c in got_counts[1:])            # later rounds do move edges in and out

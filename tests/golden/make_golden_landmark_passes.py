"""Generates tests/golden/landmark_passes_bits.json: the exact bits of every kernel that walks the reprojection edges landmark by landmark,
in its wave form (runs of landmarks with at most 64 edges) and in its workgroup form (one landmark with more than 64 edges), through the
step API and through whole LM runs -- the per-edge chi2, the landmark systems of both modes of the landmark pass, the reduced system, the
step API's back substitution (xl) and its gain-ratio denominator, the update, and the single-launch trial tail of cuba_hip_optimize --
on the fp64 library, the fp32 library and the fp64 library with mixed_precision=1.  Three graphs: the trial-chain fixture's 40-pose graph
with one free landmark of 65 to 256 edges; the landmark-prior fixture's 600-pose graph with free landmarks of more than 256 edges (the
workgroup's strided edge loop makes more than one trip); and that graph with its largest landmark moved among the fixed ones (the
workgroup kernels' fixed-landmark branches).  Doubles are stored as float.hex() strings, arrays as the sha256 of their bytes plus their
length.  tests/test_gpu_landmark_passes_bits.py recomputes every entry through record() below and asserts equality: the fixture pins a
change that must leave the results alone (a refactor of the landmark kernels) to the commit it was recorded at.  Needs the GPU; re-record
when the toolchain changes (the fixture names the hipcc it was built with), at a commit whose results are trusted.  Run from the repo
root: `python tests/golden/make_golden_landmark_passes.py`."""
import dataclasses
import functools
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
from conftest import RK_HUBER  # noqa: E402

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "landmark_passes_bits.json")
CONFIGS = {"f64": dict(precision="f64"), "f32": dict(precision="f32"), "f64_mixed": dict(precision="f64", mixed_precision=1)}
GRAPHS = ("g40_big", "big", "big_fixed")
LAMBDA = 0.9


def arr(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "len": int(a.size)}


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


@functools.lru_cache(maxsize=None)
def _sibling(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def edge_counts(fp):
    return np.bincount(fp.eL, minlength=fp.Lt)


def fix_landmark(fp, il):
    """fp with free landmark il moved behind the last landmark, among the fixed ones (flatten()'s order: free before fixed); its edges to
    fixed poses go, as flatten() drops an edge with both ends fixed"""
    assert 0 <= il < fp.Lf
    order = np.concatenate([np.arange(il), np.arange(il + 1, fp.Lt), [il]])
    new = np.empty(fp.Lt, dtype=np.int64); new[order] = np.arange(fp.Lt)
    keep = ~((fp.eL == il) & (fp.eP >= fp.Pf))
    return dataclasses.replace(fp, Lf=fp.Lf - 1, Xw=np.ascontiguousarray(fp.Xw[order]), lm_src=fp.lm_src[order],
                               eP=np.ascontiguousarray(fp.eP[keep]), eL=new[fp.eL[keep]].astype(np.int32), eDim=np.ascontiguousarray(fp.eDim[keep]),
                               meas=np.ascontiguousarray(fp.meas[keep]), omega=np.ascontiguousarray(fp.omega[keep]), edge_src=fp.edge_src[keep])


@functools.lru_cache(maxsize=None)
def graph(name):
    """the FlatProblem of a case; the assertions are what makes the case what it is"""
    if name == "g40_big":
        fp = flatten(_sibling("make_golden_trial_chain").with_big_landmark(synth_ba(40, 600, 2400, seed=1)))
        n = edge_counts(fp)[:fp.Lf]
        assert (n > 64).sum() == 1 and n.max() <= 256, n[n > 64]         # one free landmark for the workgroup kernels, one trip of their loop
        return fp
    fp = _sibling("make_golden_landmark_priors").big_graph()[0]
    n = edge_counts(fp)
    assert ((n[:fp.Lf] > 64) & (n[:fp.Lf] <= 256)).any() and (n[:fp.Lf] > 256).any() and not (n[fp.Lf:] > 64).any(), n[n > 64]
    if name == "big":
        return fp
    assert name == "big_fixed"
    fx = fix_landmark(fp, int(np.argmax(n[:fp.Lf])))
    m = edge_counts(fx)
    assert fx.Lf == fp.Lf - 1 and m[fx.Lt - 1] > 256, m[fx.Lt - 1]        # a fixed landmark among the big ones ...
    assert (m[:fx.Lf] > 256).any() and ((m[:fx.Lf] > 64) & (m[:fx.Lf] <= 256)).any(), m[m > 64]     # ... next to free ones of both sizes
    return fx


def state(h, out, prefix=""):
    q, t, X = h.state()
    out[prefix + "q"], out[prefix + "t"], out[prefix + "Xw"] = arr(q), arr(t), arr(X)


def record(config, name):
    fp = graph(name)
    out = {}
    h = HipSolver(fp, RK_HUBER, **CONFIGS[config])
    out["compute_errors"] = float(h.compute_errors()).hex()
    out["chi_squares"] = arr(h.chi_squares())
    h.build_system()
    h.assemble()                                      # (the mode-0 landmark pass; max_diagonal() below runs it once more)
    out["lm_sys_mode0"] = arr(h.array("lm_sys"))
    out["max_diagonal"] = float(h.max_diagonal()).hex()
    h.set_lambda(LAMBDA)
    h.schur()
    out["lm_sys_mode1"] = arr(h.array("lm_sys"))
    out["hsc"] = arr(h.array("hsc"))
    out["bsc"] = arr(h.array("bsc"))
    assert h.solve()
    out["xp"] = arr(h.array("xp"))
    h.back_substitute()
    out["xl"] = arr(h.array("xl"))
    out["compute_scale"] = float(h.compute_scale(LAMBDA)).hex()
    h.update()
    state(h, out, "updated_")
    out["updated_compute_errors"] = float(h.compute_errors()).hex()
    h = HipSolver(fp, RK_HUBER, **CONFIGS[config])
    out["optimize"] = hexes(h.optimize(3)["chi2"])
    state(h, out, "optimize_")
    out["optimize_lm_trials"] = h.counters()["lm_trials"]
    assert h.counter("late_decision_records") == 0
    return out


if __name__ == "__main__":
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_landmark_passes.py", "hipcc_version": hipcc}
    for config in CONFIGS:
        out[config] = {name: record(config, name) for name in GRAPHS}
        print(config, {name: (o["optimize"][-1], o["optimize_lm_trials"]) for name, o in out[config].items()}, flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(out, f, indent=1)

"""Generates tests/golden/factor_kinds_bits.json: the exact bits of what the solver computes with the factor kinds and instantiations that
pose_factors_bits.json and landmark_priors_bits.json leave out -- position factors and direction factors (each alone, without and with
robust kernels), pose priors and relative-pose edges WITH robust kernels, all five kinds on one handle, sets large enough for several chi2
partials per kind (the offsets into the partials buffer; the direction factors past the chi2 kernel's 64 workgroups of 256 threads, so its
grid-stride loop runs), and a graph whose pose ids are shuffled -- on the fp64 and the fp32 library.  Doubles are stored as float.hex()
strings, arrays as the sha256 of their bytes plus their length.  tests/test_gpu_factor_kinds_bits.py recomputes every entry through
record() below and asserts equality: the fixture pins a change that must leave the results alone (a refactor of the factor code) to the
commit it was recorded at.  Needs the GPU; re-record when the toolchain changes (the fixture names the hipcc it was built with).  Run from
the repo root: `python tests/golden/make_golden_factor_kinds.py`."""
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
import direction_factor_reference as dr  # noqa: E402
import landmark_prior_reference as lr  # noqa: E402
import position_factor_reference as pfr  # noqa: E402
import robust_pose_factor_reference as rb  # noqa: E402
from conftest import RK_HUBER  # noqa: E402
from test_gpu_configs import shuffled_pose_ids  # noqa: E402
from test_gpu_direction_factors import main_set as direction_main_set  # noqa: E402
from test_gpu_landmark_priors import main_set as landmark_main_set  # noqa: E402
from test_gpu_pose_priors import make_priors  # noqa: E402
from test_gpu_position_factors import DELTAS, main_set as position_main_set  # noqa: E402
from test_gpu_relative_pose import make_rel  # noqa: E402

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "factor_kinds_bits.json")
PRECISIONS = ("f64", "f32")
PRIORS, EDGES = 0, 1
# many_parts: factors per kind, each a different multiple of the chi2 workgroup (256) plus something; the direction factors one more than
# the 64 workgroups of a chi2 launch hold in one trip
MANY = dict(priors=300, rel=600, lmp=900, pos=1200, dir=64 * 256 + 1)
MANY_ITERATIONS = 3


def arr(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "len": int(a.size)}


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def _pose_factors():
    spec = importlib.util.spec_from_file_location("make_golden_pose_factors", os.path.join(HERE, "make_golden_pose_factors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.factors


def cycling(s):
    """a position / direction / landmark set with the kernels none / Huber / Tukey / Cauchy in turn, the sibling tests' deltas"""
    kind = (np.arange(len(s[0])) % 4).astype(np.int32)
    return s[:-2] + (kind, np.array([DELTAS[int(k)] for k in kind]))


def pose_kernels(n, shift):
    """kernels of n pose priors / relative-pose edges, the four kinds in turn, delta^2 4 and 4000 in runs of four
    (tests/test_gpu_robust_pose_factors.py: the case of more than one workgroup)"""
    k = np.arange(n)
    return ((k + shift) % 4).astype(np.int32), np.sqrt(np.where((k // 4) % 2 == 0, 4.0, 4000.0))


def names_twice_and_fixed(fp, poses):
    poses = np.asarray(poses).ravel()
    return len(poses) != len(set(poses.tolist())) and (poses >= fp.Pf).any()


@functools.lru_cache(maxsize=None)
def g40():
    return flatten(synth_ba(40, 600, 2400, seed=1))


@functools.lru_cache(maxsize=None)
def shuffled60():
    return flatten(shuffled_pose_ids(synth_ba(60, 900, 3600, seed=2), seed=1))


def all_five(fp):
    """the sets of tests/test_gpu_direction_factors.py::test_with_every_other_kind_of_factor"""
    return dict(priors=make_priors(fp, [1, 5, 17], seed=1), rel=make_rel(fp, [(3, 20)], seed=2),
                lmp=lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0),
                pos=pfr.make_factors(fp, [5, 8, 22], seed=4, kind=rb.HUBER, delta=2.0), dir=direction_main_set(fp, rb.CAUCHY))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the sets of a handle on g40(): priors, rel, lmp, pos, dir, and the pose factors' kernels kp, kr"""
    fp = g40()
    pri, rel = _pose_factors()(fp)
    out = {
        "position": dict(pos=position_main_set(fp)),
        "position_robust": dict(pos=cycling(position_main_set(fp))),
        "direction": dict(dir=direction_main_set(fp)),
        "direction_robust": dict(dir=cycling(direction_main_set(fp))),
        "pose_robust": dict(priors=pri, rel=rel, kp=pose_kernels(len(pri[0]), 1), kr=pose_kernels(len(rel[0]), 0)),
        "all_five": all_five(fp),
    }
    for name in ("position", "position_robust"):
        assert names_twice_and_fixed(fp, out[name]["pos"][0])
    for name in ("direction", "direction_robust"):
        assert names_twice_and_fixed(fp, out[name]["dir"][0])
    assert names_twice_and_fixed(fp, pri[0]) and names_twice_and_fixed(fp, np.concatenate([rel[0], rel[1]]))
    for name, key in (("position_robust", "pos"), ("direction_robust", "dir")):
        assert sorted(set(out[name][key][4].tolist())) == [0, 1, 2, 3]
    return out


@functools.lru_cache(maxsize=None)
def many_parts():
    """every kind with more than one chi2 workgroup on one handle: the poses, pairs and landmarks of the small sets repeated, with fresh
    seeded values; the pose priors and the position factors with kernels in turn, the edges and the direction factors without"""
    fp = g40()
    pri, rel = _pose_factors()(fp)
    pairs = list(zip(rel[0].tolist(), rel[1].tolist()))
    pos_poses, dir_poses, lms = position_main_set(fp)[0], direction_main_set(fp)[0], landmark_main_set(fp)[0]
    out = dict(priors=make_priors(fp, np.resize(pri[0], MANY["priors"]), seed=21),
               rel=make_rel(fp, [pairs[k % len(pairs)] for k in range(MANY["rel"])], seed=22),
               lmp=cycling(lr.make_priors(fp, np.resize(lms, MANY["lmp"]), seed=23, kind=rb.HUBER, delta=2.0)),
               pos=cycling(pfr.make_factors(fp, np.resize(pos_poses, MANY["pos"]), seed=24)),
               dir=dr.make_factors(fp, np.resize(dir_poses, MANY["dir"]), seed=25),
               kp=pose_kernels(MANY["priors"], 1))
    sizes = [len(out[k][0]) for k in ("priors", "rel", "lmp", "pos", "dir")]
    assert sizes == [300, 600, 900, 1200, 16385] and all(n > 256 and n % 256 for n in sizes)
    return out


def handle(fp, precision, sets, **opts):
    h = HipSolver(fp, RK_HUBER, precision=precision, **opts)
    if "priors" in sets:
        h.set_pose_priors(*sets["priors"])
    if "rel" in sets:
        h.set_relative_pose_edges(*sets["rel"])
    if "kp" in sets:
        h.set_pose_factor_robust_kernels(PRIORS, *sets["kp"])
    if "kr" in sets:
        h.set_pose_factor_robust_kernels(EDGES, *sets["kr"])
    if "lmp" in sets:
        h.set_landmark_priors(*sets["lmp"])
    if "pos" in sets:
        h.set_position_factors(*sets["pos"])
    if "dir" in sets:
        h.set_direction_factors(*sets["dir"])
    return h


def chi_squares(h):
    return {"prior": h.prior_chi_squares(), "relative_pose": h.relative_pose_chi_squares(), "landmark_prior": h.landmark_prior_chi_squares(),
            "position_factor": h.position_factor_chi_squares(), "direction_factor": h.direction_factor_chi_squares()}


def record_case(fp, precision, sets):
    out = {}
    h = handle(fp, precision, sets)
    h.set_lambda(0.0)
    h.schur()
    out["hsc"] = arr(h.hsc()[2])
    out["bp"] = arr(h.array("bp"))
    out["bsc"] = arr(h.array("bsc"))
    out["compute_errors"] = float(h.compute_errors()).hex()
    for name, chi in chi_squares(h).items():
        out[name + "_chi_squares"] = hexes(chi)
    h = handle(fp, precision, sets)
    out["optimize"] = hexes(h.optimize(10)["chi2"])
    q, t, X = h.state()
    out["q"], out["t"], out["Xw"] = arr(q), arr(t), arr(X)
    out["optimize_host_loop"] = hexes(handle(fp, precision, sets, profile=1).optimize(10)["chi2"])
    return out


def record_many_parts(precision):
    h = handle(g40(), precision, many_parts())
    out = {"compute_errors": float(h.compute_errors()).hex()}
    for name, chi in chi_squares(h).items():
        out[name + "_chi_squares"] = arr(chi)
    out["optimize"] = hexes(h.optimize(MANY_ITERATIONS)["chi2"])
    return out


def record(precision):
    out = {name: record_case(g40(), precision, sets) for name, sets in cases().items()}
    out["many_parts"] = record_many_parts(precision)
    out["shuffled60"] = {"optimize": hexes(handle(shuffled60(), precision, all_five(shuffled60())).optimize(10)["chi2"])}
    return out


if __name__ == "__main__":
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_factor_kinds.py", "hipcc_version": hipcc, "iterations": 10, "many_parts_iterations": MANY_ITERATIONS}
    for precision in PRECISIONS:
        out[precision] = record(precision)
        print(precision, out[precision]["all_five"]["optimize"][-1], out[precision]["many_parts"]["optimize"][-1],
              out[precision]["shuffled60"]["optimize"][-1], flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(out, f, indent=1)

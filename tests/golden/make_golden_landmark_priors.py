"""Generates tests/golden/landmark_priors_bits.json: the exact bits of what the solver computes with landmark position priors (the landmark
systems of both passes, the Schur complement, the objective, the per-prior chi2, LM trajectories and final states) and of the big-landmark
pass with and without priors, on the fp64 library, the fp32 library and the fp64 library with mixed_precision=1.  Doubles are stored as
float.hex() strings, arrays as the sha256 of their bytes plus their length.  tests/test_gpu_landmark_prior_bits.py recomputes every entry
through record() below and asserts equality: the fixture pins a change that must leave the results alone (a refactor of the factor code or
of the landmark passes) to the commit it was recorded at.  Needs the GPU; re-record when the toolchain changes (the fixture names the hipcc
it was built with).  Run from the repo root: `python tests/golden/make_golden_landmark_priors.py`."""
import copy
import functools
import hashlib
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
import landmark_prior_reference as lr  # noqa: E402
import robust_pose_factor_reference as rb  # noqa: E402
from conftest import RK_HUBER  # noqa: E402
from test_gpu_landmark_priors import DELTAS, main_set, small_case  # noqa: E402

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "landmark_priors_bits.json")
CONFIGS = {"f64": dict(precision="f64"), "f32": dict(precision="f32"), "f64_mixed": dict(precision="f64", mixed_precision=1)}
BIG_SEED = 4


def arr(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "len": int(a.size)}


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def handle(fp, lmp, config, **opts):
    h = HipSolver(fp, RK_HUBER, **CONFIGS[config], **opts)
    if lmp is not None:
        h.set_landmark_priors(*lmp)
    return h


def mixed_kernels(lmp):
    """the same set with the kernels none / Huber / Tukey / Cauchy in turn"""
    kind = (np.arange(len(lmp[0])) % 4).astype(np.int32)
    return lmp[:3] + (kind, np.array([DELTAS[int(k)] for k in kind]))


def lm_systems(h, lam):
    """lm_sys after build_system + assemble (mode 0), max_diagonal, and lm_sys after set_lambda + schur (mode 1)"""
    out = {}
    h.build_system()
    h.assemble()
    out["lm_sys_mode0"] = arr(h.array("lm_sys"))
    out["max_diagonal"] = float(h.max_diagonal()).hex()
    h.set_lambda(lam)
    h.schur()
    out["lm_sys_mode1"] = arr(h.array("lm_sys"))
    return out


def final_state(h, out):
    q, t, X = h.state()
    out["q"], out["t"], out["Xw"] = arr(q), arr(t), arr(X)


@functools.lru_cache(maxsize=None)
def g40():
    fp = flatten(synth_ba(40, 600, 2400, seed=1))
    lmp = mixed_kernels(main_set(fp, rb.HUBER))
    assert len(lmp[0]) != len(set(lmp[0].tolist())) and sorted(set(lmp[3].tolist())) == [0, 1, 2, 3]
    return fp, lmp


def record_g40(config):
    fp, lmp = g40()
    h = handle(fp, lmp, config)
    out = lm_systems(h, 3.7)
    out["hsc"] = arr(h.hsc()[2])
    out["bp"] = arr(h.array("bp"))
    out["bsc"] = arr(h.array("bsc"))
    out["compute_errors"] = float(h.compute_errors()).hex()
    out["landmark_prior_chi_squares"] = arr(h.landmark_prior_chi_squares())
    h = handle(fp, lmp, config)
    out["optimize"] = hexes(h.optimize(10)["chi2"])
    final_state(h, out)
    out["optimize_host_loop"] = hexes(handle(fp, lmp, config, profile=1).optimize(10)["chi2"])
    return out


def record_rejected(config):
    """small_case() of tests/test_gpu_landmark_priors.py: trials are rejected, so landmark passes that carry a restore are in the bits"""
    fp, lmp = small_case()
    h = handle(fp, lmp, config)
    chi = h.optimize(28)["chi2"]
    assert h.counters()["lm_trials"] > len(chi), (h.counters()["lm_trials"], len(chi))
    out = {"optimize": hexes(chi), "landmark_prior_chi_squares": arr(h.landmark_prior_chi_squares())}
    final_state(h, out)
    return out


@functools.lru_cache(maxsize=None)
def big_graph(seed=BIG_SEED):
    """tests/test_gpu_parity.py::graph_with_big_landmarks's construction on 600 poses: six far landmarks seen from most poses, every other
    one thinned to a third of its observations, so that the workgroup's 256-thread edge loop makes one trip for some and two for others"""
    from scipy.spatial.transform import Rotation
    g = synth_ba(600, 3000, 12000, seed=seed)
    rng = np.random.default_rng(seed + 1)
    R = Rotation.from_quat(g.truth["q"]).as_matrix()
    cam = g.pose_cam[0]
    first = int(g.lm_ids.max()) + 1
    extra_X, vp, vl, meas = [], [], [], []
    for k in range(6):
        mid = 120 + 60 * k
        c = -R[mid].T @ g.truth["t"][mid]
        X = c + R[mid].T @ np.array([rng.uniform(-20, 20), rng.uniform(-5, 5), rng.uniform(150, 250)])
        Xc = np.einsum("nij,j->ni", R, X) + g.truth["t"]
        ok = np.nonzero(Xc[:, 2] > 20)[0]
        if k % 2:
            ok = ok[::3]
        u = cam[0] * Xc[ok, 0] / Xc[ok, 2] + cam[2]; v = cam[1] * Xc[ok, 1] / Xc[ok, 2] + cam[3]
        meas.append(np.stack([u, v, u - cam[4] / Xc[ok, 2]], 1) + rng.normal(0, 1, (len(ok), 3)))
        extra_X.append(X + rng.normal(0, 0.5, 3)); vp.append(ok); vl.append(np.full(len(ok), first + k))
    g = copy.deepcopy(g)
    g.lm_ids = np.concatenate([g.lm_ids, first + np.arange(6)])
    g.lm_fixed = np.concatenate([g.lm_fixed, np.zeros(6, bool)])
    g.lm_X = np.concatenate([g.lm_X, np.array(extra_X)])
    g.stereo_vp = np.concatenate([g.stereo_vp] + vp); g.stereo_vl = np.concatenate([g.stereo_vl] + vl)
    g.stereo_meas = np.concatenate([g.stereo_meas] + meas); g.stereo_info = np.concatenate([g.stereo_info] + [np.ones(len(m)) for m in meas])
    fp = flatten(g)
    counts = np.bincount(fp.eL, minlength=fp.Lt)[:fp.Lf]
    big = np.nonzero(counts > 64)[0]
    assert ((counts > 64) & (counts <= 256)).any() and (counts > 256).any(), counts[big]
    lmp = mixed_kernels(lr.make_priors(fp, np.concatenate([big, big[:1], [0, 7, 1500]]), seed=3, kind=rb.CAUCHY, delta=2.0))
    return fp, lmp


def record_big(config):
    fp, lmp = big_graph()
    out = {}
    for name, s in (("priors", lmp), ("plain", None)):
        o = lm_systems(handle(fp, s, config), 0.9)
        h = handle(fp, s, config)
        o["optimize"] = hexes(h.optimize(5)["chi2"])
        final_state(h, o)
        out[name] = o
    return out


@functools.lru_cache(maxsize=None)
def many():
    fp = g40()[0]
    lmp = mixed_kernels(lr.make_priors(fp, np.tile(np.arange(fp.Lf), 30), seed=8, kind=rb.HUBER, delta=2.0))
    assert len(lmp[0]) > 64 * 256                     # (past the chi2 kernel's 64 workgroups of 256 threads: its grid-stride loop runs)
    return fp, lmp


def record_many(config):
    fp, lmp = many()
    h = handle(fp, lmp, config)
    return {"compute_errors": float(h.compute_errors()).hex(), "landmark_prior_chi_squares": arr(h.landmark_prior_chi_squares())}


def record(config):
    return {"g40": record_g40(config), "rejected": record_rejected(config), "big": record_big(config), "many": record_many(config)}


if __name__ == "__main__":
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_landmark_priors.py", "hipcc_version": hipcc}
    for config in CONFIGS:
        out[config] = record(config)
        print(config, out[config]["g40"]["optimize"][-1], out[config]["big"]["plain"]["optimize"][-1], flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(out, f, indent=1)

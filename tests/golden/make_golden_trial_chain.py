"""Generates tests/golden/trial_chain_bits.json: the exact bits of whole device-decided LM runs (cuba_hip_optimize) on the paths that differ
in how a trial's decision, report and restore are launched -- the single-launch trial tail (10 iterations, and 1 iteration: a run whose
only decision the host waits for), a start with rejected trials (the restore between trials; and, where one exists, a run that ENDS on a
rejected trial: at the recording none of this start's first 12 iterations on either library ended on a rejection, so the sub-case is absent), a
landmark with more than 64 observations and pose factors (the tail in several launches), and two runs in a row on one handle.  Per case
and per library (fp64, fp32): the chi2 series, the final state, the number of LM trials and the PCG iteration history.  Doubles are stored
as float.hex() strings, arrays as the sha256 of their bytes plus their length.  tests/test_gpu_trial_chain_bits.py recomputes every entry
through record() below and asserts equality: the fixture pins changes that move launches, copies, fences and host calls and must leave
every floating-point operation alone.  Needs the GPU; re-record when the toolchain changes (the fixture names the hipcc it was built
with), at a commit whose results are trusted.  Run from the repo root: `python tests/golden/make_golden_trial_chain.py`."""
import copy
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
from conftest import RK_HUBER, RK_TUKEY  # noqa: E402

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "trial_chain_bits.json")
PRECISIONS = ("f64", "f32")
TUKEY_ITERS = 12


def arr(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "len": int(a.size)}


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def _sibling(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rough_start(g, seed=1, sx=3.0, st=0.6):
    """the start of tests/test_ref_lm.py::rough_start: landmarks + N(0, sx) m, free-pose translations + N(0, st) m"""
    h = copy.deepcopy(g)
    rng = np.random.default_rng(seed)
    h.lm_X = h.lm_X + rng.normal(0, sx, h.lm_X.shape)
    free = ~h.pose_fixed
    h.pose_t = h.pose_t.copy(); h.pose_t[free] += rng.normal(0, st, (int(free.sum()), 3))
    return h


def with_big_landmark(g):
    """g plus one far landmark that every pose it lies in front of observes three times, as a stereo edge and as two monocular ones: more
    than 64 observations of one landmark on a 40-pose graph"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(5)
    R = Rotation.from_quat(g.truth["q"]).as_matrix(); t = g.truth["t"]; cam = g.pose_cam[0]
    best = None
    for mid in range(len(t)):
        X = -R[mid].T @ t[mid] + R[mid].T @ np.array([0.0, 0.0, 400.0])
        Xc = np.einsum("nij,j->ni", R, X) + t
        ok = np.nonzero(Xc[:, 2] > 20)[0]
        if best is None or len(ok) > len(best[1]):
            best = (X, ok, Xc)
    X, ok, Xc = best
    assert 3 * len(ok) > 64, len(ok)
    u = cam[0] * Xc[ok, 0] / Xc[ok, 2] + cam[2]; v = cam[1] * Xc[ok, 1] / Xc[ok, 2] + cam[3]
    m = np.stack([u, v, u - cam[4] / Xc[ok, 2]], 1)
    g = copy.deepcopy(g)
    lid = g.lm_ids.max() + 1
    g.lm_ids = np.concatenate([g.lm_ids, [lid]]); g.lm_fixed = np.concatenate([g.lm_fixed, [False]])
    g.lm_X = np.concatenate([g.lm_X, (X + rng.normal(0, 0.5, 3))[None]])
    g.stereo_vp = np.concatenate([g.stereo_vp, ok]); g.stereo_vl = np.concatenate([g.stereo_vl, np.full(len(ok), lid)])
    g.stereo_meas = np.concatenate([g.stereo_meas, m + rng.normal(0, 1, m.shape)]); g.stereo_info = np.concatenate([g.stereo_info, np.ones(len(ok))])
    for _ in range(2):
        g.mono_vp = np.concatenate([g.mono_vp, ok]); g.mono_vl = np.concatenate([g.mono_vl, np.full(len(ok), lid)])
        g.mono_meas = np.concatenate([g.mono_meas, m[:, :2] + rng.normal(0, 1, (len(ok), 2))]); g.mono_info = np.concatenate([g.mono_info, np.ones(len(ok))])
    return g


def run(h, niter):
    """one cuba_hip_optimize on the handle: everything the fixture records of it"""
    trials0 = h.counters()["lm_trials"]
    chi2 = h.optimize(niter)["chi2"]
    q, t, X = h.state()
    assert h.counter("late_decision_records") == 0
    return {"chi2": hexes(chi2), "q": arr(q), "t": arr(t), "Xw": arr(X), "lm_trials": h.counters()["lm_trials"] - trials0,
            "pcg_history": [int(v) for v in h.pcg_history()[0]]}


def tukey_graph():
    return flatten(rough_start(synth_ba(60, 1500, 6000, seed=3)))


def find_rejected_end(precision):
    """niter with which the Tukey start's run ends on a rejected trial (an iteration that leaves the objective where it was), or None:
    looked up once, when the fixture is recorded"""
    fp = tukey_graph()
    f0 = HipSolver(fp, RK_TUKEY, precision=precision).compute_errors()
    chi2 = HipSolver(fp, RK_TUKEY, precision=precision).optimize(TUKEY_ITERS)["chi2"]
    prev = f0
    for k, v in enumerate(chi2):
        if v == prev:
            return k + 1
        prev = v
    return None


def record(precision, rejected_end_niter):
    out = {}
    g40 = synth_ba(40, 600, 2400, seed=1)
    fp = flatten(g40)
    out["g40_optimize10"] = run(HipSolver(fp, RK_HUBER, precision=precision), 10)
    out["g40_optimize1"] = run(HipSolver(fp, RK_HUBER, precision=precision), 1)
    fpt = tukey_graph()
    out["tukey60"] = run(HipSolver(fpt, RK_TUKEY, precision=precision), TUKEY_ITERS)
    assert out["tukey60"]["lm_trials"] > len(out["tukey60"]["chi2"]), out["tukey60"]["lm_trials"]     # rejected trials: the restore runs
    if rejected_end_niter is not None:
        r = out["tukey60_rejected_end"] = run(HipSolver(fpt, RK_TUKEY, precision=precision), rejected_end_niter)
        assert len(r["chi2"]) == rejected_end_niter and (rejected_end_niter == 1 or r["chi2"][-1] == r["chi2"][-2])
    fpb = flatten(with_big_landmark(g40))
    assert np.bincount(fpb.eL).max() > 64
    out["big_landmark"] = run(HipSolver(fpb, RK_HUBER, precision=precision), 10)
    pri, rel = _sibling("make_golden_pose_factors").factors(fp)
    h = HipSolver(fp, RK_HUBER, precision=precision)
    h.set_pose_priors(*pri); h.set_relative_pose_edges(*rel)
    out["pose_factors"] = run(h, 10)
    h = HipSolver(fp, RK_HUBER, precision=precision)
    h.snapshot_state()
    out["two_runs_first"] = run(h, 10)
    h.restore_state()
    out["two_runs_second"] = run(h, 10)
    return out


if __name__ == "__main__":
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_trial_chain.py", "hipcc_version": hipcc}
    for precision in PRECISIONS:
        # (no niter ends the run on a rejected trial when none of the start's rejections closes an iteration: the sub-case is left out then)
        n = find_rejected_end(precision)
        out[precision] = {"rejected_end_niter": n, "runs": record(precision, n)}
        print(precision, "rejected_end_niter", n, {k: (len(v["chi2"]), v["lm_trials"]) for k, v in out[precision]["runs"].items()}, flush=True)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1)

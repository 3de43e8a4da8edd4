"""The triangulation reference (tests/triangulation_reference.py) on the CPU: against its own 60-digit twin, against the truth, and the
properties the GPU tests rely on.

D, the largest |X_np - X_mp|_inf / max(1, |X_mp|_inf) between the fp64 reference and the 60-digit model over a set of landmarks, is what
tests/test_gpu_triangulation.py scales its position bound with (8 D, measured there on the same landmarks).  Measured here: 9.9e-16 on the
zoo (well-conditioned: up to 257 views), 9.5e-15 on the first 100 landmarks of the small graph at the true poses (two to ten views, depths
up to 40 m; 10 iterations)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import triangulation_reference as T  # noqa: E402

from conftest import RK_HUBER, RK_TUKEY  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402


@pytest.fixture(scope="module")
def true_graph():
    from cuba_amd.synth import synth_ba
    return synth_ba(40, 600, 2400, seed=1, perturb=False)


@pytest.fixture(scope="module")
def true_fp(true_graph):
    return flatten(true_graph)


@pytest.fixture(scope="module")
def zoo():
    return T.zoo_problem()


@pytest.fixture(scope="module")
def zoo_ref(zoo):
    fp, idx, select, edge_mask = zoo
    return T.triangulate(fp, select=select, refine_iterations=5, rk=RK_HUBER, omega=np.where(edge_mask, fp.omega, 0.0))


def test_the_figures_of_the_small_graph(true_fp, small_fp):
    """the definition as prototyped: 488 OK without refinement, 487 / 3 / 2 / 108 with 2 to 10 steps, and steps that converge"""
    r0 = T.triangulate(true_fp, refine_iterations=0, rk=RK_HUBER)
    assert r0["counts"]["ok"] == 488 and sum(r0["counts"].values()) == true_fp.Lt
    r10 = T.triangulate(true_fp, refine_iterations=10, rk=RK_HUBER)
    for it in (2, 5):
        r = T.triangulate(true_fp, refine_iterations=it, rk=RK_HUBER)
        assert (r["counts"]["ok"], r["counts"]["low_parallax"], r["counts"]["behind_camera"], r["counts"]["chi2"]) == (487, 3, 2, 108)
        assert np.array_equal(r["status"], r10["status"])
    assert T.threshold_margin(r10).min() == pytest.approx(6.2e-6, rel=0.01) and T.determinant_margin(r10).min() > 1e-5
    # the largest move of an accepted landmark in step k (metres): the Gauss-Newton step as signed converges (a landmark with an outlier
    # among two or three views, rejected as CHI2 or BEHIND_CAMERA in the end, may wander)
    ok = [s for l, s in enumerate(r10["steps"]) if r10["status"][l] == T.OK]
    move = lambda k: max(float(np.abs(np.subtract(s["iterates"][k], s["iterates"][k - 1])).max()) for s in ok)  # noqa: E731
    assert move(2) == pytest.approx(1.8, rel=0.05) and move(3) == pytest.approx(0.10, rel=0.1) and move(4) == pytest.approx(1e-3, rel=0.2)
    assert move(6) < 1.8e-5 and move(10) < 4.5e-9
    # from the perturbed start (0.5 degrees / 5 cm of pose noise) most landmarks end as CHI2
    p = T.triangulate(small_fp, refine_iterations=5, rk=RK_HUBER)
    assert p["counts"]["chi2"] == 545 and p["counts"]["ok"] == 47 and T.threshold_margin(p).min() > 1e-6


def test_against_the_60_digit_twin(true_fp, zoo, zoo_ref):
    fp, idx, select, edge_mask = zoo
    omega = np.where(edge_mask, fp.omega, 0.0)
    D, st = T.model_distance(fp, zoo_ref, range(fp.Lt), 5, RK_HUBER, omega=omega)
    print(f"\n[triangulation reference] zoo: D = {D:.2e}")
    # (the overflowing pose is finite in 60 digits: there the twin goes on where fp64 stops)
    assert all(s == zoo_ref["status"][l] for l, s in st.items() if l != idx["overflow"]) and st[idx["overflow"]] != T.SINGULAR
    assert D < 1e-13
    for rk, name in ((RK_HUBER, "huber"), (RK_TUKEY, "tukey")):
        ref = T.triangulate(true_fp, refine_iterations=10, rk=rk, landmarks=range(100))
        D, st = T.model_distance(true_fp, ref, range(100), 10, rk)
        sure = T.determinant_margin(ref) > 1e-6
        print(f"[triangulation reference] small graph, 100 landmarks, 10 iterations, {name}: D = {D:.2e}, determinants in the noise: {(~sure).sum()}")
        assert all(s == ref["status"][l] for l, s in st.items() if sure[l]) and len(st) > 90
        assert D < 1e-11


def test_noise_free_measurements_recover_the_true_points(true_graph, true_fp):
    """measurements replaced by the exact projections of the true points at the true poses"""
    import copy
    fp = copy.copy(true_fp)
    X = true_graph.truth["Xw"][fp.lm_src]
    meas = fp.meas.copy()
    for e in range(fp.E):
        R = T.quat_to_rot(fp.q[fp.eP[e]])
        Xc = R @ X[fp.eL[e]] + fp.t[fp.eP[e]]
        fx, fy, cx, cy, bf = fp.cam[fp.eP[e]]
        u = fx * Xc[0] / Xc[2] + cx
        meas[e] = (u, fy * Xc[1] / Xc[2] + cy, u - bf / Xc[2] if fp.eDim[e] == 3 else 0.0)
    fp.meas = meas
    for it in (0, 3):
        r = T.triangulate(fp, state=(fp.q, fp.t, np.full_like(fp.Xw, np.nan)), refine_iterations=it, rk=RK_HUBER, min_parallax_deg=0.0)
        assert r["counts"]["ok"] == fp.Lt
        err = T.position_distance(r["xyz"], X)
        print(f"\n[triangulation reference] noise-free, {it} iterations: largest error {err.max():.2e}")
        assert err.max() < 1e-7


def test_the_robust_gradient_vanishes_after_ten_iterations(true_fp):
    """on every accepted landmark (measured: 2.2e-12 of the sum of its terms' sizes)"""
    r = T.triangulate(true_fp, refine_iterations=10, rk=RK_HUBER)
    worst = 0.0
    for l, s in enumerate(r["steps"]):
        if s is None or r["status"][l] != T.OK:
            continue
        # h against the size of its terms: sum |w' JL^T r| is of the order fx / z * |r| per edge
        eds = [T._edge(true_fp, (true_fp.q, true_fp.t, true_fp.Xw), true_fp.omega, e, T.Arith) for e in r["active"][l]]
        scale = sum(max(abs(v) for v in T._gn_terms(ed, s["X"], RK_HUBER, T.Arith)[1]) for ed in eds)
        worst = max(worst, max(abs(v) for v in s["h"]) / max(scale, 1e-300))
    print(f"\n[triangulation reference] largest |h| / sum |terms| after 10 iterations: {worst:.2e}")
    assert worst < 1e-9


def test_every_status_occurs_in_the_zoo(zoo, zoo_ref):
    fp, idx, select, edge_mask = zoo
    want = dict(one_stereo=T.OK, no_disparity=T.FEW_OBSERVATIONS, parallel=T.LOW_PARALLAX, behind=T.BEHIND_CAMERA, overflow=T.SINGULAR, outlier=T.CHI2,
                fixed=T.FIXED, gated=T.FEW_OBSERVATIONS, fill0=T.NOT_SELECTED, **{f"n{n}": T.OK for n in T.ZOO_COUNTS})
    assert {k: int(zoo_ref["status"][idx[k]]) for k in want} == want
    assert all(v > 0 for v in zoo_ref["counts"].values()) and sum(zoo_ref["counts"].values()) == fp.Lt
    assert [int(np.bincount(fp.eL)[idx[f"n{n}"]]) for n in T.ZOO_COUNTS] == list(T.ZOO_COUNTS) and fp.Pt == 301
    assert T.threshold_margin(zoo_ref).min() > 1e-6 and T.determinant_margin(zoo_ref).min() > 1e-6
    # OK landmarks lie near the truth (0.5 px of noise), every other one keeps the state's position
    ok = zoo_ref["status"] == T.OK
    assert np.abs(zoo_ref["xyz"][ok] - fp.Xw[ok]).max() < 0.1 and np.array_equal(zoo_ref["xyz"][~ok], fp.Xw[~ok])
    # without the parallax test the parallel rays' matrix has the determinant 0 exactly
    r = T.triangulate(fp, refine_iterations=0, min_parallax_deg=0.0, landmarks=[idx["parallel"]])
    assert r["status"][idx["parallel"]] == T.SINGULAR and T.determinant_margin(r)[idx["parallel"]] == np.inf


def test_the_float_rounded_problem_decides_alike(true_fp):
    """what the fp32 library's reference is: the same definition on float-rounded inputs"""
    f, _ = T.float_rounded(true_fp)
    a = T.triangulate(true_fp, refine_iterations=5, rk=RK_HUBER)
    b = T.triangulate(f, refine_iterations=5, rk=T.float_rounded_kernels(RK_HUBER))
    assert T.threshold_margin(b).min() > 1e-6 and (a["status"] != b["status"]).sum() <= 2
    assert np.abs(a["xyz"] - b["xyz"]).max() < 1e-2

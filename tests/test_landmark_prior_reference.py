"""CPU checks of the landmark position priors: the numpy model of tests/landmark_prior_reference.py (which the GPU tests hold the library
to) against central differences, the behaviour of the dense LM on the shapes the GPU tests use, and what exists without a GPU: the C-ABI
symbols and the Python methods."""
import ctypes
import os
import re

import numpy as np
import pytest

import landmark_prior_reference as lr
import robust_pose_factor_reference as rb
from conftest import ROOT, RK_HUBER, with_fixed
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle.oracle import OracleSolver

KINDS = (rb.NONE, rb.HUBER, rb.TUKEY, rb.CAUCHY)
DELTAS = {rb.NONE: 1.0, rb.HUBER: 2.0, rb.TUKEY: 6.0, rb.CAUCHY: 2.0}


def main_set(fp, kind):
    """the set of the GPU tests: 75 priors on random free landmarks, one landmark taken twice"""
    rng = np.random.default_rng(5)
    lms = rng.choice(fp.Lf, 74, replace=False)
    lms = np.concatenate([lms, lms[:1]])
    return lr.make_priors(fp, lms, seed=6, kind=None if kind == rb.NONE else kind, delta=DELTAS[kind])


@pytest.fixture(scope="module")
def fp40():
    return flatten(synth_ba(40, 600, 2400, seed=1))


@pytest.mark.parametrize("kind", KINDS)
def test_weight_is_the_derivative_of_rho_on_a_prior(fp40, kind):
    """rho'(e) of the model's per-prior (e, rho, w) against central differences of rho along the prior's own residual, on both sides of
    delta^2: the residual is scaled so that e = x delta^2"""
    delta = DELTAS[kind]
    lmp = lr.make_priors(fp40, [3], seed=1, kind=kind, delta=delta)
    # (Xbar at the origin: X - Xbar then carries no rounding of its own, which at |X| ~ 50, |r| ~ 0.01 would cost the difference quotient 1e-8)
    lmp = (lmp[0], np.zeros((1, 3)), lmp[2], lmp[3], lmp[4])
    X = np.asarray(fp40.Xw, dtype=np.float64).reshape(-1, 3).copy()
    X[3] = [0.3, -0.2, 0.1]
    e0, _, _, l, Om, r0 = lr.prior_terms(lmp, X, fp40.Lf)[0]
    for x in (1e-3, 0.2, 0.7, 0.95, 1.05, 1.6, 5.0, 40.0):
        s = np.sqrt(x * delta * delta / e0)

        def at(scale):
            Y = X.copy()
            Y[l] = lmp[1][0] + scale * r0
            return lr.prior_terms(lmp, Y, fp40.Lf)[0]

        e, _, w, _, _, _ = at(s)
        assert abs(e - x * delta * delta) <= 1e-12 * e
        # d rho / d e by a step in the scale: e(s) = s^2 e0, so h_e = e ((1 + h)^2 - (1 - h)^2) = 4 h e
        h = 2.5e-5
        num = (at(s * (1 + h))[1] - at(s * (1 - h))[1]) / (4 * h * e)
        print("kind %d e / delta^2 %g: w %.12g, central difference %.12g" % (kind, x, w, num))
        # (step 1e-4 e in e: truncation and rounding as in test_robust_pose_factor_reference, <= 5e-9)
        assert abs(w - num) <= 1e-8


@pytest.mark.parametrize("kind", KINDS)
def test_b_is_minus_half_the_gradient_of_the_objective(fp40, kind):
    """-2 b of the priors' dense system against central differences of sum rho(e) over the landmark coordinates"""
    lmp = main_set(fp40, kind)
    X = np.asarray(fp40.Xw, dtype=np.float64).reshape(-1, 3).copy()
    _, b = lr.prior_system(lmp, X, fp40.Pf, fp40.Lf)
    assert not b[:6 * fp40.Pf].any()
    e = lr.prior_chi2(lmp, X, fp40.Lf)
    d2 = DELTAS[kind] ** 2
    if kind != rb.NONE:
        assert (e < d2).any() and (e > d2).any()                  # priors on both sides of delta^2
    scale = np.abs(b).max()
    for l in np.unique(lmp[0])[:12]:
        for c in range(3):
            h = 1e-6
            Xp, Xm = X.copy(), X.copy()
            Xp[l, c] += h; Xm[l, c] -= h
            num = (lr.prior_objective(lmp, Xp, fp40.Lf) - lr.prior_objective(lmp, Xm, fp40.Lf)) / (2 * h)
            # (rho is C^1, piecewise smooth: truncation h^2 |rho'''| ~ 1e-12 * 1e3, rounding eps F / h ~ 1e-16 * 1e4 / 1e-6 = 1e-6)
            assert abs(-2 * b[6 * fp40.Pf + 3 * l + c] - num) <= 1e-7 * scale


def test_prior_on_a_fixed_landmark_has_no_term():
    fp = flatten(with_fixed(synth_ba(40, 600, 2400, seed=1), fixed_lm_rows=[5, 9]))
    assert fp.Lt - fp.Lf == 2
    lmp = lr.make_priors(fp, [2, fp.Lt - 1], seed=2)
    X = np.asarray(fp.Xw, dtype=np.float64).reshape(-1, 3)
    e = lr.prior_chi2(lmp, X, fp.Lf)
    assert e[0] > 0 and e[1] == 0.0
    H, b = lr.prior_system(lmp, X, fp.Pf, fp.Lf)
    assert np.count_nonzero(b) == 3


@pytest.mark.parametrize("kind", KINDS)
def test_dense_lm_descends_on_the_main_set(fp40, kind):
    """the set-up of the GPU parity tests: at the start e spans both sides of delta^2, 10 iterations without a rejected trial and a
    strictly decreasing objective"""
    lmp = main_set(fp40, kind)
    o = OracleSolver(fp40, RK_HUBER)
    res = lr.dense_lm(o, fp40, lmp, 10)
    print("kind %d: chi2 %s rejected %d" % (kind, res["chi2"], res["rejected"]))
    assert len(res["chi2"]) == 10 and res["rejected"] == 0
    assert np.all(np.diff(res["chi2"]) < 0)


def test_leaving_the_weight_out_of_hll_is_seen():
    """what the 1e-6 bar of the GPU parity tests separates: Omega instead of w Omega in Hll (the gradient kept right) moves the
    per-iteration objective by more than 1e-4 relative"""
    fp = flatten(synth_ba(40, 600, 2400, seed=1))
    lmp = main_set(fp, rb.HUBER)
    ref = lr.dense_lm(OracleSolver(fp, RK_HUBER), fp, lmp, 6)["chi2"]
    saved = lr.landmark_blocks

    def wrong(lmp_, X, Lf):
        H, g = saved(lmp_, X, Lf)
        H2, _ = saved((lmp_[0], lmp_[1], lmp_[2], None, None), X, Lf)
        return H2, g

    lr.landmark_blocks = wrong
    try:
        bad = lr.dense_lm(OracleSolver(fp, RK_HUBER), fp, lmp, 6)["chi2"]
    finally:
        lr.landmark_blocks = saved
    n = min(len(ref), len(bad))
    assert np.abs(bad[:n] - ref[:n]).max() / ref[0] > 1e-4


def test_library_exports_the_landmark_prior_symbols():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    capi.build_library()
    for name in ("cuba_hip_set_landmark_priors", "cuba_hip_landmark_prior_chi_squares"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
        for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {path}"
    assert hasattr(capi.HipSolver, "set_landmark_priors") and hasattr(capi.HipSolver, "landmark_prior_chi_squares")

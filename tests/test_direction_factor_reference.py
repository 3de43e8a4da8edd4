"""CPU checks of the direction factors on the poses: the numpy model of tests/direction_factor_reference.py (which the GPU tests hold the
library to) against central differences through the oracle's pose update, its robust kernels, the behaviour of the dense LM on the shapes
the GPU tests use (the body-frame Jacobian -R [d]x included: the mistake the GPU bars are sized against), the gauge of two position fixes
plus one direction, and what exists without a GPU: the sample, the C-ABI symbols and the Python methods."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import direction_factor_reference as dr
import position_factor_reference as pfr
import robust_pose_factor_reference as rb
from conftest import ROOT, RK_HUBER
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle import oracle
from oracle.oracle import OracleSolver

KINDS = (rb.NONE, rb.HUBER, rb.TUKEY, rb.CAUCHY)
DELTAS = {rb.NONE: 1.0, rb.HUBER: 2.0, rb.TUKEY: 6.0, rb.CAUCHY: 2.0}
HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")


def with_kernel(s, kind):
    n = len(s[0])
    return s[:4] + ((None, None) if kind == rb.NONE else (np.full(n, kind, dtype=np.int32), np.full(n, DELTAS[kind])))


def main_set(fp, kind=rb.NONE):
    """the set of the GPU tests: 14 random free poses, pose 5 twice and the fixed pose (flatten puts it last)"""
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.choice(fp.Pf, 14, replace=False), [5, 5, fp.Pt - 1]])
    return with_kernel(dr.make_factors(fp, poses, seed=6), kind)


def free_graph(g):
    g = copy.deepcopy(g)
    g.pose_fixed[:] = False
    return flatten(g)


def reduced_matrix(H, Pf):
    n = 6 * Pf
    return H[:n, :n] - H[:n, n:] @ np.linalg.solve(H[n:, n:], H[n:, :n])


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


@pytest.fixture(scope="module")
def fp40(g40):
    return flatten(g40)


def test_jacobian_is_the_derivative_through_the_pose_update(fp40):
    """dr/ddelta = [-[R d]x | 0] against central differences of r along T <- exp(delta) T (oracle.pose_update), entry by entry, h = 1e-6,
    50 random cases; the body-frame form -R [d]x is off by about 2"""
    rng = np.random.default_rng(3)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    worst, worst_body, h = 0.0, 0.0, 1e-6
    for _ in range(50):
        p = int(rng.integers(fp40.Pt))
        d, m = rng.normal(size=3), rng.normal(size=3)
        d /= np.linalg.norm(d)
        J, Jb = dr.jacobian(q0[p], d), dr.jacobian(q0[p], d, body_frame=True)
        for c in range(6):
            x = np.zeros(6); x[c] = h
            qp, _ = oracle.pose_update(x, q0[p], t0[p])
            qm, _ = oracle.pose_update(-x, q0[p], t0[p])
            num = (dr.residual(qp, d, m) - dr.residual(qm, d, m)) / (2 * h)
            worst = max(worst, np.abs(num - J[:, c]).max())
            worst_body = max(worst_body, np.abs(num - Jb[:, c]).max())
        assert not J[:, 3:].any()
    print("worst entry of J against central differences: %.3g (bar 1e-8); the body-frame form: %.3g" % (worst, worst_body))
    # (truncation h^2 |d| / 6 ~ 2e-13, rounding eps |r| / h ~ 1e-16 * 2 / 1e-6 = 2e-10)
    assert worst <= 1e-8
    assert worst_body >= 0.5


@pytest.mark.parametrize("kind", KINDS)
def test_rho_and_weight_are_those_of_the_pose_factors(fp40, kind):
    """(under Tukey three times the main set's noise: e then spans both sides of delta^2 = 36 too)"""
    s = with_kernel(dr.make_factors(fp40, main_set(fp40)[0], seed=6, sigma=0.15 if kind == rb.TUKEY else 0.05), kind)
    q0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4)
    terms = dr.factor_terms(s, q0, fp40.Pf)
    e = np.array([x[0] for x in terms])
    d2 = DELTAS[kind] ** 2
    if kind != rb.NONE:
        assert (e[e > 0] < d2).any() and (e > d2).any()               # factors on both sides of delta^2
    for ek, rho, w, p, J, Om, r in terms:
        if p >= fp40.Pf:
            assert (ek, rho, w) == (0.0, 0.0, 0.0) and J is None
            continue
        assert ek == float(r @ Om @ r)
        assert rho == rb.rho(kind, DELTAS[kind], ek) and w == rb.weight(kind, DELTAS[kind], ek)


@pytest.mark.parametrize("kind", KINDS)
def test_b_is_minus_half_the_gradient_of_the_objective(fp40, kind):
    """-2 b of the factors' dense system against central differences of sum rho(e) along the pose update"""
    s = main_set(fp40, kind)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    _, b = dr.factor_system(s, q0, fp40.Pf)
    scale, h = np.abs(b).max(), 1e-6
    for p in np.unique(s[0][s[0] < fp40.Pf])[:8]:
        for c in range(6):
            d = np.zeros(6); d[c] = h
            F = []
            for sign in (1.0, -1.0):
                q = q0.copy()
                q[p], _ = oracle.pose_update(sign * d, q0[p], t0[p])
                F.append(dr.factor_objective(s, q, fp40.Pf))
            num = (F[0] - F[1]) / (2 * h)
            # (rho is C^1, piecewise smooth: rounding eps F / h ~ 1e-16 * 50 / 1e-6 = 5e-9 against |b| ~ 50)
            assert abs(-2 * b[6 * p + c] - num) <= 1e-7 * scale
            if c >= 3:
                assert b[6 * p + c] == 0.0 and num == 0.0


def test_factor_on_a_fixed_pose_has_no_term(fp40):
    s = dr.make_factors(fp40, [2, fp40.Pt - 1], seed=2)
    q0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4)
    e = dr.factor_chi2(s, q0, fp40.Pf)
    assert e[0] > 0 and e[1] == 0.0
    H, b = dr.factor_system(s, q0, fp40.Pf)
    assert np.count_nonzero(b) == 3 and np.count_nonzero(H) == 9


def test_rank2_information_has_the_measurement_in_its_null_space(fp40):
    s = dr.make_factors(fp40, [3, 9], seed=2, rank2=True)
    for k in range(2):
        assert np.abs(s[3][k] @ s[2][k]).max() <= 1e-12 * np.abs(s[3][k]).max()
        assert np.linalg.matrix_rank(s[3][k], tol=1e-9 * np.abs(s[3][k]).max()) == 2


@pytest.mark.parametrize("kind", KINDS)
def test_dense_lm_descends_on_the_main_set(fp40, kind):
    """the set-up of the GPU parity tests: 10 iterations without a rejected trial and a strictly decreasing objective; at the start the
    factors' e sum to 43.6 with a maximum of 7.6, so Huber (delta^2 = 4) and Cauchy engage"""
    s = main_set(fp40, kind)
    e = dr.factor_chi2(s, np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), fp40.Pf)
    res = dr.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, s, 10)
    print("kind %d: start e sum %.4g max %.4g, chi2 %s rejected %d" % (kind, e.sum(), e.max(), res["chi2"], res["rejected"]))
    assert e.max() > 4.0
    assert len(res["chi2"]) == 10 and res["rejected"] == 0
    assert np.all(np.diff(res["chi2"]) < 0)


@pytest.mark.parametrize("kind", KINDS)
def test_the_body_frame_jacobian_stalls_the_dense_lm(kind):
    """what the 1e-6 bar of the GPU optimality test separates (its shape): synth_ba(12, 96, 400, seed=1), a factor on every free pose plus
    the fixed pose, make_factors(seed=7), 80 iterations allowed.  With the right Jacobian the dense LM ends below 1e-7 of the start
    gradient, with -R [d]x in the system it stalls above 1e-5.  Measured with this model (none / Huber / Tukey / Cauchy): right
    1.1e-9 / 1.0e-11 / 2.6e-10 / 1.1e-10, body-frame 4.0e-4 / 3.8e-4 / 3.3e-4 / 2.6e-4; the factors' e end at a sum of about 15 and a
    maximum of about 5.7: a genuinely non-zero residual."""
    fp = flatten(synth_ba(12, 96, 400, seed=1))
    s = with_kernel(dr.make_factors(fp, list(range(fp.Pf)) + [fp.Pt - 1], seed=7), kind)
    out = []
    for body in (False, True):
        o = OracleSolver(fp, RK_HUBER)
        g0 = np.linalg.norm(dr.gradient(o, fp, s))
        dr.dense_lm(o, fp, s, 80, body_frame=body)
        out.append(np.linalg.norm(dr.gradient(o, fp, s)) / g0)
        if not body:
            e = dr.factor_chi2(s, o.state()[0], fp.Pf)
    print("kind %d: gradient / start: right Jacobian %.3g, body-frame %.3g; factor chi2 sum %.4g max %.4g" % (kind, out[0], out[1], e.sum(), e.max()))
    assert out[0] <= 1e-7 and out[1] >= 1e-5
    assert e.max() > 1e-3


def test_two_fixes_leave_one_gauge_direction_that_a_direction_factor_closes(g40):
    """every vertex free, position fixes on poses 2 and 37: the reduced matrix has one null direction, the rotation about the line
    through the fixes (measured -4.5e-11 of a largest eigenvalue 1.9e7); one direction factor on pose 20 closes it (0.45)"""
    fp = free_graph(g40)
    assert fp.Pf == fp.Pt and fp.Lf == fp.Lt
    fixes = pfr.make_factors(fp, [2, 37], seed=4, sigma=0.05, arm=0.0)
    one = dr.make_factors(fp, [20], seed=8)
    o = OracleSolver(fp, RK_HUBER)
    ev0 = np.linalg.eigvalsh(reduced_matrix(dr.system(o, fp, None, 0.0, pf=fixes)[0], fp.Pf))
    ev1 = np.linalg.eigvalsh(reduced_matrix(dr.system(o, fp, one, 0.0, pf=fixes)[0], fp.Pf))
    print("smallest eigenvalues: two fixes %.3g %.3g, with the direction factor %.3g; largest %.3g" % (ev0[0], ev0[1], ev1[0], ev1[-1]))
    assert abs(ev0[0]) <= 1e-6 and ev0[1] >= 1e-4
    assert ev1[0] >= 0.1


def test_gravity_aligned_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/gravity_aligned"])
    sample = os.path.join(HOST, "samples", "gravity_aligned")
    assert os.access(sample, os.X_OK)
    out = subprocess.run([sample], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout


def test_library_exports_the_direction_factor_symbols():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    capi.build_library()
    for name in ("cuba_hip_set_direction_factors", "cuba_hip_direction_factor_chi_squares"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
        for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {path}"
    assert hasattr(capi.HipSolver, "set_direction_factors") and hasattr(capi.HipSolver, "direction_factor_chi_squares")

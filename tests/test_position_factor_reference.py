"""CPU checks of the position factors on the poses: the numpy model of tests/position_factor_reference.py (which the GPU tests hold the
library to) against central differences through the oracle's pose update, its robust kernels, the behaviour of the dense LM on the shapes
the GPU tests use, and what exists without a GPU: the sample, the C-ABI symbols and the Python methods."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import position_factor_reference as pf
import robust_pose_factor_reference as rb
from conftest import ROOT, RK_HUBER, with_fixed
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


def main_set(fp, kind):
    """the set of the GPU tests: 14 random free poses, pose 5 twice and the fixed pose"""
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.choice(fp.Pf, 14, replace=False), [5, 5, fp.Pt - 1]])
    return with_kernel(pf.make_factors(fp, poses, seed=6), kind)


@pytest.fixture(scope="module")
def fp40():
    return flatten(synth_ba(40, 600, 2400, seed=1))


def test_jacobian_is_the_derivative_through_the_pose_update(fp40):
    """dr/dd = [R^T [a]x | -R^T] against central differences of r along T <- exp(d) T (oracle.pose_update), entry by entry"""
    s = pf.make_factors(fp40, [0, 7, 7, 21, 38], seed=3, arm=0.8)
    s[3][1] = 0.0                                   # a zero lever arm: the rotation column vanishes
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    worst, h = 0.0, 1e-5
    for k, p in enumerate(s[0]):
        J = pf.jacobian(q0[p], s[3][k])
        for c in range(6):
            d = np.zeros(6); d[c] = h
            qp, tp = oracle.pose_update(d, q0[p], t0[p])
            qm, tm = oracle.pose_update(-d, q0[p], t0[p])
            num = (pf.residual(qp, tp, s[3][k], s[1][k]) - pf.residual(qm, tm, s[3][k], s[1][k])) / (2 * h)
            worst = max(worst, np.abs(num - J[:, c]).max())
    print("worst entry of J against central differences: %.3g (bar 1e-8)" % worst)
    # (truncation h^2 |r'''| / 6 ~ 1e-10 * |a - t| ~ 1e-9 at most, rounding eps |r| / h ~ 1e-16 * 50 / 1e-5 = 5e-10)
    assert worst <= 1e-8
    assert not pf.jacobian(q0[7], s[3][1])[:, :3].any()


@pytest.mark.parametrize("kind", KINDS)
def test_rho_and_weight_are_those_of_the_pose_factors(fp40, kind):
    """(under Tukey the main set's poses with three times its noise: e then spans both sides of delta^2 = 36 too)"""
    s = with_kernel(pf.make_factors(fp40, main_set(fp40, rb.NONE)[0], seed=6, sigma=0.6 if kind == rb.TUKEY else 0.2), kind)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    terms = pf.factor_terms(s, q0, t0, fp40.Pf)
    e = np.array([x[0] for x in terms])
    d2 = DELTAS[kind] ** 2
    if kind != rb.NONE:
        assert (e[e > 0] < d2).any() and (e > d2).any()               # factors on both sides of delta^2
    for k, (ek, rho, w, p, J, Om, r) in enumerate(terms):
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
    _, b = pf.factor_system(s, q0, t0, fp40.Pf)
    scale, h = np.abs(b).max(), 1e-6
    for p in np.unique(s[0][s[0] < fp40.Pf])[:8]:
        for c in range(6):
            d = np.zeros(6); d[c] = h
            F = []
            for sign in (1.0, -1.0):
                q, t = q0.copy(), t0.copy()
                q[p], t[p] = oracle.pose_update(sign * d, q0[p], t0[p])
                F.append(pf.factor_objective(s, q, t, fp40.Pf))
            num = (F[0] - F[1]) / (2 * h)
            # (rho is C^1, piecewise smooth: rounding eps F / h ~ 1e-16 * 1e2 / 1e-6 = 1e-8 against |b| ~ 1e2)
            assert abs(-2 * b[6 * p + c] - num) <= 1e-7 * scale


def test_factor_on_a_fixed_pose_has_no_term(fp40):
    s = pf.make_factors(fp40, [2, fp40.Pt - 1], seed=2)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    e = pf.factor_chi2(s, q0, t0, fp40.Pf)
    assert e[0] > 0 and e[1] == 0.0
    H, b = pf.factor_system(s, q0, t0, fp40.Pf)
    assert np.count_nonzero(b) == 6


@pytest.mark.parametrize("kind", KINDS)
def test_dense_lm_descends_on_the_main_set(fp40, kind):
    """the set-up of the GPU parity tests: 10 iterations without a rejected trial and a strictly decreasing objective"""
    res = pf.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, main_set(fp40, kind), 10)
    print("kind %d: chi2 %s rejected %d" % (kind, res["chi2"], res["rejected"]))
    assert len(res["chi2"]) == 10 and res["rejected"] == 0
    assert np.all(np.diff(res["chi2"]) < 0)


def test_dropping_the_rotation_column_stalls_the_dense_lm():
    """what the 1e-6 bar of the GPU optimality test separates (its shape, no kernel): with the right Jacobian the dense LM ends below 1e-9
    of the start gradient, with J = [0 | -R^T] in the system it stalls above 1e-5"""
    fp = flatten(synth_ba(12, 96, 400, seed=1))
    s = pf.make_factors(fp, list(range(fp.Pf)) + [fp.Pt - 1], seed=7)
    out = []
    for rc in (True, False):
        o = OracleSolver(fp, RK_HUBER)
        g0 = np.linalg.norm(pf.gradient(o, fp, s))
        pf.dense_lm(o, fp, s, 40, rotation_column=rc)
        out.append(np.linalg.norm(pf.gradient(o, fp, s)) / g0)
    print("gradient / start: right Jacobian %.3g, without the rotation column %.3g" % tuple(out))
    assert out[0] <= 1e-9 and out[1] >= 1e-5


def test_gnss_positions_sample_builds_and_prints_its_usage():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/gnss_positions"])
    sample = os.path.join(HOST, "samples", "gnss_positions")
    assert os.access(sample, os.X_OK)
    out = subprocess.run([sample], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout


def test_library_exports_the_position_factor_symbols():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    capi.build_library()
    for name in ("cuba_hip_set_position_factors", "cuba_hip_position_factor_chi_squares"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
        for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {path}"
    assert hasattr(capi.HipSolver, "set_position_factors") and hasattr(capi.HipSolver, "position_factor_chi_squares")

"""CPU checks of the range factors on the poses: the numpy model of tests/range_factor_reference.py (which the GPU tests hold the library
to) against central differences through the oracle's own pose update (prior_reference.apply_step), the rule at rho = 0, its robust
kernels, factors on fixed poses, the gauge and scale that four non-coplanar anchors heard from three poses give a graph without a fixed
vertex, the sizing of the GPU optimality case (both wrong Jacobians included: the mistakes the GPU bar is sized against), and what exists
without a GPU: the C-ABI symbols and the Python methods."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import prior_reference as pr
import range_factor_reference as rr
import robust_pose_factor_reference as rb
from conftest import ROOT, RK_HUBER
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle import oracle
from oracle.oracle import OracleSolver

KINDS = (rb.NONE, rb.HUBER, rb.TUKEY, rb.CAUCHY)
DELTAS = {rb.NONE: 1.0, rb.HUBER: 2.0, rb.TUKEY: 6.0, rb.CAUCHY: 2.0}
WRONG = (rr.WORLD_DIRECTION, rr.NO_ROTATION)

# the optimality case of the GPU tests (tests/test_gpu_range_factors.py): the shape, the set and the bar on the gradient
OPT_SHAPE = (12, 96, 400)
OPT_SET = dict(seed=8, sigma=0.5, span=3.0, arm=0.5)
OPT_ITERATIONS = 120
GRADIENT_BAR = 1e-6


def with_kernel(s, kind):
    n = len(s[0])
    return s[:5] + ((None, None) if kind == rb.NONE else (np.full(n, kind, dtype=np.int32), np.full(n, DELTAS[kind])))


def main_set(fp, kind=rb.NONE):
    """the set of the GPU tests: 14 random free poses, pose 5 twice and the fixed pose (flatten puts it last)"""
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.choice(fp.Pf, 14, replace=False), [5, 5, fp.Pt - 1]])
    return with_kernel(rr.make_factors(fp, poses, seed=6), kind)


def optimality_case(kind):
    fp = flatten(synth_ba(*OPT_SHAPE, seed=1))
    return fp, with_kernel(rr.make_factors(fp, list(range(fp.Pf)) + [fp.Pt - 1], **OPT_SET), kind)


def free_graph(g):
    g = copy.deepcopy(g)
    g.pose_fixed[:] = False
    return flatten(g)


def gauge_set(fp):
    """four non-coplanar anchors, each heard from poses 2, 20 and 37 (twelve ranges)"""
    s = rr.make_factors(fp, [2] * 4 + [20] * 4 + [37] * 4, seed=4, sigma=0.02)
    A = s[1][:4]
    assert abs(np.linalg.det(A[1:] - A[0])) > 1.0          # non-coplanar: the tetrahedron has a volume
    return s


def reduced_matrix(H, Pf):
    n = 6 * Pf
    return H[:n, :n] - H[:n, n:] @ np.linalg.solve(H[n:, n:], H[n:, :n])


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


@pytest.fixture(scope="module")
def fp40(g40):
    return flatten(g40)


def test_jacobian_is_the_derivative_through_the_pose_update():
    """dr/dd = [(m x a)^T | -m^T] against central differences of the model's residual along the oracle's own update of all free poses
    (prior_reference.apply_step), entry by entry, h = 1e-6, on 6 poses x 8 draws of anchor and arm.  The two wrong forms -- the
    world-frame direction R^T m for m, no rotation columns -- are off by tenths"""
    fp = flatten(synth_ba(*OPT_SHAPE, seed=1))
    o = OracleSolver(fp, RK_HUBER)
    q0, t0, X0 = (x.copy() for x in o.state())
    rng = np.random.default_rng(3)
    worst, wrong, h = 0.0, {v: 0.0 for v in WRONG}, 1e-6
    for _ in range(8):
        b = 5.0 * rng.normal(size=(fp.Pf, 3))
        a = 0.5 * rng.normal(size=(fp.Pf, 3))
        J = {v: np.array([rr.jacobian(q0[p], t0[p], a[p], b[p], v) for p in range(fp.Pf)]) for v in (rr.RIGHT,) + WRONG}
        for c in range(6):
            r = []
            for sign in (1.0, -1.0):
                x = np.zeros(6 * fp.Pf + 3 * fp.Lf)
                x[c:6 * fp.Pf:6] = sign * h
                o.set_state(q0, t0, X0)
                pr.apply_step(o, fp, x)
                q, t, _ = o.state()
                r.append(np.array([rr.residual(q[p], t[p], a[p], b[p], 0.0) for p in range(fp.Pf)]))
            num = (r[0] - r[1]) / (2 * h)
            worst = max(worst, np.abs(num - J[rr.RIGHT][:, c]).max())
            for v in WRONG:
                wrong[v] = max(wrong[v], np.abs(num - J[v][:, c]).max())
    print("worst entry of J against central differences: %.3g (bar 1e-8); world-frame direction: %.3g, no rotation columns: %.3g"
          % (worst, wrong[rr.WORLD_DIRECTION], wrong[rr.NO_ROTATION]))
    # (truncation h^2 |d^3 rho| / 6 ~ 1e-12 / rho^2, rounding eps rho / h ~ 1e-16 * 10 / 1e-6 = 1e-9)
    assert worst <= 1e-8
    assert min(wrong.values()) >= 0.1


def test_a_zero_arm_has_no_rotation_columns_only_then():
    q, t, b = np.array([0.1, -0.2, 0.3, 0.9]) / np.linalg.norm([0.1, -0.2, 0.3, 0.9]), np.array([0.3, -1.0, 2.0]), np.array([4.0, 1.0, -2.0])
    assert not rr.jacobian(q, t, np.zeros(3), b)[:3].any()
    assert np.abs(rr.jacobian(q, t, np.array([0.2, 0.1, -0.4]), b)[:3]).max() > 0.1
    assert abs(np.linalg.norm(rr.jacobian(q, t, np.zeros(3), b)[3:]) - 1) <= 1e-15


def test_the_point_rho_zero_has_a_zero_jacobian_and_keeps_its_residual():
    """identity rotation, b = 0, a = t: u is exactly 0, so m = 0, J = 0, the factor adds nothing to H or b and e = Omega rbar^2"""
    q, t = np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.25, -1.5, 3.0])
    rho, m = rr.direction(q, t, t, np.zeros(3))
    assert rho == 0.0 and not m.any()
    for v in (rr.RIGHT,) + WRONG:
        assert not rr.jacobian(q, t, t, np.zeros(3), v).any()
    s = (np.array([0]), np.zeros((1, 3)), np.array([0.75]), np.array([16.0]), t[None], None, None)
    (e, rho_k, w, p, J, Om, r), = rr.factor_terms(s, q[None], t[None], 1)
    assert e == 16.0 * 0.75 ** 2 and rho_k == e and w == 1.0 and r == -0.75
    H, b = rr.factor_system(s, q[None], t[None], 1)
    assert np.isfinite(H).all() and not H.any() and not b.any()


@pytest.mark.parametrize("kind", KINDS)
def test_rho_and_weight_are_those_of_the_pose_factors(fp40, kind):
    """(under Tukey four times the main set's noise: e then spans both sides of delta^2 = 36 too)"""
    s = with_kernel(rr.make_factors(fp40, main_set(fp40)[0], seed=6, sigma=0.4 if kind == rb.TUKEY else 0.1), kind)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    terms = rr.factor_terms(s, q0, t0, fp40.Pf)
    e = np.array([x[0] for x in terms])
    d2 = DELTAS[kind] ** 2
    if kind != rb.NONE:
        assert (e[e > 0] < d2).any() and (e > d2).any()               # factors on both sides of delta^2
    for ek, rho, w, p, J, Om, r in terms:
        if p >= fp40.Pf:
            assert (ek, rho, w) == (0.0, 0.0, 0.0) and J is None
            continue
        assert ek == Om * r * r
        assert rho == rb.rho(kind, DELTAS[kind], ek) and w == rb.weight(kind, DELTAS[kind], ek)


@pytest.mark.parametrize("kind", KINDS)
def test_b_is_minus_half_the_gradient_of_the_objective(fp40, kind):
    """-2 b of the factors' dense system against central differences of sum rho_k(e) along the pose update"""
    s = main_set(fp40, kind)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    _, b = rr.factor_system(s, q0, t0, fp40.Pf)
    scale, h = np.abs(b).max(), 1e-6
    for p in np.unique(s[0][s[0] < fp40.Pf])[:8]:
        for c in range(6):
            d = np.zeros(6); d[c] = h
            F = []
            for sign in (1.0, -1.0):
                q, t = q0.copy(), t0.copy()
                q[p], t[p] = oracle.pose_update(sign * d, q0[p], t0[p])
                F.append(rr.factor_objective(s, q, t, fp40.Pf))
            num = (F[0] - F[1]) / (2 * h)
            # (rho_k is C^1, piecewise smooth: rounding eps F / h ~ 1e-16 * 50 / 1e-6 = 5e-9 against |b| ~ 50)
            assert abs(-2 * b[6 * p + c] - num) <= 1e-7 * scale


def test_factor_on_a_fixed_pose_has_no_term(fp40):
    s = rr.make_factors(fp40, [2, fp40.Pt - 1], seed=2)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    e = rr.factor_chi2(s, q0, t0, fp40.Pf)
    assert e[0] > 0 and e[1] == 0.0
    H, b = rr.factor_system(s, q0, t0, fp40.Pf)
    assert np.count_nonzero(b) == 6 and np.count_nonzero(H) == 36
    assert np.linalg.matrix_rank(H) == 1                               # (one factor: a rank-1 term)


@pytest.mark.parametrize("kind", KINDS)
def test_dense_lm_descends_on_the_main_set(fp40, kind):
    """the set-up of the GPU parity tests: 10 iterations without a rejected trial and a strictly decreasing objective; Huber
    (delta^2 = 4) and Cauchy engage at the start"""
    s = main_set(fp40, kind)
    q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
    e = rr.factor_chi2(s, q0, t0, fp40.Pf)
    res = rr.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, s, 10)
    print("kind %d: start e sum %.4g max %.4g, chi2 %s rejected %d" % (kind, e.sum(), e.max(), res["chi2"], res["rejected"]))
    assert e.max() > 4.0
    assert len(res["chi2"]) == 10 and res["rejected"] == 0
    assert np.all(np.diff(res["chi2"]) < 0)


def test_four_anchors_heard_from_three_poses_give_gauge_and_scale(g40):
    """every vertex free: the dense lambda = 0 Hessian of the reprojection edges alone has the gauge's null directions (at least six
    eigenvalues within rounding of zero); twelve ranges -- four non-coplanar anchors x poses 2, 20, 37 -- give it full rank"""
    fp = free_graph(g40)
    assert fp.Pf == fp.Pt and fp.Lf == fp.Lt
    s = gauge_set(fp)
    o = OracleSolver(fp, RK_HUBER)
    ev0 = np.linalg.eigvalsh(rr.system(o, fp, None, 0.0)[0])
    H1 = rr.system(o, fp, s, 0.0)[0]
    ev1 = np.linalg.eigvalsh(H1)
    print("smallest eigenvalues: plain %s, with the ranges %.3g; largest %.3g" % (ev0[:8], ev1[0], ev1[-1]))
    assert np.abs(ev0[:6]).max() <= 1e-9 * ev0[-1]
    assert ev1[0] >= 1e-3 and ev1[0] >= 1e6 * np.abs(ev0[:6]).max()
    assert np.linalg.matrix_rank(H1, tol=1e-12 * ev1[-1]) == H1.shape[0]


@pytest.mark.parametrize("kind", KINDS)
def test_the_optimality_case_separates_the_right_jacobian_from_the_wrong_ones(kind):
    """what the 1e-6 bar of the GPU optimality test separates (its shape): synth_ba(12, 96, 400, seed=1), a factor on every free pose plus
    the fixed pose, make_factors(seed=8, sigma=0.5, span=3, arm=0.5): ranges of 0.7 ... 8.8 m, half a metre of noise and of arm, 120
    iterations allowed.  With the right Jacobian the dense LM ends at least a decade below the bar, with either wrong one it stalls at
    least a decade above it.  Measured with this model (none / Huber / Tukey / Cauchy): right 1.4e-9 / 5.4e-11 / 4.6e-9 / 5.7e-12,
    world-frame direction 5.2e-4 / 2.8e-4 / 2.2e-4 / 1.2e-4, no rotation columns 3.3e-4 / 2.3e-4 / 1.5e-5 / 1.1e-4.  The run has
    genuinely rejected trials (gain ratio below -1e-3, the first at trial 15 / 7 / 10 / 16, long before rounding decides anything), and the
    factors' e end at a sum of 61 ... 536: a genuinely non-zero residual."""
    fp, s = optimality_case(kind)
    assert s[2].min() > 0.5 and s[2].max() < 10.0
    out = {}
    for v in (rr.RIGHT,) + WRONG:
        o = OracleSolver(fp, RK_HUBER)
        g0 = np.linalg.norm(rr.gradient(o, fp, s))
        res = rr.dense_lm(o, fp, s, OPT_ITERATIONS, variant=v)
        out[v] = np.linalg.norm(rr.gradient(o, fp, s)) / g0
        if v == rr.RIGHT:
            e = rr.factor_chi2(s, *o.state()[:2], fp.Pf)
            genuine = [i for i, x in enumerate(res["gains"]) if x < -1e-3]
    print("kind %d: gradient / start: right %.3g, world-frame direction %.3g, no rotation columns %.3g; first genuinely rejected trial %s of "
          "%d; factor chi2 sum %.4g max %.4g" % (kind, out[rr.RIGHT], out[rr.WORLD_DIRECTION], out[rr.NO_ROTATION], genuine[:1], len(genuine),
                                                 e.sum(), e.max()))
    assert out[rr.RIGHT] <= 0.1 * GRADIENT_BAR
    assert min(out[v] for v in WRONG) >= 10 * GRADIENT_BAR
    assert genuine and genuine[0] < 20
    assert e.max() > 1e-3


def test_library_exports_the_range_factor_symbols():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    capi.build_library()
    for name in ("cuba_hip_set_range_factors", "cuba_hip_range_factor_chi_squares"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
        for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {path}"
    assert hasattr(capi.HipSolver, "set_range_factors") and hasattr(capi.HipSolver, "range_factor_chi_squares")

"""CPU checks of the range factors between two poses: the numpy model of tests/pose_range_factor_reference.py (which the GPU tests hold
the library to) against central differences through the oracle's own pose update, the symmetry under swapping the two ends, the rule at
rho = 0, fixed ends, the scale that odometer distances give a monocular graph with one fixed pose, the sizing of the GPU optimality case
(the three wrong Jacobians included: the mistakes the GPU bar is sized against), and what exists without a GPU: the C-ABI symbols and the
Python methods."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import pose_range_factor_reference as pp
import robust_pose_factor_reference as rb
from conftest import ROOT, RK_HUBER
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle import oracle
from oracle.oracle import OracleSolver
from test_range_factor_reference import DELTAS, GRADIENT_BAR, KINDS, OPT_ITERATIONS, OPT_SHAPE

WRONG = (pp.WORLD_DIRECTION, pp.NO_ROTATION, pp.WRONG_SIGN)

# the optimality case of the GPU tests (tests/test_gpu_pose_range_factors.py): the set on synth_ba(*OPT_SHAPE, seed=1)
OPT_SET = dict(seed=8, sigma=0.5, arm=0.5)


def with_kernel(s, kind):
    n = len(s[0])
    return s[:6] + ((None, None) if kind == rb.NONE else (np.full(n, kind, dtype=np.int32), np.full(n, DELTAS[kind])))


def main_pairs(fp):
    """the pairs of the GPU tests' main set: 12 random free-free pairs, the block (3, 9) three times -- once as (9, 3) --, pose 5 in three
    more factors, and one factor with a fixed end in either seat (flatten puts the fixed pose last)"""
    rng = np.random.default_rng(5)
    pairs = [tuple(rng.choice(fp.Pf, 2, replace=False)) for _ in range(12)]
    return np.array(pairs + [(3, 9), (9, 3), (3, 9), (5, 1), (2, 5), (5, 30), (fp.Pt - 1, 7), (8, fp.Pt - 1)], dtype=np.int32)


def main_set(fp, kind=rb.NONE):
    return with_kernel(pp.make_factors(fp, main_pairs(fp), seed=6), kind)


def optimality_pairs(fp):
    """every consecutive pair of free poses (an odometer), every pose with the one four on, and the last free pose with the fixed one"""
    P = fp.Pf
    return np.array([(k, k + 1) for k in range(P - 1)] + [(k + 4, k) for k in range(P - 4)] + [(P - 1, fp.Pt - 1)], dtype=np.int32)


def optimality_case(kind):
    fp = flatten(synth_ba(*OPT_SHAPE, seed=1))
    return fp, with_kernel(pp.make_factors(fp, optimality_pairs(fp), **OPT_SET), kind)


def monocular(g):
    """the graph with every stereo edge as a monocular one (u, v), behind the monocular edges; the fixed flags stay"""
    return dataclasses.replace(g, mono_vp=np.concatenate([g.mono_vp, g.stereo_vp]), mono_vl=np.concatenate([g.mono_vl, g.stereo_vl]),
                               mono_meas=np.concatenate([np.asarray(g.mono_meas).reshape(-1, 2), np.asarray(g.stereo_meas).reshape(-1, 3)[:, :2]]),
                               mono_info=np.concatenate([g.mono_info, g.stereo_info]), stereo_vp=g.stereo_vp[:0], stereo_vl=g.stereo_vl[:0],
                               stereo_meas=np.asarray(g.stereo_meas).reshape(-1, 3)[:0], stereo_info=g.stereo_info[:0])


# the scale case of the GPU tests: a monocular graph with one fixed pose and an odometer factor on every SCALE_STRIDE-th consecutive pair
SCALE_SHAPE = (12, 96, 400)
SCALE_STRIDE = 1
SCALE_INFO = 1e4


def scale_case():
    fp = flatten(monocular(synth_ba(*SCALE_SHAPE, seed=2)))
    assert fp.Pt - fp.Pf == 1
    pairs = np.array([(k, k + 1) for k in range(0, fp.Pf - 1, SCALE_STRIDE)] + [(fp.Pf - 1, fp.Pt - 1)], dtype=np.int32)
    return fp, pp.make_factors(fp, pairs, seed=4, sigma=0.01, info=SCALE_INFO)


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


@pytest.fixture(scope="module")
def fp40(g40):
    return flatten(g40)


def state0(fp):
    return np.asarray(fp.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp.t, dtype=np.float64).reshape(-1, 3)


def test_jacobians_are_the_derivatives_through_the_pose_update(fp40):
    """J_i and J_j against central differences of the model's residual along the oracle's own update T <- exp(d) T of either end, entry by
    entry, h = 1e-6, on the 20 factors of the main set (arms of 0.3 m, distances of metres).  The three wrong forms are off by tenths"""
    s = main_set(fp40)
    q0, t0 = state0(fp40)
    worst, wrong, h = 0.0, {v: 0.0 for v in WRONG}, 1e-6
    for k in range(len(s[0])):
        i, j = int(s[0][k]), int(s[1][k])
        ai, aj = pp.arms_of(s, k)
        J = {v: np.concatenate(pp.jacobians(q0[i], t0[i], q0[j], t0[j], ai, aj, v)) for v in (pp.RIGHT,) + WRONG}
        num = np.zeros(12)
        for end in range(2):
            for c in range(6):
                r = []
                for sign in (1.0, -1.0):
                    d = np.zeros(6); d[c] = sign * h
                    q, t = q0.copy(), t0.copy()
                    p = (i, j)[end]
                    q[p], t[p] = oracle.pose_update(d, q0[p], t0[p])
                    r.append(pp.residual(q[i], t[i], q[j], t[j], ai, aj, 0.0))
                num[6 * end + c] = (r[0] - r[1]) / (2 * h)
        worst = max(worst, np.abs(num - J[pp.RIGHT]).max())
        for v in WRONG:
            wrong[v] = max(wrong[v], np.abs(num - J[v]).max())
    print("worst entry of J against central differences: %.3g (bar 1e-8); world-frame directions: %.3g, no rotation columns: %.3g, m_i with the "
          "wrong sign: %.3g" % (worst, wrong[pp.WORLD_DIRECTION], wrong[pp.NO_ROTATION], wrong[pp.WRONG_SIGN]))
    # (truncation h^2 |d^3 rho| / 6 ~ 1e-12 / rho^2, rounding eps rho / h ~ 1e-16 * 10 / 1e-6 = 1e-9)
    assert worst <= 1e-8
    assert min(wrong.values()) >= 0.1


@pytest.mark.parametrize("kind", KINDS)
def test_swapping_the_ends_with_their_arms_changes_nothing(fp40, kind):
    """(i, a_i) <-> (j, a_j): the distance is that of the same two world points, so e is unchanged to rounding and H, b -- already indexed
    by pose, hence 'permuted' -- are the same system"""
    s = main_set(fp40, kind)
    swapped = (s[1], s[0], s[2], s[3], s[5], s[4], s[6], s[7])
    q0, t0 = state0(fp40)
    e, es = pp.factor_chi2(s, q0, t0, fp40.Pf), pp.factor_chi2(swapped, q0, t0, fp40.Pf)
    # (rho is computed in frame j or in frame i: the same length to a few ulp of the coordinates, 1e-15 * 10 m, against r ~ 0.05 m)
    assert np.abs(e - es).max() <= 1e-11 * e.max()
    (H, b), (Hs, bs) = pp.factor_system(s, q0, t0, fp40.Pf), pp.factor_system(swapped, q0, t0, fp40.Pf)
    assert np.abs(H - Hs).max() <= 1e-11 * np.abs(H).max() and np.abs(b - bs).max() <= 1e-11 * np.abs(b).max()
    # (J[a] (w J[b]) against J[b] (w J[a]): an ulp of the entry)
    assert np.abs(H - H.T).max() <= 4 * np.finfo(np.float64).eps * np.abs(H).max()


def test_the_point_rho_zero_has_zero_jacobians_and_keeps_its_residual():
    """identity rotations, a_i - t_i = a_j - t_j exactly: u is exactly 0, so m_i = m_j = 0, both J = 0, the factor adds nothing to H or b
    and e = Omega rbar^2"""
    q = np.array([[0.0, 0.0, 0.0, 1.0]] * 2)
    t = np.array([[0.25, -1.5, 3.0], [1.25, 0.5, -1.0]])
    ai, aj = np.array([0.5, 0.25, 1.0]), np.array([1.5, 2.25, -3.0])
    assert ((ai - t[0]) == (aj - t[1])).all()
    rho, mi, mj = pp.directions(q[0], t[0], q[1], t[1], ai, aj)
    assert rho == 0.0 and not mi.any() and not mj.any()
    for v in (pp.RIGHT,) + WRONG:
        Ji, Jj = pp.jacobians(q[0], t[0], q[1], t[1], ai, aj, v)
        assert not Ji.any() and not Jj.any()
    s = (np.array([0]), np.array([1]), np.array([0.75]), np.array([16.0]), ai[None], aj[None], None, None)
    (e, rho_k, w, i, j, Ji, Jj, Om, r), = pp.factor_terms(s, q, t, 2)
    assert e == 16.0 * 0.75 ** 2 and rho_k == e and w == 1.0 and r == -0.75
    H, b = pp.factor_system(s, q, t, 2)
    assert np.isfinite(H).all() and not H.any() and not b.any()


@pytest.mark.parametrize("kind", KINDS)
def test_b_is_minus_half_the_gradient_of_the_objective(fp40, kind):
    """-2 b of the factors' dense system against central differences of sum rho_k(e) along the pose update"""
    s = main_set(fp40, kind)
    q0, t0 = state0(fp40)
    _, b = pp.factor_system(s, q0, t0, fp40.Pf)
    scale, h = np.abs(b).max(), 1e-6
    for p in (3, 9, 5, 7, 8):
        for c in range(6):
            d = np.zeros(6); d[c] = h
            F = []
            for sign in (1.0, -1.0):
                q, t = q0.copy(), t0.copy()
                q[p], t[p] = oracle.pose_update(sign * d, q0[p], t0[p])
                F.append(pp.factor_objective(s, q, t, fp40.Pf))
            num = (F[0] - F[1]) / (2 * h)
            assert abs(-2 * b[6 * p + c] - num) <= 1e-7 * scale


def test_fixed_ends(fp40):
    """one end fixed: the unary range factor on the free end with the fixed end's point as the anchor (a rank-1 diagonal term, no
    off-diagonal one); both fixed: nothing, e = 0 -- on a graph with two fixed poses"""
    import range_factor_reference as rr
    g = synth_ba(40, 600, 2400, seed=1)
    g.pose_fixed[:2] = True
    fp = flatten(g)
    assert fp.Pt - fp.Pf == 2
    F0, F1 = fp.Pt - 2, fp.Pt - 1
    s = pp.make_factors(fp, [(2, F0), (F1, 4), (F0, F1), (2, 4)], seed=2)
    q0, t0 = state0(fp)
    e = pp.factor_chi2(s, q0, t0, fp.Pf)
    assert (e[[0, 1, 3]] > 0).all() and e[2] == 0.0
    H, b = pp.factor_system(tuple(x[:3] if x is not None else None for x in s), q0, t0, fp.Pf)
    assert np.count_nonzero(b) == 12 and np.count_nonzero(H) == 72 and np.linalg.matrix_rank(H) == 2
    # factor 0 as a unary range factor on pose 2: anchor = the world point of the fixed end
    unary = (s[0][:1], rr.antenna(fp, F0, s[5][0])[None], s[2][:1], s[3][:1], s[4][:1], None, None)
    Hu, bu = rr.factor_system(unary, q0, t0, fp.Pf)
    H0, b0 = pp.factor_system(tuple(x[:1] if x is not None else None for x in s), q0, t0, fp.Pf)
    assert np.abs(H0 - Hu).max() <= 1e-12 * np.abs(Hu).max() and np.abs(b0 - bu).max() <= 1e-10 * np.abs(bu).max()
    # the free-free factor: two rank-1 diagonal terms and the off-diagonal block J_2^T w Omega J_4, rank 1 in all
    H3, _ = pp.factor_system(tuple(x[3:] if x is not None else None for x in s), q0, t0, fp.Pf)
    assert np.count_nonzero(H3) == 144 and np.linalg.matrix_rank(H3) == 1 and np.abs(H3[12:18, 24:30]).max() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_dense_lm_descends_on_the_main_set(fp40, kind):
    """the set-up of the GPU parity tests: 10 iterations without a rejected trial and a strictly decreasing objective"""
    s = main_set(fp40, kind)
    q0, t0 = state0(fp40)
    e = pp.factor_chi2(s, q0, t0, fp40.Pf)
    res = pp.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, s, 10)
    print("kind %d: start e sum %.4g max %.4g, chi2 %s rejected %d" % (kind, e.sum(), e.max(), res["chi2"], res["rejected"]))
    assert len(res["chi2"]) == 10 and res["rejected"] == 0
    assert np.all(np.diff(res["chi2"]) < 0)


def inverse_error(H, Pf, Lf):
    """the error of np.linalg.inv(H) itself, by one step of refinement in extended precision: Hi (I - H Hi) block by block (the poses'
    6 x 6 and the landmarks' 3 x 3 diagonal blocks), relative to the block of Hi's largest entry -- the measure of the GPU covariance tests"""
    Hi = np.linalg.inv(H)
    Hl, Hil = H.astype(np.longdouble), Hi.astype(np.longdouble)
    C = (Hil @ (np.eye(len(H), dtype=np.longdouble) - Hl @ Hil)).astype(np.float64)
    blocks = [slice(6 * p, 6 * p + 6) for p in range(Pf)] + [slice(6 * Pf + 3 * l, 6 * Pf + 3 * l + 3) for l in range(Lf)]
    return max(np.abs(C[b, b]).max() / np.abs(Hi[b, b]).max() for b in blocks)


def test_odometer_distances_give_a_monocular_graph_its_scale():
    """the scale case of the GPU tests: synth_ba(12, 96, 400, seed=2) read as a monocular graph, one fixed pose, an odometer factor on every
    consecutive pair and on the last free pose with the fixed one, sigma 0.01 m, information 1e4 ... 2e4.  The dense lambda = 0 Hessian of
    the reprojection edges alone has the scale's null direction (one eigenvalue within rounding of zero, the next 2.4e-3); the odometer
    factors give it full rank.  Its condition number stays 5.0e9 -- the weakest landmark direction, 2.3e-3, against the rotations' 1.1e7 --
    whatever the factors' information, so eps * cond = 1e-6 says nothing about the 1e-9 of the GPU covariance test; what the dense inverse
    itself reaches is measured by one step of refinement in extended precision: 4.8e-12 of a block's largest entry at this information
    (1.7e-10 ... 4.5e-10 at information 1e6 on the seed-1 graph: too close to the bar, hence this set).  Bar here: a decade below 1e-9."""
    fp, s = scale_case()
    o = OracleSolver(fp, RK_HUBER)
    ev0 = np.linalg.eigvalsh(pp.system(o, fp, None, 0.0)[0])
    H1 = pp.system(o, fp, s, 0.0)[0]
    ev1 = np.linalg.eigvalsh(H1)
    err = inverse_error(H1, fp.Pf, fp.Lf)
    print("smallest eigenvalues: plain %s, with the odometer %.3g; largest %.3g; condition %.3g; the dense inverse's own error %.3g"
          % (ev0[:3], ev1[0], ev1[-1], ev1[-1] / ev1[0], err))
    assert abs(ev0[0]) <= 1e-9 * ev0[-1] and ev0[1] > 1e3 * abs(ev0[0])
    assert ev1[0] >= 1e6 * abs(ev0[0])
    assert err <= 1e-10


@pytest.mark.parametrize("kind", KINDS)
def test_the_optimality_case_separates_the_right_jacobian_from_the_wrong_ones(kind):
    """what the 1e-6 bar of the GPU optimality test separates (its shape): synth_ba(12, 96, 400, seed=1), optimality_pairs (an odometer chain,
    every pose with the one four on, the last free pose with the fixed one), make_factors(seed=8, sigma=0.5, arm=0.5): half a metre of noise
    and of arm, 120 iterations allowed.  With the right Jacobians the dense LM ends at least a decade below the bar, with any wrong form it
    stalls at least a decade above it.  Measured with this model (none / Huber / Tukey / Cauchy): right 7.8e-12 / 2.5e-11 / 7.7e-13 /
    2.2e-11, world-frame directions 1.7e-3 / 4.3e-4 / 1.2e-4 / 1.5e-4, no rotation columns 7.4e-4 / 2.4e-4 / 4.3e-5 / 7.5e-5, m_i with the
    wrong sign 2.1e-3 / 5.9e-4 / 1.6e-4 / 1.9e-4.  The run has genuinely rejected trials (gain ratio below -1e-3, the first at trial 10,
    long before rounding decides anything; distances of 1.0 ... 4.0 m), and the factors' e end at a sum of 306 ... 315: a genuinely
    non-zero residual."""
    fp, s = optimality_case(kind)
    out = {}
    for v in (pp.RIGHT,) + WRONG:
        o = OracleSolver(fp, RK_HUBER)
        g0 = np.linalg.norm(pp.gradient(o, fp, s))
        res = pp.dense_lm(o, fp, s, OPT_ITERATIONS, variant=v)
        out[v] = np.linalg.norm(pp.gradient(o, fp, s)) / g0
        if v == pp.RIGHT:
            e = pp.factor_chi2(s, *o.state()[:2], fp.Pf)
            genuine = [i for i, x in enumerate(res["gains"]) if x < -1e-3]
    print("kind %d: gradient / start: right %.3g, world-frame directions %.3g, no rotation columns %.3g, m_i with the wrong sign %.3g; first "
          "genuinely rejected trial %s of %d; factor chi2 sum %.4g max %.4g"
          % (kind, out[pp.RIGHT], out[pp.WORLD_DIRECTION], out[pp.NO_ROTATION], out[pp.WRONG_SIGN], genuine[:1], len(genuine), e.sum(), e.max()))
    assert out[pp.RIGHT] <= 0.1 * GRADIENT_BAR
    assert min(out[v] for v in WRONG) >= 10 * GRADIENT_BAR
    assert genuine and genuine[0] < 20
    assert e.max() > 1e-3


def test_library_exports_the_pose_range_factor_symbols():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    capi.build_library()
    for name in ("cuba_hip_set_pose_range_factors", "cuba_hip_pose_range_factor_chi_squares"):
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
        for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {path}"
    assert hasattr(capi.HipSolver, "set_pose_range_factors") and hasattr(capi.HipSolver, "pose_range_factor_chi_squares")

"""CPU checks of the SE(3) pose-prior maths of tests/prior_reference.py (the model the GPU tests hold the library to): log against the
oracle's exponential, the closed-form inverse left Jacobian against central differences under the oracle's pose update, and the dense
LM loop of the helper against the oracle's own loop."""
import numpy as np
import pytest

import prior_reference as pr
from conftest import RK_HUBER, RK_NONE
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle import oracle
from oracle.oracle import OracleSolver

ANGLES = (0.0, 1e-9, 1e-6, 1e-3, 0.5, 2.0, 3.1)


def _tangent(theta, seed):
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return np.concatenate([theta * ax, rng.normal(size=3)])


@pytest.mark.parametrize("theta", ANGLES)
def test_log_inverts_the_oracle_exponential(theta):
    r = _tangent(theta, 1)
    q, t = oracle.se3_exp(r)
    assert np.abs(pr.se3_log(q, t) - r).max() <= 1e-12 * max(1.0, np.abs(r).max())
    # the same through the pose update from the identity, and the prior residual of exp(r) against the identity
    q2, t2 = oracle.pose_update(r, [0, 0, 0, 1], [0, 0, 0])
    assert np.abs(pr.prior_residual(q2, t2, [0, 0, 0, 1], [0, 0, 0]) - r).max() <= 1e-12 * max(1.0, np.abs(r).max())


@pytest.mark.parametrize("theta", ANGLES)
def test_inverse_left_jacobian_is_the_residual_derivative(theta):
    r = _tangent(theta, 2)
    # a prior pose away from the identity: T = exp(r) Tbar
    qb, tb = oracle.se3_exp(_tangent(0.7, 3))
    qe, te = oracle.se3_exp(r)
    q = pr.quat_mul(qe, qb)
    t = oracle.quat_to_rot(qe) @ tb + te
    assert np.abs(pr.prior_residual(q, t, qb, tb) - r).max() <= 1e-11
    J = pr.se3_jl_inv(r)
    h = 1e-6
    Jn = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        qp, tp = oracle.pose_update(d, q, t)
        qm, tm = oracle.pose_update(-d, q, t)
        Jn[:, k] = (pr.prior_residual(qp, tp, qb, tb) - pr.prior_residual(qm, tm, qb, tb)) / (2 * h)
    assert np.abs(J - Jn).max() <= 1e-7 * np.abs(J).max()
    assert np.abs(J @ pr.se3_jl(r) - np.eye(6)).max() <= 1e-12


def test_dense_lm_without_priors_is_the_oracle_loop():
    fp = flatten(synth_ba(12, 150, 500, seed=4))
    ref = OracleSolver(fp, RK_HUBER).optimize(6)
    got = pr.dense_lm(OracleSolver(fp, RK_HUBER), fp, None, 6)
    assert len(got["chi2"]) == len(ref["chi2"])
    assert np.abs(got["chi2"] - ref["chi2"]).max() <= 1e-12 * ref["chi2"].max()


def test_dense_lm_with_priors_reaches_a_stationary_point():
    fp = flatten(synth_ba(12, 150, 500, seed=4))
    o = OracleSolver(fp, RK_NONE)          # (without a robust kernel Gauss-Newton converges fast enough to test stationarity)
    q, t, _ = o.state()
    rng = np.random.default_rng(5)
    poses = np.arange(0, fp.Pf, 3)
    qb, tb = [], []
    for p in poses:
        dq, dt = oracle.se3_exp(np.concatenate([0.05 * rng.normal(size=3), 0.2 * rng.normal(size=3)]))
        qb.append(pr.quat_mul(dq, q[p]))
        tb.append(oracle.quat_to_rot(dq) @ t[p] + dt)
    info = np.array([np.diag([4e4, 4e4, 4e4, 1e3, 1e3, 1e3])] * len(poses))
    priors = (poses, np.array(qb), np.array(tb), info)
    g0 = np.linalg.norm(pr.gradient(o, fp, priors))
    res = pr.dense_lm(o, fp, priors, 30)
    assert np.all(np.diff(res["chi2"]) <= 0)
    q, t, _ = o.state()
    assert pr.prior_chi2(priors, q, t, fp.Pf).sum() > 1e-3          # the optimum sits at a non-zero prior residual
    assert np.linalg.norm(pr.gradient(o, fp, priors)) <= 1e-6 * g0

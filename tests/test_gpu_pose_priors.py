"""SE(3) pose priors (cuba_hip_set_pose_priors / HipSolver.set_pose_priors) on the GPU against the numpy model of
tests/prior_reference.py: the assembled system, the objective, LM trajectories against a dense fp64 LM, optimality at a non-zero prior
residual, special prior sets, covariances, batches, the handle's life cycle, the refusals and the other builds."""
import copy

import numpy as np
import pytest

import prior_reference as pr
from conftest import RK_HUBER, RK_NONE, RK_TUKEY, with_fixed
from test_gpu_configs import dense_normal_equations, shuffled_pose_ids

from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba, synth_named
from oracle import oracle
from oracle.oracle import OracleSolver

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6


def freed(g, rows=(0,)):
    h = copy.deepcopy(g)
    h.pose_fixed[list(rows)] = False
    return h


def make_priors(fp, poses, seed=0, rot=0.05, trans=0.2, w_rot=4e4, w_trans=1e3, corr=True):
    """priors a few degrees / decimetres off the current estimate, with information that conflicts with the observations"""
    rng = np.random.default_rng(seed)
    q0, t0 = np.asarray(fp.q).reshape(-1, 4), np.asarray(fp.t).reshape(-1, 3)
    poses = np.asarray(poses, dtype=np.int32)
    qb, tb, info = [], [], []
    for p in poses:
        dq, dt = oracle.se3_exp(np.concatenate([rot * rng.normal(size=3), trans * rng.normal(size=3)]))
        qb.append(pr.quat_mul(dq, q0[p]))
        tb.append(oracle.quat_to_rot(dq) @ t0[p] + dt)
        O = np.diag([w_rot] * 3 + [w_trans] * 3)
        if corr:
            A = rng.normal(size=(6, 6)) * 0.1
            O = O + np.sqrt(w_rot * w_trans) * (A @ A.T) * 0.01
        info.append(O)
    return poses, np.array(qb), np.array(tb), np.array(info)


def solver(fp, rk, priors=None, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if priors is not None:
        h.set_pose_priors(*priors)
    return h


def dense_run(fp, rk, priors, niter):
    return pr.dense_lm(OracleSolver(fp, rk), fp, priors, niter)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


# ---- assembly and objective ----------------------------------------------------------------------------------------------------------
def test_assembled_system_is_the_plain_one_plus_the_prior_terms(g40):
    fp = flatten(g40)
    pri = make_priors(fp, [1, 5, 5, 17, fp.Pf - 1, fp.Pt - 1], seed=1)       # two on pose 5, one on the fixed pose (flatten puts it last)
    plain, withp = solver(fp, RK_HUBER), solver(fp, RK_HUBER, pri)
    for h in (plain, withp):
        h.set_lambda(0.0)
        h.schur()
    rp, ci, v0 = plain.hsc()
    _, _, v1 = withp.hsc()
    q, t, _ = withp.state()
    Hp, bp = pr.prior_system(pri, q, t, fp.Pf)
    diag = rp[:-1]
    off = np.setdiff1d(np.arange(len(ci)), diag)
    assert np.array_equal(v0[off], v1[off])
    for p in range(fp.Pf):
        want = v0[diag[p]] + Hp[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        up = np.triu_indices(6)
        assert np.abs(v1[diag[p]][up] - want[up]).max() <= 1e-12 * np.abs(want[up]).max()
    for name in ("bp", "bsc"):
        a0, a1 = plain.array(name), withp.array(name)
        want = a0 + bp
        assert np.abs(a1 - want).max() <= 1e-12 * np.abs(want).max()


def test_objective_and_prior_chi_squares(g40):
    fp = flatten(g40)
    pri = make_priors(fp, [2, 9, fp.Pt - 1, 30], seed=2)
    plain, withp = solver(fp, RK_HUBER), solver(fp, RK_HUBER, pri)
    q, t, _ = withp.state()
    want = pr.prior_chi2(pri, q, t, fp.Pf)
    got = withp.prior_chi_squares()
    assert got[2] == 0.0 and want[2] == 0.0                      # the prior on the fixed pose is ignored
    assert np.abs(got - want).max() <= 1e-10 * want.max()
    assert abs(withp.compute_errors() - (plain.compute_errors() + want.sum())) <= 1e-12 * withp.compute_errors()
    # lambda_0 includes the priors: the maximum diagonal is that of Hpp + priors
    assert withp.max_diagonal() >= plain.max_diagonal()


# ---- LM parity against the dense reference -----------------------------------------------------------------------------------------
CASES = {
    "huber": (RK_HUBER, {}),
    "none": (RK_NONE, {}),
    "tukey": (RK_TUKEY, {}),
    "exact": (RK_HUBER, {"reduced_solver": 1}),
    "upper": (RK_HUBER, {"spmv_upper": 1}),
    "profile": (RK_HUBER, {"profile": 1}),
    "lm_order_off": (RK_HUBER, {"landmark_reorder": 0}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_lm_follows_the_dense_reference(g40, case):
    rk, opts = CASES[case]
    fp = flatten(freed(g40))
    pri = make_priors(fp, list(range(0, fp.Pf, 4)), seed=3)
    ref = dense_run(fp, rk, pri, 10)
    got = solver(fp, rk, pri, **opts).optimize(10)["chi2"]
    assert len(got) == len(ref["chi2"])
    assert rel(got, ref["chi2"]).max() <= CHI2_TOL


def test_shuffled_pose_ids_follow_the_dense_reference():
    g = shuffled_pose_ids(synth_ba(60, 900, 3600, seed=2), seed=1)
    fp = flatten(g)
    pri = make_priors(fp, list(range(0, fp.Pf, 3)), seed=4)
    got = solver(fp, RK_HUBER, pri).optimize(10)["chi2"]
    ref = dense_run(fp, RK_HUBER, pri, 10)
    assert len(got) == len(ref["chi2"]) and rel(got, ref["chi2"]).max() <= CHI2_TOL


def test_motion_only_with_priors_follows_the_dense_reference(g40):
    fp = flatten(with_fixed(freed(g40), fixed_lm_rows=range(g40.nlandmarks)))
    assert fp.Lf == 0
    pri = make_priors(fp, list(range(0, fp.Pf, 2)), seed=5)
    got = solver(fp, RK_HUBER, pri).optimize(10)["chi2"]
    ref = dense_run(fp, RK_HUBER, pri, 10)
    assert len(got) == len(ref["chi2"]) and rel(got, ref["chi2"]).max() <= CHI2_TOL


def test_host_loop_is_the_device_decision_loop(g40):
    """the host loop sums the edges' chi2 in other partials than the fused trial tail (as without priors, tests/test_gpu_parity.py): the
    two agree to rounding, trial for trial; each is bit-reproducible"""
    fp = flatten(freed(g40))
    pri = make_priors(fp, list(range(0, fp.Pf, 3)), seed=6)
    a, b = solver(fp, RK_HUBER, pri, pcg_tol=1e-11), solver(fp, RK_HUBER, pri, pcg_tol=1e-11, profile=1)
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    assert len(ca) == len(cb) and rel(ca, cb).max() <= 1e-9
    assert a.counters()["lm_trials"] == b.counters()["lm_trials"]
    for x, y in zip(a.state(), b.state()):
        assert np.abs(x - y).max() <= 1e-8
    c = solver(fp, RK_HUBER, pri, pcg_tol=1e-11, profile=1)
    assert np.array_equal(c.optimize(10)["chi2"], cb)


# ---- optimality ----------------------------------------------------------------------------------------------------------------------
def test_gradient_vanishes_at_a_non_zero_prior_residual(g40):
    """an identity Jacobian in place of J_l(r)^-1 leaves the gradient of the priors at ~1e-3 of its start: this test fails then"""
    fp = flatten(freed(g40))
    pri = make_priors(fp, list(range(0, fp.Pf, 2)), seed=7, rot=0.1, trans=0.5)
    o = OracleSolver(fp, RK_NONE)
    g0 = np.linalg.norm(pr.gradient(o, fp, pri))
    h = solver(fp, RK_NONE, pri, pcg_tol=1e-12)
    h.optimize(40)
    o.set_state(*h.state())
    q, t, _ = h.state()
    assert pr.prior_chi2(pri, q, t, fp.Pf).sum() > 1.0
    assert np.linalg.norm(pr.gradient(o, fp, pri)) <= 1e-6 * g0


# ---- special prior sets --------------------------------------------------------------------------------------------------------------
def test_zero_information_is_no_prior(g40):
    fp = flatten(g40)
    pri = make_priors(fp, [1, 2, 3], seed=8)
    pri = (pri[0], pri[1], pri[2], np.zeros_like(pri[3]))
    a, b = solver(fp, RK_HUBER), solver(fp, RK_HUBER, pri)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)


def test_strong_prior_is_a_fixed_pose(g40):
    fixed = flatten(g40)
    fp = flatten(freed(g40))
    q0, t0 = np.asarray(fp.q).reshape(-1, 4), np.asarray(fp.t).reshape(-1, 3)
    pri = (np.array([0]), q0[:1].copy(), t0[:1].copy(), np.array([1e10 * np.eye(6)]))
    a, b = solver(fixed, RK_HUBER, pcg_tol=1e-12), solver(fp, RK_HUBER, pri, pcg_tol=1e-12)
    a.optimize(60); b.optimize(60)         # (to convergence: the prior's lambda_0 = tau * 1e10 starts the run far more damped)
    qa, ta, Xa = a.state()
    qb, tb, Xb = b.state()
    # (flatten puts the fixed pose after the free ones: compare by the graph's own rows)
    ia, ib = np.asarray(fixed.pose_src), np.asarray(fp.pose_src)
    oa, ob = np.argsort(ia), np.argsort(ib)
    assert np.abs(qa[oa] - qb[ob]).max() <= 1e-6
    assert np.abs(ta[oa] - tb[ob]).max() <= 1e-6
    # (landmarks: the weakly observed ones -- far out, or seen from two poses -- are determined no better than the LM tail converges them
    # in either run; one of the 600 runs off to 1e5 m in both)
    near = (np.abs(Xa) < 1e3).all(axis=1) & (np.abs(Xb) < 1e3).all(axis=1)
    d = np.abs(Xa - Xb).max(axis=1)[near]
    assert near.mean() > 0.98 and np.mean(d <= 1e-6) >= 0.95 and d.max() <= 1e-2


def test_duplicate_priors_add_up(g40):
    fp = flatten(g40)
    pri = make_priors(fp, [4, 4], seed=9)
    one = (pri[0][:1], pri[1][:1], pri[2][:1], (pri[3][0] + pri[3][1])[None])
    two = (pri[0], np.repeat(pri[1][:1], 2, axis=0), np.repeat(pri[2][:1], 2, axis=0), pri[3])
    a, b = solver(fp, RK_HUBER, one), solver(fp, RK_HUBER, two)
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    assert len(ca) == len(cb) and rel(ca, cb).max() <= 1e-9


# ---- scale ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitti07", "big"])
def test_pcg_and_exact_solver_agree_at_scale(name):
    g = synth_named("kitti07") if name == "kitti07" else synth_ba(1700, 12000, 60000, seed=3)
    fp = flatten(g)
    pri = make_priors(fp, list(range(0, fp.Pf, 10)), seed=10)
    a = solver(fp, RK_HUBER, pri)
    ca = a.optimize(10)["chi2"]
    cb = solver(fp, RK_HUBER, pri, reduced_solver=1).optimize(10)["chi2"]
    assert len(ca) == len(cb) and rel(ca, cb).max() <= CHI2_TOL
    hist, unconverged = a.pcg_history()
    assert unconverged == 0 and np.all(hist >= 0)


# ---- covariance ----------------------------------------------------------------------------------------------------------------------
def test_covariance_of_a_graph_anchored_by_a_prior_only(g40):
    fp = flatten(freed(g40))
    assert fp.Pf == fp.Pt
    pri = make_priors(fp, [0], seed=11)
    h = solver(fp, RK_HUBER, pri)
    h.optimize(3)
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    H, _ = pr.system(o, fp, pri, 0.0)
    Hi = np.linalg.inv(H)
    cov = h.covariance(landmarks=False)
    assert not cov["not_positive_definite"]
    for p in range(fp.Pf):
        want = Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        assert np.abs(cov["pose"][p] - want).max() <= 1e-9 * np.abs(want).max()
    pairs = [("pose", 0, "pose", fp.Pf - 1), ("pose", 3, "pose", 20)]
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    for k, (_, a, _, b) in enumerate(pairs):
        want = Hi[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        assert np.abs(np.asarray(blocks[k])[:6, :6] - want).max() <= 1e-9 * np.abs(want).max()
    # the call changes nothing the LM path sees
    c = solver(fp, RK_HUBER, pri)
    c.optimize(3)
    assert np.array_equal(h.optimize(5)["chi2"], c.optimize(5)["chi2"])


# ---- batch ---------------------------------------------------------------------------------------------------------------------------
def test_batch_with_priors_is_the_solo_runs(g40):
    fps = [flatten(freed(synth_ba(40, 600, 2400, seed=s))) for s in (1, 2, 3)]
    pris = [make_priors(fps[0], range(0, 40, 3), seed=12), None, make_priors(fps[2], range(1, 40, 5), seed=13)]
    solo = [solver(f, RK_HUBER, p).optimize(8)["chi2"] for f, p in zip(fps, pris)]
    hs = [solver(f, RK_HUBER, p) for f, p in zip(fps, pris)]
    chi, _ = optimize_batch(hs, 8)
    for k in range(3):
        assert np.array_equal(np.asarray(chi[k])[:len(solo[k])], solo[k])


def test_plain_batch_still_batches():
    fps = [flatten(synth_ba(40, 600, 2400, seed=s)) for s in (1, 2)]
    hs = [solver(f, RK_HUBER) for f in fps]
    _, batched = optimize_batch(hs, 5)
    assert batched > 0


# ---- life cycle ----------------------------------------------------------------------------------------------------------------------
def test_set_graph_clears_the_priors(g40):
    fp = flatten(g40)
    h = solver(fp, RK_HUBER, make_priors(fp, [1, 2], seed=14))
    h.set_graph(fp)
    assert len(h.prior_chi_squares()) == 0
    assert np.array_equal(h.optimize(5)["chi2"], solver(fp, RK_HUBER).optimize(5)["chi2"])


def test_changing_priors_depends_on_state_and_priors_only(g40):
    fp = flatten(freed(g40))
    A = make_priors(fp, range(0, 40, 2), seed=15)
    B = make_priors(fp, range(1, 40, 3), seed=16)
    h = solver(fp, RK_HUBER, A, heuristics=0)
    q, t, X = h.state()
    h.optimize(6)
    h.set_pose_priors(*B)
    h.set_state(q, t, X)
    ch = h.optimize(6)["chi2"]
    f = solver(fp, RK_HUBER, B, heuristics=0)
    assert np.array_equal(ch, f.optimize(6)["chi2"])
    for x, y in zip(h.state(), f.state()):
        assert np.array_equal(x, y)
    g = solver(fp, RK_HUBER, B, heuristics=0)
    assert np.array_equal(g.optimize(6)["chi2"], ch)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_usable_handle(g40):
    fp = flatten(g40)
    good = make_priors(fp, [1, 2], seed=17)
    h = solver(fp, RK_HUBER, good)
    before = h.prior_chi_squares()
    bad_index = (np.array([1, fp.Pt]), good[1], good[2], good[3])
    nan_q = (good[0], good[1].copy(), good[2], good[3]); nan_q[1][0, 0] = np.nan
    asym = (good[0], good[1], good[2], good[3].copy()); asym[3][0, 0, 5] += 1.0
    for bad in (bad_index, nan_q, asym):
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_pose_priors(*bad)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_partition(0, fp.Lt // 2)
    assert np.array_equal(h.prior_chi_squares(), before)
    p = solver(fp, RK_HUBER)
    p.set_partition(0, fp.Lt // 2)
    with pytest.raises(CubaHipError, match="status 3"):
        p.set_pose_priors(*good)
    assert len(h.optimize(5)["chi2"]) > 0


# ---- other builds --------------------------------------------------------------------------------------------------------------------
def test_fp32_library_and_mixed_precision(g40):
    fp = flatten(freed(g40))
    pri = make_priors(fp, range(0, 40, 4), seed=18)
    ref = solver(fp, RK_HUBER, pri).optimize(10)["chi2"]
    f32 = solver(fp, RK_HUBER, pri, precision="f32").optimize(10)["chi2"]
    n = min(len(f32), len(ref))
    assert n >= 8 and rel(f32[:n], ref[:n]).max() <= 1e-5
    mixed = solver(fp, RK_HUBER, pri, mixed_precision=1).optimize(10)["chi2"]
    assert len(mixed) == len(ref) and rel(mixed, ref).max() <= CHI2_TOL

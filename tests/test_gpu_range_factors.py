"""Range factors on the poses (cuba_hip_set_range_factors / HipSolver.set_range_factors) on the GPU against the numpy model of
tests/range_factor_reference.py: the assembled system (which numbers are touched and which keep their bits), the objective, LM
trajectories against a dense fp64 LM, optimality at a non-zero residual with rejected trials (the bar both wrong Jacobians miss), the
point rho = 0 and other special sets, the gauge and scale of four anchors heard from three poses, covariances, the handle's life cycle,
the refusals, batches, the other builds, repeatability, and the smallest shapes at which the launch geometry changes.  The bars are those
of tests/test_gpu_position_factors.py: assembled terms 1e-12, chi2 series 1e-6, covariances 1e-9, other builds 1e-5."""
import dataclasses
import math

import numpy as np
import pytest

import direction_factor_reference as dr
import landmark_prior_reference as lr
import position_factor_reference as pfr
import range_factor_reference as rr
import robust_pose_factor_reference as rb
from conftest import RK_HUBER, with_fixed
from test_gpu_configs import shuffled_pose_ids
from test_gpu_pose_priors import make_priors as make_pose_priors
from test_gpu_relative_pose import make_rel
from test_range_factor_reference import GRADIENT_BAR, OPT_ITERATIONS, free_graph, gauge_set, main_set, optimality_case, with_kernel

from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle.oracle import OracleSolver

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
KINDS = {"none": rb.NONE, "huber": rb.HUBER, "tukey": rb.TUKEY, "cauchy": rb.CAUCHY}
UP = np.triu(np.ones((6, 6), dtype=bool))


def solver(fp, factors=None, rk=RK_HUBER, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if factors is not None:
        h.set_range_factors(*factors)
    return h


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


@pytest.fixture(scope="module")
def fp40(g40):
    return flatten(g40)


_dense = {}


def dense_ref(fp40, kind):
    """the dense LM of the main set under one kernel, 10 iterations: computed once, shared by the cases that run the same problem"""
    if kind not in _dense:
        _dense[kind] = rr.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, main_set(fp40, kind), 10)["chi2"]
    return _dense[kind]


def follows(got, ref, at_least=8):
    """the per-iteration chi2 within CHI2_TOL over the iterations both ran (the dense LM on the CPU runs all 10 without a rejection)"""
    n = min(len(got), len(ref))
    worst = rel(got[:n], ref[:n]).max()
    print("%d / %d iterations, worst relative chi2 difference %.3g (bar %g)" % (len(got), len(ref), worst, CHI2_TOL))
    assert n >= at_least
    assert worst <= CHI2_TOL


def assembled(h, mode):
    if mode == 0:
        h.build_system()
        h.assemble()
    else:
        h.set_lambda(0.0)
        h.schur()


def check_assembled(fp, s, mode, label):
    """(with factors) - (plain) against the model's terms: the upper triangle of the diagonal block and bp (mode 1: bsc too) of every free
    pose with factors within 1e-12 of the block's (vector's) largest entry; everything else -- the off-diagonal blocks, the blocks and
    entries of the poses without factors -- keeps the plain handle's bits"""
    plain, withf = solver(fp), solver(fp, s)
    for h in (plain, withf):
        assembled(h, mode)
    rp, ci, v0 = plain.hsc()
    _, _, v1 = withf.hsc()
    q, t, _ = withf.state()
    Hd, bd = rr.factor_system(s, q, t, fp.Pf)
    diag = rp[:-1]
    off = np.setdiff1d(np.arange(len(ci)), diag)
    if mode == 1:
        assert np.array_equal(v0[off], v1[off])
    have = np.zeros(fp.Pf, dtype=bool)
    have[np.unique(s[0][s[0] < fp.Pf])] = True
    worst = 0.0
    for p in range(fp.Pf):
        a0, a1 = v0[diag[p]], v1[diag[p]]
        if not have[p]:
            assert np.array_equal(a0[UP], a1[UP])
            continue
        assert not np.array_equal(a0[UP], a1[UP])
        want = a0 + Hd[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        worst = max(worst, np.abs(a1[UP] - want[UP]).max() / np.abs(want[UP]).max())
    print(label, "mode", mode, "diagonal blocks %.3g (bar 1e-12)" % worst)
    assert np.isfinite(v1[diag][:, UP]).all()
    assert worst <= 1e-12
    for name in ("bp", "bsc")[:mode + 1]:
        a0, a1 = plain.array(name).reshape(-1, 6), withf.array(name).reshape(-1, 6)
        assert np.array_equal(a0[~have], a1[~have])
        want = a0 + bd.reshape(-1, 6)
        err = np.abs(a1 - want).max() / np.abs(want).max()
        print(label, "mode", mode, name, "%.3g (bar 1e-12)" % err)
        assert err <= 1e-12
        assert np.abs(bd).max() >= 1e-6 * np.abs(want).max()          # (the terms are far above the bar: a missing one would show)
    return withf


# ---- assembly ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["none", "huber"])
def test_assembled_system_is_the_plain_one_plus_the_factor_terms(fp40, kind, mode):
    """the main set (two factors on pose 5, one on the fixed pose) -- a missing term or a wrong Jacobian stands near 1e-6 of the block"""
    s = main_set(fp40, KINDS[kind])
    if kind == "huber":
        q0, t0 = np.asarray(fp40.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp40.t, dtype=np.float64).reshape(-1, 3)
        e = rr.factor_chi2(s, q0, t0, fp40.Pf)
        assert (e[e > 0] < 4.0).any() and (e > 4.0).any()     # factors on both sides of delta^2
    check_assembled(fp40, s, mode, kind)


# ---- objective -----------------------------------------------------------------------------------------------------------------------
def test_objective_and_factor_chi_squares(fp40):
    fp = fp40
    s = with_kernel(rr.make_factors(fp, [2, 9, fp.Pt - 1, 30, 9], seed=2), rb.HUBER)
    plain, withf = solver(fp), solver(fp, s)
    q, t, _ = withf.state()
    want = rr.factor_chi2(s, q, t, fp.Pf)
    got = withf.range_factor_chi_squares()
    assert got[2] == 0.0 and want[2] == 0.0                       # the factor on the fixed pose is ignored
    print("per-factor chi2 %.3g of the largest (bar 1e-10)" % (np.abs(got - want).max() / want.max()))
    assert np.abs(got - want).max() <= 1e-10 * want.max()
    F = withf.compute_errors()
    assert abs(F - (plain.compute_errors() + rr.factor_objective(s, q, t, fp.Pf))) <= 1e-12 * F
    # lambda_0 includes the factors: the maximum diagonal is that of Hpp + their terms
    assert withf.max_diagonal() >= plain.max_diagonal()


# ---- LM parity against the dense reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_lm_follows_the_dense_reference(fp40, kind):
    s = main_set(fp40, KINDS[kind])
    h = solver(fp40, s)
    follows(h.optimize(10)["chi2"], dense_ref(fp40, KINDS[kind]))
    # the per-factor chi2 and the objective at the result
    q, t, _ = h.state()
    want = rr.factor_chi2(s, q, t, fp40.Pf)
    assert np.abs(h.range_factor_chi_squares() - want).max() <= 1e-10 * want.max()
    plain = solver(fp40)
    plain.set_state(*h.state())
    F = h.compute_errors()
    assert abs(F - (plain.compute_errors() + rr.factor_objective(s, q, t, fp40.Pf))) <= 1e-12 * F


OPTIONS = {"exact": {"reduced_solver": 1}, "upper": {"spmv_upper": 1}, "profile": {"profile": 1}}


@pytest.mark.parametrize("case", sorted(OPTIONS))
def test_lm_follows_the_dense_reference_under_options(fp40, case):
    follows(solver(fp40, main_set(fp40, rb.HUBER), **OPTIONS[case]).optimize(10)["chi2"], dense_ref(fp40, rb.HUBER))


def test_shuffled_pose_ids_follow_the_dense_reference(g40):
    fp = flatten(shuffled_pose_ids(g40, seed=1))
    assert not np.array_equal(fp.eP, flatten(g40).eP)
    s = main_set(fp, rb.HUBER)
    follows(solver(fp, s).optimize(10)["chi2"], rr.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_motion_only_follows_the_dense_reference(g40):
    fp = flatten(with_fixed(g40, fixed_lm_rows=range(g40.nlandmarks)))
    assert fp.Lf == 0
    s = main_set(fp, rb.CAUCHY)
    follows(solver(fp, s).optimize(10)["chi2"], rr.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_with_every_other_kind_of_factor(fp40):
    """pose priors, a relative-pose edge, landmark priors, position and direction factors on one handle: the range factors' launch is
    the last"""
    fp = fp40
    s = main_set(fp, rb.CAUCHY)
    pri = make_pose_priors(fp, [1, 5, 17], seed=1)
    edges = make_rel(fp, [(3, 20)], seed=2)
    lmp = lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0)
    pos = pfr.make_factors(fp, [5, 8, 22], seed=4, kind=rb.HUBER, delta=2.0)
    dirs = dr.make_factors(fp, [5, 9, 30], seed=5, kind=rb.HUBER, delta=2.0)
    ref = rr.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10, df=dirs, pf=pos, lmp=lmp, priors=pri, rel=edges)["chi2"]
    h = solver(fp, s)
    h.set_pose_priors(*pri)
    h.set_relative_pose_edges(*edges)
    h.set_landmark_priors(*lmp)
    h.set_position_factors(*pos)
    h.set_direction_factors(*dirs)
    follows(h.optimize(10)["chi2"], ref)


# ---- rejected trials, optimality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rejected_trials_and_a_vanishing_gradient_at_a_non_zero_residual(kind):
    """the case sized on the CPU (tests/test_range_factor_reference.py: optimality_case): synth_ba(12, 96, 400, seed=1), one factor on
    every free pose plus one on the fixed pose, ranges of 0.7 ... 8.8 m with half a metre of noise and of arm, 120 iterations allowed.
    There the dense LM with the right Jacobian ends at 1.4e-9 / 5.4e-11 / 4.6e-9 / 5.7e-12 of the start gradient (none / Huber / Tukey /
    Cauchy) with genuinely rejected trials from trial 15 / 7 / 10 / 16 on (gain ratio below -1e-3: the residual is non-linear and large,
    long before rounding decides anything), the factors' e summing to 61 ... 536; with the world-frame direction R^T m for m it stalls at
    >= 1.2e-4, without the rotation columns at >= 1.5e-5.  The bar 1e-6 sits 15 x below the wrong Jacobians' best result and 200 x above
    the right one's worst.  A restore after a rejected trial linearises the factors at the restored poses: the chi2 series follows the
    dense LM over the iterations both ran."""
    fp, s = optimality_case(KINDS[kind])
    o = OracleSolver(fp, RK_HUBER)
    g0 = np.linalg.norm(rr.gradient(o, fp, s))
    ref = rr.dense_lm(o, fp, s, OPT_ITERATIONS)
    genuine = [i for i, x in enumerate(ref["gains"]) if x < -1e-3]
    assert genuine
    h = solver(fp, s, pcg_tol=1e-12)
    got = h.optimize(OPT_ITERATIONS)["chi2"]
    n = min(len(got), len(ref["chi2"]))
    worst = rel(got[:n], ref["chi2"][:n]).max()
    o.set_state(*h.state())
    g1 = np.linalg.norm(rr.gradient(o, fp, s))
    q, t, _ = h.state()
    e = rr.factor_chi2(s, q, t, fp.Pf)
    print("%s: dense %d iterations, %d rejected (first genuine one at trial %d); library %d iterations, %d trials; worst relative chi2 "
          "difference %.3g; gradient %.3g of its start; factor chi2 sum %.4g max %.4g"
          % (kind, len(ref["chi2"]), ref["rejected"], genuine[0], len(got), h.counters()["lm_trials"], worst, g1 / g0, e.sum(), e.max()))
    # (both sides run past the first genuinely rejected trial: the series compared includes a restore)
    assert n > genuine[0] and h.counters()["lm_trials"] > len(got)
    assert worst <= CHI2_TOL
    assert e.max() > 1e-3
    assert g1 <= GRADIENT_BAR * g0


# ---- the point rho = 0 and other special sets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "huber"])
def test_the_antenna_at_the_anchor_adds_nothing_and_keeps_its_residual(fp40, kind):
    """identity quaternion on pose 7, b = 0, a = t: u = (a - t) - R b is exactly 0.  The rule: m = 0, so J = 0 -- a finite system, the
    plain handle's bits in H and g, chi2 = Omega rbar^2 -- under both instantiations of the kernels; a second factor on another pose keeps
    its terms, and a run from there stays finite"""
    fp = fp40
    plain = solver(fp)
    q, t, X = plain.state()
    q, t = q.copy(), t.copy()
    q[7] = (0.0, 0.0, 0.0, 1.0)
    plain.set_state(q, t, X)
    at_zero = (np.array([7], dtype=np.int32), np.zeros((1, 3)), np.array([0.75]), np.array([16.0]), t[7][None].copy())
    s = with_kernel(at_zero + (None, None), KINDS[kind])
    withf = solver(fp, s)
    withf.set_state(q, t, X)
    chi = withf.range_factor_chi_squares()
    assert chi[0] == 16.0 * 0.75 ** 2
    F0, F1 = plain.compute_errors(), withf.compute_errors()
    assert abs(F1 - (F0 + rb.rho(KINDS[kind], 2.0, 9.0))) <= 1e-12 * F1
    for mode in (0, 1):
        for h in (plain, withf):
            assembled(h, mode)
        assert np.array_equal(plain.hsc()[2], withf.hsc()[2]) and np.isfinite(withf.hsc()[2]).all()
        for name in ("bp", "bsc")[:mode + 1]:
            assert np.array_equal(plain.array(name), withf.array(name)) and np.isfinite(withf.array(name)).all()
    # with a second, ordinary factor: that one's terms, nothing of the first
    other = rr.make_factors(fp, [12], seed=3)
    both = tuple(np.concatenate([x, y]) for x, y in zip(at_zero, other[:5]))
    two, one = solver(fp, with_kernel(both + (None, None), KINDS[kind])), solver(fp, with_kernel(other, KINDS[kind]))
    for h in (two, one):
        h.set_state(q, t, X)
        assembled(h, 1)
    assert np.array_equal(two.hsc()[2], one.hsc()[2]) and np.array_equal(two.array("bsc"), one.array("bsc"))
    chi2 = two.optimize(5)["chi2"]
    assert len(chi2) > 0 and np.isfinite(chi2).all() and all(np.isfinite(x).all() for x in two.state())


def test_zero_information_is_no_factor(fp40):
    s = main_set(fp40)
    zero = s[:3] + (np.zeros_like(s[3]), s[4], None, None)
    a, b = solver(fp40), solver(fp40, zero)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)


def test_kinds_all_zero_is_no_kernel(fp40):
    s = main_set(fp40)
    n = len(s[0])
    given = s[:5] + (np.zeros(n, dtype=np.int32), np.full(n, 2.5))
    a, b = solver(fp40, s), solver(fp40, given)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.range_factor_chi_squares(), b.range_factor_chi_squares())


def test_two_factors_with_one_anchor_are_one_with_the_summed_information(fp40):
    s = rr.make_factors(fp40, [31, 31], seed=9)
    b, rng, arm = np.repeat(s[1][:1], 2, axis=0), np.repeat(s[2][:1], 2), np.repeat(s[4][:1], 2, axis=0)
    two = (s[0], b, rng, s[3], arm, None, None)
    one = (s[0][:1], b[:1], rng[:1], s[3][:1] + s[3][1:], arm[:1], None, None)
    ca, cb = solver(fp40, one).optimize(10)["chi2"], solver(fp40, two).optimize(10)["chi2"]
    print("worst relative chi2 difference %.3g (bar 1e-9)" % rel(ca, cb).max())
    assert len(ca) == len(cb) and rel(ca, cb).max() <= 1e-9


def test_factors_on_fixed_poses_are_ignored(fp40):
    fp = fp40
    assert fp.Pt > fp.Pf
    s = with_kernel(rr.make_factors(fp, [fp.Pt - 1] * 3, seed=2), rb.HUBER)
    a, b = solver(fp), solver(fp, s)
    assert not b.range_factor_chi_squares().any()
    assert np.array_equal(a.optimize(6)["chi2"], b.optimize(6)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    assert not b.range_factor_chi_squares().any()


# ---- gauge, covariance ---------------------------------------------------------------------------------------------------------------
def test_four_anchors_heard_from_three_poses_hold_a_graph_without_a_fixed_vertex(g40):
    """every pose and landmark free, four non-coplanar anchors each heard from poses 2, 20 and 37: the plain handle's reduced matrix is
    not positive definite for the exact solver's factorisation, with the ranges it is: an LM run under reduced_solver = 1 descends, and
    the pose covariances are the blocks of the dense inverse of the weighted Hessian, block by block within the covariances' bar 1e-9 of
    the block's largest entry, as in test_covariance_includes_the_weighted_factor_terms.  (The system is ill-conditioned -- 2.6e10: the
    seventh eigenvalue of the free system, 1.15e-3, against 3e7 -- and both sides invert it in fp64; the worst block is printed.)"""
    fp = free_graph(g40)
    assert fp.Pf == fp.Pt and fp.Lf == fp.Lt
    s = gauge_set(fp)
    assert solver(fp).covariance(landmarks=False)["not_positive_definite"]
    h = solver(fp, s)
    cov = h.covariance(landmarks=False)
    assert not cov["not_positive_definite"]
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    H = rr.system(o, fp, s, 0.0)[0]
    ev = np.linalg.eigvalsh(H)
    Hi = np.linalg.inv(H)
    worst = 0.0
    for p in range(fp.Pf):
        want = Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        worst = max(worst, np.abs(cov["pose"][p] - want).max() / np.abs(want).max())
    print("pose covariance blocks against the dense inverse: %.3g of the block's largest entry (bar 1e-9, condition number %.3g)" % (worst, ev[-1] / ev[0]))
    assert worst <= 1e-9
    ex = solver(fp, s, reduced_solver=1)
    res = ex.optimize(6)
    chi2 = res["chi2"]
    assert len(chi2) >= 3 and np.isfinite(chi2).all() and chi2[-1] < chi2[0]
    assert ex.counter("exact_solve_fallbacks") > 0 and ex.counter("exact_solve_failures") == 0


def test_covariance_includes_the_weighted_factor_terms(fp40):
    fp = fp40
    s = main_set(fp, rb.HUBER)
    h = solver(fp, s)
    h.optimize(3)
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    Hi = np.linalg.inv(rr.system(o, fp, s, 0.0)[0])
    cov = h.covariance()
    assert not cov["not_positive_definite"]
    n = 6 * fp.Pf
    worst = 0.0
    for p in range(fp.Pf):
        want = Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        worst = max(worst, np.abs(cov["pose"][p] - want).max() / np.abs(want).max())
    for l in range(fp.Lf):
        want = Hi[n + 3 * l:n + 3 * l + 3, n + 3 * l:n + 3 * l + 3]
        worst = max(worst, np.abs(cov["landmark"][l] - want).max() / np.abs(want).max())
    print("covariance blocks against the dense inverse: %.3g (bar 1e-9)" % worst)
    assert worst <= 1e-9
    pa, pb = int(s[0][0]), int(s[0][1])
    pairs = [("pose", pa, "landmark", 40), ("pose", pa, "pose", pb), ("landmark", 7, "landmark", 300)]
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    off = {"pose": lambda i: (6 * i, 6), "landmark": lambda i: (n + 3 * i, 3)}
    for k, (ka, a, kb, b) in enumerate(pairs):
        (ra, da), (cb, db) = off[ka](a), off[kb](b)
        want = Hi[ra:ra + da, cb:cb + db]
        assert np.abs(np.asarray(blocks[k])[:da, :db] - want).max() <= 1e-9 * np.abs(Hi).max()
    # (the factors are in it: without them the pose blocks differ far beyond the bar)
    Hplain = np.linalg.inv(rr.system(o, fp, None, 0.0)[0])
    assert np.abs(Hplain[6 * pa:6 * pa + 6, 6 * pa:6 * pa + 6] - Hi[6 * pa:6 * pa + 6, 6 * pa:6 * pa + 6]).max() > 1e-6 * np.abs(Hi[6 * pa:6 * pa + 6, 6 * pa:6 * pa + 6]).max()


# ---- life cycle and refusals ---------------------------------------------------------------------------------------------------------
def test_set_graph_clears_the_factors(fp40):
    h = solver(fp40, main_set(fp40, rb.HUBER))
    h.set_graph(fp40)
    assert len(h.range_factor_chi_squares()) == 0
    assert np.array_equal(h.optimize(5)["chi2"], solver(fp40).optimize(5)["chi2"])


def test_replacing_the_set_depends_on_state_and_set_only(fp40):
    A = main_set(fp40, rb.HUBER)
    B = with_kernel(rr.make_factors(fp40, [3, 8, 8, 30], seed=11), rb.CAUCHY)
    h = solver(fp40, A, heuristics=0)
    q, t, X = h.state()
    h.optimize(6)
    builds = h.counter("structure_builds")
    h.set_range_factors(*B)
    h.set_state(q, t, X)
    ch = h.optimize(6)["chi2"]
    assert h.counter("structure_builds") == builds
    f = solver(fp40, B, heuristics=0)
    assert np.array_equal(ch, f.optimize(6)["chi2"])
    for x, y in zip(h.state(), f.state()):
        assert np.array_equal(x, y)
    # n = 0 clears the set
    h.set_range_factors([], np.zeros((0, 3)), np.zeros(0), np.zeros(0))
    h.set_state(q, t, X)
    assert np.array_equal(h.optimize(4)["chi2"], solver(fp40, heuristics=0).optimize(4)["chi2"])
    assert h.counter("structure_builds") == builds


def test_refusals_leave_a_usable_handle(fp40):
    fp = fp40
    good = with_kernel(rr.make_factors(fp, [4, 11, 11, 25, 30, 36], seed=3), rb.HUBER)
    h = solver(fp, good)
    before = h.range_factor_chi_squares()
    n = len(good[0])

    def variant(**kw):
        d = dict(pose=good[0], anchor=good[1], range=good[2], info=good[3], lever_arm=good[4], kind=good[5], delta=good[6])
        d.update(kw)
        return d["pose"], d["anchor"], d["range"], d["info"], d["lever_arm"], d["kind"], d["delta"]

    def changed(x, at, value):
        x = x.copy()
        x[at] = value
        return x

    bads = [variant(pose=changed(good[0], 2, fp.Pt)), variant(pose=changed(good[0], 0, -1)), variant(anchor=changed(good[1], (1, 2), np.nan)),
            variant(lever_arm=changed(good[4], (4, 0), np.inf)), variant(range=changed(good[2], 3, np.nan)), variant(range=changed(good[2], 3, np.inf)),
            variant(range=changed(good[2], 5, -1e-3)), variant(info=changed(good[3], 0, np.inf)), variant(info=changed(good[3], 1, np.nan)),
            variant(info=changed(good[3], 2, -1.0)), variant(kind=changed(good[5], 1, 4)), variant(kind=changed(good[5], 1, -1)),
            variant(delta=changed(good[6], 2, 0.0)), variant(delta=changed(good[6], 2, -1.0)), variant(delta=changed(good[6], 2, np.nan)),
            variant(kind=None), variant(delta=None)]
    for bad in bads:
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_range_factors(*bad)
        assert np.array_equal(h.range_factor_chi_squares(), before)
    # a zero range and a zero information are valid
    h.set_range_factors(*variant(range=changed(good[2], 0, 0.0), info=changed(good[3], 1, 0.0)))
    assert h.range_factor_chi_squares()[1] == 0.0
    h.set_range_factors(*good)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_partition(0, fp.Lt // 2)
    assert np.array_equal(h.range_factor_chi_squares(), before)
    p = solver(fp)
    p.set_partition(0, fp.Lt // 2)
    with pytest.raises(CubaHipError, match="status 3"):
        p.set_range_factors(*good)
    p.set_partition(0, -1)                            # (the whole graph again: the same call is accepted)
    p.set_range_factors(*good)
    assert np.array_equal(p.range_factor_chi_squares(), before)
    assert len(h.optimize(5)["chi2"]) > 0
    assert n == len(h.range_factor_chi_squares())


def test_graph_without_edges_is_refused(fp40):
    fp = fp40
    none = dataclasses.replace(fp, eP=fp.eP[:0], eL=fp.eL[:0], eDim=fp.eDim[:0], meas=fp.meas[:0], omega=fp.omega[:0], edge_src=fp.edge_src[:0])
    h = solver(none)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_range_factors(*rr.make_factors(none, [1, 2], seed=1))
    h.set_graph(fp)
    assert len(h.optimize(2)["chi2"]) > 0


# ---- batch ---------------------------------------------------------------------------------------------------------------------------
def test_batch_with_factors_is_the_solo_runs():
    fps = [flatten(synth_ba(40, 600, 2400, seed=s)) for s in (1, 2)]
    sets = [main_set(fps[0], rb.HUBER), main_set(fps[1], rb.TUKEY)]
    solo = [solver(f, s).optimize(8)["chi2"] for f, s in zip(fps, sets)]
    chi, _ = optimize_batch([solver(f, s) for f, s in zip(fps, sets)], 8)
    for k in range(2):
        assert np.array_equal(np.asarray(chi[k])[:len(solo[k])], solo[k])
    # (a plain batch still batches fully)
    _, batched = optimize_batch([solver(f) for f in fps], 5)
    assert batched > 0


# ---- other builds, repeatability -----------------------------------------------------------------------------------------------------
def test_fp32_library_and_mixed_precision(fp40):
    s = main_set(fp40, rb.HUBER)
    ref = solver(fp40, s).optimize(10)["chi2"]
    plain = solver(fp40).optimize(10)["chi2"]
    k = min(len(ref), len(plain))
    assert rel(ref[:k], plain[:k]).max() > 1e-4          # (the factors' share of chi2 is far above the bar below)
    for name, got in (("f32", solver(fp40, s, precision="f32").optimize(10)["chi2"]),
                      ("mixed", solver(fp40, s, mixed_precision=1).optimize(10)["chi2"])):
        n = min(len(got), len(ref))
        print(name, "%d iterations, worst relative chi2 difference %.3g (bar 1e-5)" % (n, rel(got[:n], ref[:n]).max()))
        assert n >= 8 and rel(got[:n], ref[:n]).max() <= 1e-5


def test_two_runs_are_bit_identical(fp40):
    s = main_set(fp40, rb.CAUCHY)
    a, b = solver(fp40, s), solver(fp40, s)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.range_factor_chi_squares(), b.range_factor_chi_squares())


# ---- the smallest shapes where the launch geometry changes ---------------------------------------------------------------------------
def check_chi_squares(fp, s, label):
    """the per-factor chi2 and the objective of a set against the model"""
    plain, withf = solver(fp), solver(fp, s)
    q, t, _ = withf.state()
    terms = rr.factor_terms(s, q, t, fp.Pf)
    want = np.array([x[0] for x in terms])
    got = withf.range_factor_chi_squares()
    print(label, "%d factors: per-factor chi2 %.3g of the largest (bar 1e-10)" % (len(want), np.abs(got - want).max() / want.max()))
    assert len(got) == len(want) and np.abs(got - want).max() <= 1e-10 * want.max()
    assert np.array_equal(got == 0, want == 0)
    F = withf.compute_errors()
    assert abs(F - (plain.compute_errors() + math.fsum(x[1] for x in terms))) <= 1e-12 * F


@pytest.mark.parametrize("mode", [0, 1])
def test_factors_on_more_than_64_free_poses(mode):
    """two workgroups of the 64-lane linearisation kernel: 67 free poses, one factor on each but poses 3 and 64 (65 lanes), a second one on
    the last free pose"""
    fp = flatten(synth_ba(68, 400, 2000, seed=3))
    assert fp.Pf == 67
    poses = [p for p in range(fp.Pf) if p not in (3, 64)] + [fp.Pf - 1, fp.Pt - 1]
    s = with_kernel(rr.make_factors(fp, poses, seed=12), rb.HUBER)
    assert len(np.unique(s[0][s[0] < fp.Pf])) == 65
    check_assembled(fp, s, mode, "65 poses")


def test_257_factors_make_two_chi2_partials(fp40):
    poses = np.random.default_rng(2).integers(0, fp40.Pt, size=257)
    check_chi_squares(fp40, with_kernel(rr.make_factors(fp40, poses, seed=13), rb.CAUCHY), "two partials")
    check_assembled(fp40, with_kernel(rr.make_factors(fp40, poses, seed=13), rb.CAUCHY), 0, "257 factors")


def test_16385_factors_take_the_chi2_kernel_round_its_grid_stride_loop():
    """64 workgroups of 256 lanes cover 16 384 factors in one trip: the last factor is the second trip's"""
    fp = flatten(synth_ba(12, 96, 400, seed=1))
    poses = np.random.default_rng(4).integers(0, fp.Pt, size=16385)
    poses[-1] = 2
    s = rr.make_factors(fp, poses, seed=14)
    check_chi_squares(fp, s, "grid stride")
    check_chi_squares(fp, with_kernel(s, rb.HUBER), "grid stride, robust")

"""Position factors on the poses (cuba_hip_set_position_factors / HipSolver.set_position_factors) on the GPU against the numpy model of
tests/position_factor_reference.py: the assembled system, the objective, LM trajectories against a dense fp64 LM (rejected trials
included), optimality at a non-zero residual, special sets, the gauge, covariances, the handle's life cycle, the refusals, batches, the
other builds and repeatability."""
import copy
import dataclasses

import numpy as np
import pytest

import landmark_prior_reference as lr
import position_factor_reference as pf
import robust_pose_factor_reference as rb
from conftest import RK_HUBER, with_fixed
from test_gpu_configs import shuffled_pose_ids
from test_gpu_pose_priors import make_priors as make_pose_priors
from test_gpu_relative_pose import make_rel

from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle.oracle import OracleSolver

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
KINDS = {"none": rb.NONE, "huber": rb.HUBER, "tukey": rb.TUKEY, "cauchy": rb.CAUCHY}
DELTAS = {rb.NONE: 1.0, rb.HUBER: 2.0, rb.TUKEY: 6.0, rb.CAUCHY: 2.0}


def with_kernel(s, kind):
    """the set under one kernel for all its factors (the sibling tests' deltas)"""
    n = len(s[0])
    return s[:4] + ((None, None) if kind == rb.NONE else (np.full(n, kind, dtype=np.int32), np.full(n, DELTAS[kind])))


def main_set(fp, kind=rb.NONE):
    """17 factors: 14 random free poses, pose 5 twice and the fixed pose (flatten puts it last); fixes 0.2 N(0, 1) off, arms 0.5 N(0, 1)"""
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.choice(fp.Pf, 14, replace=False), [5, 5, fp.Pt - 1]])
    return with_kernel(pf.make_factors(fp, poses, seed=6), kind)


def solver(fp, factors=None, rk=RK_HUBER, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if factors is not None:
        h.set_position_factors(*factors)
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
        _dense[kind] = pf.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, main_set(fp40, kind), 10)["chi2"]
    return _dense[kind]


def follows(got, ref, at_least=8):
    """the per-iteration chi2 within CHI2_TOL over the iterations both ran (the dense LM on the CPU runs all 10 without a rejection)"""
    n = min(len(got), len(ref))
    worst = rel(got[:n], ref[:n]).max()
    print("%d / %d iterations, worst relative chi2 difference %.3g (bar %g)" % (len(got), len(ref), worst, CHI2_TOL))
    assert n >= at_least
    assert worst <= CHI2_TOL


# ---- assembly ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "huber"])
def test_assembled_system_is_the_plain_one_plus_the_factor_terms(fp40, kind):
    """two factors on pose 5, one on the fixed pose, a zero lever arm among non-zero ones: the diagonal blocks (upper triangle), bp and
    bsc are the plain handle's plus the numpy terms, the off-diagonal blocks keep their bits"""
    fp = fp40
    s = pf.make_factors(fp, [1, 5, 5, 17, fp.Pf - 1, fp.Pt - 1], seed=1)
    s[3][3] = 0.0                                              # (pose 17: the camera centre itself)
    s = with_kernel(s, KINDS[kind])
    plain, withf = solver(fp), solver(fp, s)
    for h in (plain, withf):
        h.set_lambda(0.0)
        h.schur()
    rp, ci, v0 = plain.hsc()
    _, _, v1 = withf.hsc()
    q, t, _ = withf.state()
    if kind == "huber":
        e = pf.factor_chi2(s, q, t, fp.Pf)
        assert (e[e > 0] < 4.0).any() and (e > 4.0).any()     # factors on both sides of delta^2
    Hp, bp = pf.factor_system(s, q, t, fp.Pf)
    diag = rp[:-1]
    off = np.setdiff1d(np.arange(len(ci)), diag)
    assert np.array_equal(v0[off], v1[off])
    up = np.triu_indices(6)
    worst = 0.0
    for p in range(fp.Pf):
        want = v0[diag[p]] + Hp[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        worst = max(worst, np.abs(v1[diag[p]][up] - want[up]).max() / np.abs(want[up]).max())
    assert worst <= 1e-12
    for name in ("bp", "bsc"):
        a0, a1 = plain.array(name), withf.array(name)
        want = a0 + bp
        err = np.abs(a1 - want).max() / np.abs(want).max()
        print(kind, name, "%.3g" % err, "diagonal blocks %.3g (bar 1e-12)" % worst)
        assert err <= 1e-12


# ---- objective -----------------------------------------------------------------------------------------------------------------------
def test_objective_and_factor_chi_squares(fp40):
    fp = fp40
    s = with_kernel(pf.make_factors(fp, [2, 9, fp.Pt - 1, 30, 9], seed=2), rb.HUBER)
    plain, withf = solver(fp), solver(fp, s)
    q, t, _ = withf.state()
    want = pf.factor_chi2(s, q, t, fp.Pf)
    got = withf.position_factor_chi_squares()
    assert got[2] == 0.0 and want[2] == 0.0                       # the factor on the fixed pose is ignored
    assert np.abs(got - want).max() <= 1e-10 * want.max()
    F = withf.compute_errors()
    assert abs(F - (plain.compute_errors() + pf.factor_objective(s, q, t, fp.Pf))) <= 1e-12 * F
    # lambda_0 includes the factors: the maximum diagonal is that of Hpp + their terms
    assert withf.max_diagonal() >= plain.max_diagonal()


# ---- LM parity against the dense reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_lm_follows_the_dense_reference(fp40, kind):
    follows(solver(fp40, main_set(fp40, KINDS[kind])).optimize(10)["chi2"], dense_ref(fp40, KINDS[kind]))


OPTIONS = {"exact": {"reduced_solver": 1}, "upper": {"spmv_upper": 1}, "profile": {"profile": 1}}


@pytest.mark.parametrize("case", sorted(OPTIONS))
def test_lm_follows_the_dense_reference_under_options(fp40, case):
    follows(solver(fp40, main_set(fp40, rb.HUBER), **OPTIONS[case]).optimize(10)["chi2"], dense_ref(fp40, rb.HUBER))


def test_shuffled_pose_ids_follow_the_dense_reference(g40):
    fp = flatten(shuffled_pose_ids(g40, seed=1))
    assert not np.array_equal(fp.eP, flatten(g40).eP)
    s = main_set(fp, rb.HUBER)
    follows(solver(fp, s).optimize(10)["chi2"], pf.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_motion_only_follows_the_dense_reference(g40):
    fp = flatten(with_fixed(g40, fixed_lm_rows=range(g40.nlandmarks)))
    assert fp.Lf == 0
    s = main_set(fp, rb.CAUCHY)
    follows(solver(fp, s).optimize(10)["chi2"], pf.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_with_pose_priors_a_relative_pose_edge_and_landmark_priors(fp40):
    """every kind of factor on one handle: the position factors' launch sits behind the priors' and ahead of the edges'"""
    fp = fp40
    s = main_set(fp, rb.CAUCHY)
    pri = make_pose_priors(fp, [1, 5, 17], seed=1)
    edges = make_rel(fp, [(3, 20)], seed=2)
    lmp = lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0)
    ref = pf.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10, lmp=lmp, priors=pri, rel=edges)["chi2"]
    h = solver(fp, s)
    h.set_pose_priors(*pri)
    h.set_relative_pose_edges(*edges)
    h.set_landmark_priors(*lmp)
    follows(h.optimize(10)["chi2"], ref)


# ---- rejected trials, optimality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rejected_trials_and_a_vanishing_gradient_at_a_non_zero_residual(kind):
    """synth_ba(12, 96, 400, seed=1), one factor on every free pose plus one on the fixed pose, make_factors(seed=7).  On the CPU (this
    model, 40 iterations allowed) the dense LM with the right Jacobian ends after 28 / 24 / 25 / 26 iterations (none / Huber / Tukey /
    Cauchy; it stops on ten rejections in a row at the optimum, the first rejection at iteration 22 / 24 / 23 / 25) with 28 / 9 / 18 / 12
    rejected trials in all, at 7.2e-11 / 9.6e-10 /
    5.4e-10 / 9.6e-11 of the start gradient, the factors' e summing to 40 / 43 / 49 / 48 (largest 20 / 26 / 33 / 29): a genuinely
    non-zero residual.  With the rotation column R^T [a]x dropped from the system it stalls at 1.2e-4 / 9.5e-5 / 7.7e-5 / 5.6e-5.  The
    bar 1e-6 sits 56 x below the wrong Jacobian's best result and 1000 x above the right one's worst.  A restore after a rejected trial
    linearises the factors at the restored poses: the chi2 series follows the dense LM over the iterations both ran."""
    fp = flatten(synth_ba(12, 96, 400, seed=1))
    s = with_kernel(pf.make_factors(fp, list(range(fp.Pf)) + [fp.Pt - 1], seed=7), KINDS[kind])
    o = OracleSolver(fp, RK_HUBER)
    g0 = np.linalg.norm(pf.gradient(o, fp, s))
    ref = pf.dense_lm(o, fp, s, 40)
    assert ref["rejected"] >= 5
    h = solver(fp, s, pcg_tol=1e-12)
    got = h.optimize(40)["chi2"]
    n = min(len(got), len(ref["chi2"]))
    worst = rel(got[:n], ref["chi2"][:n]).max()
    o.set_state(*h.state())
    g1 = np.linalg.norm(pf.gradient(o, fp, s))
    q, t, _ = h.state()
    e = pf.factor_chi2(s, q, t, fp.Pf)
    print("%s: dense %d iterations, %d rejected; library %d iterations, %d trials; worst relative chi2 difference %.3g; gradient %.3g of "
          "its start; factor chi2 sum %.4g max %.4g" % (kind, len(ref["chi2"]), ref["rejected"], len(got), h.counters()["lm_trials"], worst,
                                                        g1 / g0, e.sum(), e.max()))
    # (the rejections of either side come at the optimum, where a step moves chi2 by rounding: on the CPU not before iteration 22.  Through
    # iteration 15 every step still moves chi2 by >= 1e-10 relative, six decades above the rounding of the sums, so both sides get there)
    assert n >= 15 and h.counters()["lm_trials"] > len(got)
    assert worst <= CHI2_TOL
    assert e.max() > 1e-3
    assert g1 <= 1e-6 * g0


# ---- special sets --------------------------------------------------------------------------------------------------------------------
def test_zero_information_is_no_factor(fp40):
    s = main_set(fp40)
    zero = (s[0], s[1], np.zeros_like(s[2]), s[3], None, None)
    a, b = solver(fp40), solver(fp40, zero)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)


def test_kinds_all_zero_is_no_kernel(fp40):
    s = main_set(fp40)
    n = len(s[0])
    given = s[:4] + (np.zeros(n, dtype=np.int32), np.full(n, 2.5))
    a, b = solver(fp40, s), solver(fp40, given)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.position_factor_chi_squares(), b.position_factor_chi_squares())


def test_two_factors_on_one_pose_are_one_with_the_summed_information(fp40):
    s = pf.make_factors(fp40, [31, 31], seed=9)
    z, arm = np.repeat(s[1][:1], 2, axis=0), np.repeat(s[3][:1], 2, axis=0)
    two = (s[0], z, s[2], arm, None, None)
    one = (s[0][:1], z[:1], (s[2][0] + s[2][1])[None], arm[:1], None, None)
    ca, cb = solver(fp40, one).optimize(10)["chi2"], solver(fp40, two).optimize(10)["chi2"]
    assert len(ca) == len(cb) and rel(ca, cb).max() <= 1e-9


# ---- gauge, covariance ---------------------------------------------------------------------------------------------------------------
def test_three_factors_hold_a_graph_without_a_fixed_vertex(g40):
    """every pose and landmark free: the reduced matrix has the gauge's null space (smallest eigenvalue ~1e-11 on the CPU) until three
    position fixes hold it (1.15e-3, the seventh eigenvalue of the free system).  No covariance accuracy is asserted: the condition
    number is 2.6e10."""
    g = copy.deepcopy(g40)
    g.pose_fixed[:] = False
    fp = flatten(g)
    assert fp.Pf == fp.Pt and fp.Lf == fp.Lt
    s = pf.make_factors(fp, [2, 20, 37], seed=4, sigma=0.05, arm=0.0)
    assert solver(fp).covariance(landmarks=False)["not_positive_definite"]
    assert not solver(fp, s).covariance(landmarks=False)["not_positive_definite"]


def test_covariance_includes_the_weighted_factor_terms(fp40):
    fp = fp40
    s = main_set(fp, rb.HUBER)
    h = solver(fp, s)
    h.optimize(3)
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    Hi = np.linalg.inv(pf.system(o, fp, s, 0.0)[0])
    cov = h.covariance()
    assert not cov["not_positive_definite"]
    n = 6 * fp.Pf
    for p in range(fp.Pf):
        want = Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        assert np.abs(cov["pose"][p] - want).max() <= 1e-9 * np.abs(want).max()
    for l in range(fp.Lf):
        want = Hi[n + 3 * l:n + 3 * l + 3, n + 3 * l:n + 3 * l + 3]
        assert np.abs(cov["landmark"][l] - want).max() <= 1e-9 * np.abs(want).max()
    pa, pb = int(s[0][0]), int(s[0][1])
    pairs = [("pose", pa, "landmark", 40), ("pose", pa, "pose", pb), ("landmark", 7, "landmark", 300)]
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    off = {"pose": lambda i: (6 * i, 6), "landmark": lambda i: (n + 3 * i, 3)}
    for k, (ka, a, kb, b) in enumerate(pairs):
        (ra, da), (cb, db) = off[ka](a), off[kb](b)
        want = Hi[ra:ra + da, cb:cb + db]
        assert np.abs(np.asarray(blocks[k])[:da, :db] - want).max() <= 1e-9 * np.abs(Hi).max()


# ---- life cycle and refusals ---------------------------------------------------------------------------------------------------------
def test_set_graph_clears_the_factors(fp40):
    h = solver(fp40, main_set(fp40, rb.HUBER))
    h.set_graph(fp40)
    assert len(h.position_factor_chi_squares()) == 0
    assert np.array_equal(h.optimize(5)["chi2"], solver(fp40).optimize(5)["chi2"])


def test_replacing_the_set_depends_on_state_and_set_only(fp40):
    A = main_set(fp40, rb.HUBER)
    B = with_kernel(pf.make_factors(fp40, [3, 8, 8, 30], seed=11), rb.CAUCHY)
    h = solver(fp40, A, heuristics=0)
    q, t, X = h.state()
    h.optimize(6)
    builds = h.counter("structure_builds")
    h.set_position_factors(*B)
    h.set_state(q, t, X)
    ch = h.optimize(6)["chi2"]
    assert h.counter("structure_builds") == builds
    f = solver(fp40, B, heuristics=0)
    assert np.array_equal(ch, f.optimize(6)["chi2"])
    for x, y in zip(h.state(), f.state()):
        assert np.array_equal(x, y)
    # n = 0 clears the set
    h.set_position_factors([], np.zeros((0, 3)), np.zeros((0, 3, 3)))
    h.set_state(q, t, X)
    assert np.array_equal(h.optimize(4)["chi2"], solver(fp40, heuristics=0).optimize(4)["chi2"])
    assert h.counter("structure_builds") == builds


def test_refusals_leave_a_usable_handle(fp40):
    fp = fp40
    good = with_kernel(pf.make_factors(fp, [4, 11, 11, 25, 30, 36], seed=3), rb.HUBER)
    h = solver(fp, good)
    before = h.position_factor_chi_squares()
    n = len(good[0])

    def variant(**kw):
        d = dict(pose=good[0], position=good[1], info=good[2], lever_arm=good[3], kind=good[4], delta=good[5])
        d.update(kw)
        return d["pose"], d["position"], d["info"], d["lever_arm"], d["kind"], d["delta"]

    idx = good[0].copy(); idx[2] = fp.Pt
    neg = good[0].copy(); neg[0] = -1
    nan_z = good[1].copy(); nan_z[1, 2] = np.nan
    inf_a = good[3].copy(); inf_a[4, 0] = np.inf
    inf_o = good[2].copy(); inf_o[0, 1, 1] = np.inf
    asym = good[2].copy(); asym[3, 0, 2] += 1.0
    kind4 = good[4].copy(); kind4[1] = 4
    d0 = good[5].copy(); d0[2] = 0.0
    dn = good[5].copy(); dn[2] = np.nan
    for bad in (variant(pose=idx), variant(pose=neg), variant(position=nan_z), variant(lever_arm=inf_a), variant(info=inf_o),
                variant(info=asym), variant(kind=kind4), variant(delta=d0), variant(delta=dn), variant(kind=None), variant(delta=None)):
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_position_factors(*bad)
        assert np.array_equal(h.position_factor_chi_squares(), before)
    # an asymmetry within 1e-9 of the largest entry is averaged away
    tiny = good[2].copy(); tiny[0, 0, 1] += 1e-10 * np.abs(tiny[0]).max()
    h.set_position_factors(*variant(info=tiny))
    h.set_position_factors(*good)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_partition(0, fp.Lt // 2)
    assert np.array_equal(h.position_factor_chi_squares(), before)
    p = solver(fp)
    p.set_partition(0, fp.Lt // 2)
    with pytest.raises(CubaHipError, match="status 3"):
        p.set_position_factors(*good)
    p.set_partition(0, -1)                            # (the whole graph again: the same call is accepted)
    p.set_position_factors(*good)
    assert np.array_equal(p.position_factor_chi_squares(), before)
    assert len(h.optimize(5)["chi2"]) > 0
    assert n == len(h.position_factor_chi_squares())


def test_graph_without_edges_is_refused(fp40):
    fp = fp40
    none = dataclasses.replace(fp, eP=fp.eP[:0], eL=fp.eL[:0], eDim=fp.eDim[:0], meas=fp.meas[:0], omega=fp.omega[:0], edge_src=fp.edge_src[:0])
    h = solver(none)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_position_factors(*pf.make_factors(none, [1, 2], seed=1))
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


def test_plain_batch_still_batches():
    fps = [flatten(synth_ba(40, 600, 2400, seed=s)) for s in (1, 2)]
    _, batched = optimize_batch([solver(f) for f in fps], 5)
    assert batched > 0


# ---- other builds, repeatability -----------------------------------------------------------------------------------------------------
def test_fp32_library_and_mixed_precision(fp40):
    s = main_set(fp40, rb.HUBER)
    ref = solver(fp40, s).optimize(10)["chi2"]
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
    assert np.array_equal(a.position_factor_chi_squares(), b.position_factor_chi_squares())

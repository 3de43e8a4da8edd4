"""Direction factors on the poses (cuba_hip_set_direction_factors / HipSolver.set_direction_factors) on the GPU against the numpy model of
tests/direction_factor_reference.py: the assembled system (which numbers are touched and which keep their bits), the objective, LM
trajectories against a dense fp64 LM, optimality at a non-zero residual (the bar the body-frame Jacobian -R [d]x misses), special sets,
the gauge of two position fixes plus one direction, covariances, the handle's life cycle, the refusals, batches, the other builds and
repeatability."""
import copy
import dataclasses

import numpy as np
import pytest

import direction_factor_reference as dr
import landmark_prior_reference as lr
import position_factor_reference as pfr
import robust_pose_factor_reference as rb
from conftest import RK_HUBER, with_fixed
from test_direction_factor_reference import main_set, with_kernel
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


def solver(fp, factors=None, rk=RK_HUBER, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if factors is not None:
        h.set_direction_factors(*factors)
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
        _dense[kind] = dr.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, main_set(fp40, kind), 10)["chi2"]
    return _dense[kind]


def follows(got, ref, at_least=8):
    """the per-iteration chi2 within CHI2_TOL over the iterations both ran (the dense LM on the CPU runs all 10 without a rejection)"""
    n = min(len(got), len(ref))
    worst = rel(got[:n], ref[:n]).max()
    print("%d / %d iterations, worst relative chi2 difference %.3g (bar %g)" % (len(got), len(ref), worst, CHI2_TOL))
    assert n >= at_least
    assert worst <= CHI2_TOL


# ---- assembly ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["none", "huber"])
def test_assembled_system_is_the_plain_one_plus_the_factor_terms(fp40, kind, mode):
    """the main set (two factors on pose 5, one on the fixed pose), its first factor with rank-2 information.  The off-diagonal blocks,
    the 15 entries of every diagonal block's upper triangle outside the rotation 3 x 3 and bp[3..6) / bsc[3..6) keep the plain handle's
    bits; the 6 rotation entries and bp[0..3) / bsc[0..3) are the plain handle's plus the numpy terms within 1e-12 of the block's
    (vector's) largest entry -- a missing or body-frame term stands near 1e-6 of it"""
    fp = fp40
    s = main_set(fp)
    info = s[3].copy()
    P = np.eye(3) - np.outer(s[2][0], s[2][0])
    info[0] = P @ info[0] @ P
    s = with_kernel(s[:3] + (info,), KINDS[kind])
    plain, withf = solver(fp), solver(fp, s)
    for h in (plain, withf):
        if mode == 0:
            h.build_system()
            h.assemble()
        else:
            h.set_lambda(0.0)
            h.schur()
    rp, ci, v0 = plain.hsc()
    _, _, v1 = withf.hsc()
    q = withf.state()[0]
    if kind == "huber":
        e = dr.factor_chi2(s, q, fp.Pf)
        assert (e[e > 0] < 4.0).any() and (e > 4.0).any()     # factors on both sides of delta^2
    Hd, bd = dr.factor_system(s, q, fp.Pf)
    assert not Hd[np.arange(6 * fp.Pf) % 6 >= 3].any() and not bd[np.arange(6 * fp.Pf) % 6 >= 3].any()
    diag = rp[:-1]
    off = np.setdiff1d(np.arange(len(ci)), diag)
    if mode == 1:
        assert np.array_equal(v0[off], v1[off])
    rot = np.zeros((6, 6), dtype=bool)
    rot[:3, :3] = True
    up = np.triu(np.ones((6, 6), dtype=bool))
    worst, touched = 0.0, 0
    for p in range(fp.Pf):
        a0, a1 = v0[diag[p]], v1[diag[p]]
        assert np.array_equal(a0[up & ~rot], a1[up & ~rot])
        want = a0 + Hd[6 * p:6 * p + 6, 6 * p:6 * p + 6]
        worst = max(worst, np.abs(a1[up & rot] - want[up & rot]).max() / np.abs(want[up]).max())
        touched += not np.array_equal(a0[up & rot], a1[up & rot])
    assert touched == len(np.unique(s[0][s[0] < fp.Pf]))
    print(kind, "mode", mode, "rotation entries of the diagonal blocks %.3g (bar 1e-12)" % worst)
    assert worst <= 1e-12
    for name in ("bp", "bsc")[:mode + 1]:
        a0, a1 = plain.array(name).reshape(-1, 6), withf.array(name).reshape(-1, 6)
        assert np.array_equal(a0[:, 3:], a1[:, 3:])
        want = a0 + bd.reshape(-1, 6)
        err = np.abs(a1[:, :3] - want[:, :3]).max() / np.abs(want).max()
        print(kind, "mode", mode, name, "%.3g (bar 1e-12)" % err)
        assert err <= 1e-12
        assert np.abs(bd).max() >= 1e-6 * np.abs(want).max()          # (the terms are far above the bar: a missing one would show)


# ---- objective -----------------------------------------------------------------------------------------------------------------------
def test_objective_and_factor_chi_squares(fp40):
    fp = fp40
    s = with_kernel(dr.make_factors(fp, [2, 9, fp.Pt - 1, 30, 9], seed=2), rb.HUBER)
    plain, withf = solver(fp), solver(fp, s)
    q = withf.state()[0]
    want = dr.factor_chi2(s, q, fp.Pf)
    got = withf.direction_factor_chi_squares()
    assert got[2] == 0.0 and want[2] == 0.0                       # the factor on the fixed pose is ignored
    assert np.abs(got - want).max() <= 1e-10 * want.max()
    F = withf.compute_errors()
    assert abs(F - (plain.compute_errors() + dr.factor_objective(s, q, fp.Pf))) <= 1e-12 * F
    # lambda_0 includes the factors: the maximum diagonal is that of Hpp + their terms
    assert withf.max_diagonal() >= plain.max_diagonal()


# ---- LM parity against the dense reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_lm_follows_the_dense_reference(fp40, kind):
    s = main_set(fp40, KINDS[kind])
    h = solver(fp40, s)
    follows(h.optimize(10)["chi2"], dense_ref(fp40, KINDS[kind]))
    # the per-factor chi2 and the objective at the result
    q = h.state()[0]
    want = dr.factor_chi2(s, q, fp40.Pf)
    assert np.abs(h.direction_factor_chi_squares() - want).max() <= 1e-10 * want.max()
    plain = solver(fp40)
    plain.set_state(*h.state())
    F = h.compute_errors()
    assert abs(F - (plain.compute_errors() + dr.factor_objective(s, q, fp40.Pf))) <= 1e-12 * F


OPTIONS = {"exact": {"reduced_solver": 1}, "upper": {"spmv_upper": 1}, "profile": {"profile": 1}}


@pytest.mark.parametrize("case", sorted(OPTIONS))
def test_lm_follows_the_dense_reference_under_options(fp40, case):
    follows(solver(fp40, main_set(fp40, rb.HUBER), **OPTIONS[case]).optimize(10)["chi2"], dense_ref(fp40, rb.HUBER))


def test_shuffled_pose_ids_follow_the_dense_reference(g40):
    fp = flatten(shuffled_pose_ids(g40, seed=1))
    assert not np.array_equal(fp.eP, flatten(g40).eP)
    s = main_set(fp, rb.HUBER)
    follows(solver(fp, s).optimize(10)["chi2"], dr.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_motion_only_follows_the_dense_reference(g40):
    fp = flatten(with_fixed(g40, fixed_lm_rows=range(g40.nlandmarks)))
    assert fp.Lf == 0
    s = main_set(fp, rb.CAUCHY)
    follows(solver(fp, s).optimize(10)["chi2"], dr.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_with_every_other_kind_of_factor(fp40):
    """pose priors, a relative-pose edge, landmark priors and position factors on one handle: the direction factors' launch is the last"""
    fp = fp40
    s = main_set(fp, rb.CAUCHY)
    pri = make_pose_priors(fp, [1, 5, 17], seed=1)
    edges = make_rel(fp, [(3, 20)], seed=2)
    lmp = lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0)
    pos = pfr.make_factors(fp, [5, 8, 22], seed=4, kind=rb.HUBER, delta=2.0)
    ref = dr.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10, pf=pos, lmp=lmp, priors=pri, rel=edges)["chi2"]
    h = solver(fp, s)
    h.set_pose_priors(*pri)
    h.set_relative_pose_edges(*edges)
    h.set_landmark_priors(*lmp)
    h.set_position_factors(*pos)
    follows(h.optimize(10)["chi2"], ref)


# ---- optimality --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_vanishing_gradient_at_a_non_zero_residual(kind):
    """synth_ba(12, 96, 400, seed=1), one factor on every free pose plus one on the fixed pose, make_factors(seed=7), 80 iterations
    allowed.  On the CPU (tests/test_direction_factor_reference.py) the dense LM with the right Jacobian ends at 1.1e-9 / 1.0e-11 /
    2.6e-10 / 1.1e-10 of the start gradient (none / Huber / Tukey / Cauchy), the factors' e summing to about 15 (largest 5.7): a
    genuinely non-zero residual.  With the body-frame -R [d]x in the system it stalls at 4.0e-4 / 3.8e-4 / 3.3e-4 / 2.6e-4.  The bar 1e-6
    sits 260 x below the wrong Jacobian's best result and 900 x above the right one's worst."""
    fp = flatten(synth_ba(12, 96, 400, seed=1))
    s = with_kernel(dr.make_factors(fp, list(range(fp.Pf)) + [fp.Pt - 1], seed=7), KINDS[kind])
    o = OracleSolver(fp, RK_HUBER)
    g0 = np.linalg.norm(dr.gradient(o, fp, s))
    ref = dr.dense_lm(o, fp, s, 80)
    h = solver(fp, s, pcg_tol=1e-12)
    got = h.optimize(80)["chi2"]
    n = min(len(got), len(ref["chi2"]))
    # (at the optimum a step moves chi2 by rounding and either side may accept or reject it: the series are compared over the iterations
    # both ran, rounding of the sums ~1e-13 against the bar 1e-6)
    worst = rel(got[:n], ref["chi2"][:n]).max()
    o.set_state(*h.state())
    g1 = np.linalg.norm(dr.gradient(o, fp, s))
    e = dr.factor_chi2(s, h.state()[0], fp.Pf)
    print("%s: dense %d iterations, %d rejected; library %d iterations, %d trials; worst relative chi2 difference %.3g; gradient %.3g of "
          "its start; factor chi2 sum %.4g max %.4g" % (kind, len(ref["chi2"]), ref["rejected"], len(got), h.counters()["lm_trials"], worst,
                                                        g1 / g0, e.sum(), e.max()))
    assert n >= 8
    assert worst <= CHI2_TOL
    assert e.max() > 1e-3
    assert g1 <= 1e-6 * g0


# ---- special sets --------------------------------------------------------------------------------------------------------------------
def test_zero_information_is_no_factor(fp40):
    s = main_set(fp40)
    zero = s[:3] + (np.zeros_like(s[3]), None, None)
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
    assert np.array_equal(a.direction_factor_chi_squares(), b.direction_factor_chi_squares())


def test_two_factors_on_one_pose_are_one_with_the_summed_information(fp40):
    s = dr.make_factors(fp40, [31, 31], seed=9)
    d, m = np.repeat(s[1][:1], 2, axis=0), np.repeat(s[2][:1], 2, axis=0)
    two = (s[0], d, m, s[3], None, None)
    one = (s[0][:1], d[:1], m[:1], (s[3][0] + s[3][1])[None], None, None)
    ca, cb = solver(fp40, one).optimize(10)["chi2"], solver(fp40, two).optimize(10)["chi2"]
    assert len(ca) == len(cb) and rel(ca, cb).max() <= 1e-9


# ---- gauge, covariance ---------------------------------------------------------------------------------------------------------------
def test_two_fixes_and_one_direction_hold_a_graph_without_a_fixed_vertex(g40):
    """every pose and landmark free, position fixes on poses 2 and 37 and one direction factor on pose 20: the reduced matrix is positive
    definite (smallest eigenvalue 0.45 of a largest 1.9e7 on the CPU) and the pose covariances are the dense inverse's within 1e-6 of the
    largest entry (condition number 4e7 x eps ~ 5e-9, a margin of 200).  "Not positive definite" is NOT asserted for the two fixes alone:
    the sign of that pivot (-8.6e-11 on the CPU) is rounding."""
    g = copy.deepcopy(g40)
    g.pose_fixed[:] = False
    fp = flatten(g)
    assert fp.Pf == fp.Pt and fp.Lf == fp.Lt
    fixes = pfr.make_factors(fp, [2, 37], seed=4, sigma=0.05, arm=0.0)
    one = dr.make_factors(fp, [20], seed=8)
    h = solver(fp, one)
    h.set_position_factors(*fixes)
    cov = h.covariance(landmarks=False)
    assert not cov["not_positive_definite"]
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    Hi = np.linalg.inv(dr.system(o, fp, one, 0.0, pf=fixes)[0])
    n = 6 * fp.Pf
    worst = max(np.abs(cov["pose"][p] - Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() for p in range(fp.Pf)) / np.abs(Hi[:n, :n]).max()
    print("pose covariance blocks against the dense inverse: %.3g of the largest entry (bar 1e-6)" % worst)
    assert worst <= 1e-6


def test_covariance_includes_the_weighted_factor_terms(fp40):
    fp = fp40
    s = main_set(fp, rb.HUBER)
    h = solver(fp, s)
    h.optimize(3)
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    Hi = np.linalg.inv(dr.system(o, fp, s, 0.0)[0])
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
    # (the factors are in it: without them the pose blocks differ far beyond the bar)
    Hplain = np.linalg.inv(dr.system(o, fp, None, 0.0)[0])
    assert np.abs(Hplain[6 * pa:6 * pa + 6, 6 * pa:6 * pa + 6] - Hi[6 * pa:6 * pa + 6, 6 * pa:6 * pa + 6]).max() > 1e-6 * np.abs(Hi[6 * pa:6 * pa + 6, 6 * pa:6 * pa + 6]).max()


# ---- life cycle and refusals ---------------------------------------------------------------------------------------------------------
def test_set_graph_clears_the_factors(fp40):
    h = solver(fp40, main_set(fp40, rb.HUBER))
    h.set_graph(fp40)
    assert len(h.direction_factor_chi_squares()) == 0
    assert np.array_equal(h.optimize(5)["chi2"], solver(fp40).optimize(5)["chi2"])


def test_replacing_the_set_depends_on_state_and_set_only(fp40):
    A = main_set(fp40, rb.HUBER)
    B = with_kernel(dr.make_factors(fp40, [3, 8, 8, 30], seed=11), rb.CAUCHY)
    h = solver(fp40, A, heuristics=0)
    q, t, X = h.state()
    h.optimize(6)
    builds = h.counter("structure_builds")
    h.set_direction_factors(*B)
    h.set_state(q, t, X)
    ch = h.optimize(6)["chi2"]
    assert h.counter("structure_builds") == builds
    f = solver(fp40, B, heuristics=0)
    assert np.array_equal(ch, f.optimize(6)["chi2"])
    for x, y in zip(h.state(), f.state()):
        assert np.array_equal(x, y)
    # n = 0 clears the set
    h.set_direction_factors([], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3, 3)))
    h.set_state(q, t, X)
    assert np.array_equal(h.optimize(4)["chi2"], solver(fp40, heuristics=0).optimize(4)["chi2"])
    assert h.counter("structure_builds") == builds


def test_refusals_leave_a_usable_handle(fp40):
    fp = fp40
    good = with_kernel(dr.make_factors(fp, [4, 11, 11, 25, 30, 36], seed=3), rb.HUBER)
    h = solver(fp, good)
    before = h.direction_factor_chi_squares()
    n = len(good[0])

    def variant(**kw):
        d = dict(pose=good[0], world_dir=good[1], measured_dir=good[2], info=good[3], kind=good[4], delta=good[5])
        d.update(kw)
        return d["pose"], d["world_dir"], d["measured_dir"], d["info"], d["kind"], d["delta"]

    idx = good[0].copy(); idx[2] = fp.Pt
    neg = good[0].copy(); neg[0] = -1
    nan_d = good[1].copy(); nan_d[1, 2] = np.nan
    inf_m = good[2].copy(); inf_m[4, 0] = np.inf
    inf_o = good[3].copy(); inf_o[0, 1, 1] = np.inf
    asym = good[3].copy(); asym[3, 0, 2] += 1.0
    kind4 = good[4].copy(); kind4[1] = 4
    kindn = good[4].copy(); kindn[1] = -1
    d0 = good[5].copy(); d0[2] = 0.0
    dn = good[5].copy(); dn[2] = np.nan
    for bad in (variant(pose=idx), variant(pose=neg), variant(world_dir=nan_d), variant(measured_dir=inf_m), variant(info=inf_o),
                variant(info=asym), variant(kind=kind4), variant(kind=kindn), variant(delta=d0), variant(delta=dn), variant(kind=None),
                variant(delta=None)):
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_direction_factors(*bad)
        assert np.array_equal(h.direction_factor_chi_squares(), before)
    # an asymmetry within 1e-9 of the largest entry is averaged away
    tiny = good[3].copy(); tiny[0, 0, 1] += 1e-10 * np.abs(tiny[0]).max()
    h.set_direction_factors(*variant(info=tiny))
    h.set_direction_factors(*good)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_partition(0, fp.Lt // 2)
    assert np.array_equal(h.direction_factor_chi_squares(), before)
    p = solver(fp)
    p.set_partition(0, fp.Lt // 2)
    with pytest.raises(CubaHipError, match="status 3"):
        p.set_direction_factors(*good)
    p.set_partition(0, -1)                            # (the whole graph again: the same call is accepted)
    p.set_direction_factors(*good)
    assert np.array_equal(p.direction_factor_chi_squares(), before)
    assert len(h.optimize(5)["chi2"]) > 0
    assert n == len(h.direction_factor_chi_squares())


def test_graph_without_edges_is_refused(fp40):
    fp = fp40
    none = dataclasses.replace(fp, eP=fp.eP[:0], eL=fp.eL[:0], eDim=fp.eDim[:0], meas=fp.meas[:0], omega=fp.omega[:0], edge_src=fp.edge_src[:0])
    h = solver(none)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_direction_factors(*dr.make_factors(none, [1, 2], seed=1))
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
    assert rel(ref[:k], plain[:k]).max() > 1e-4          # (the factors' share of chi2, 15 ... 44 of ~1e4: far above the bar below)
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
    assert np.array_equal(a.direction_factor_chi_squares(), b.direction_factor_chi_squares())

"""Range factors between two poses (cuba_hip_set_pose_range_factors / HipSolver.set_pose_range_factors) on the GPU against the numpy
model of tests/pose_range_factor_reference.py: the assembled system (which numbers are touched and which keep their bits; the store-or-add
rule of the off-diagonal blocks, with and without relative-pose edges on the same blocks), the topology (the union of the two binary
kinds' pairs), the objective, LM trajectories against a dense fp64 LM, optimality at a non-zero residual with rejected trials (the bar the
three wrong Jacobians miss), the point rho = 0, the scale of a monocular graph with its covariances, batches, the other builds,
repeatability, the handle's life cycle, the refusals, and the smallest shapes at which the launch geometry changes.  The bars are those of
tests/test_gpu_position_factors.py and tests/test_gpu_relative_pose.py: assembled terms 1e-12, chi2 series 1e-6, host loop against
device-decision loop 1e-9, covariances 1e-9, other builds 1e-5."""
import dataclasses
import math

import numpy as np
import pytest

import direction_factor_reference as dr
import landmark_prior_reference as lr
import pose_range_factor_reference as pp
import position_factor_reference as pfr
import range_factor_reference as rr
import robust_pose_factor_reference as rb
from conftest import RK_HUBER
from test_gpu_configs import shuffled_pose_ids
from test_gpu_pose_priors import make_priors as make_pose_priors
from test_gpu_relative_pose import block_index, block_set, internal_position, make_rel, split_pairs
from test_pose_range_factor_reference import main_pairs, main_set, optimality_case, scale_case, state0, with_kernel
from test_range_factor_reference import GRADIENT_BAR, OPT_ITERATIONS

from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle.oracle import OracleSolver

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
KINDS = {"none": rb.NONE, "huber": rb.HUBER, "tukey": rb.TUKEY, "cauchy": rb.CAUCHY}
UP = np.triu(np.ones((6, 6), dtype=bool))
EMPTY = ([], [], np.zeros(0), np.zeros(0))
NO_REL = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4)), np.zeros((0, 3)), np.zeros((0, 6, 6)))


def solver(fp, factors=None, rel=None, rel_first=True, rk=RK_HUBER, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if rel is not None and rel_first:
        h.set_relative_pose_edges(*rel)
    if factors is not None:
        h.set_pose_range_factors(*factors)
    if rel is not None and not rel_first:
        h.set_relative_pose_edges(*rel)
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
        _dense[kind] = pp.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, main_set(fp40, kind), 10)["chi2"]
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


def check_assembled(fp, s, mode, label, edges=None, rel_first=True):
    """(with factors) - (without) against the model's terms, block by block in the caller's numbering (a block the factors' pairs added to
    the pattern counts as zeros before).  Touched: the upper triangle of the diagonal block and bp (mode 1: bsc too) of every free end, and
    in mode 1 the off-diagonal block of every free-free pair -- within 1e-12 of the block's (vector's) largest entry.  Every other number
    keeps the bits of the handle without the factors: the other blocks (those of the relative-pose edges `edges` included, which both
    handles carry), the lower triangles, the entries of the other poses, and in mode 0 every off-diagonal block."""
    plain, withf = solver(fp, None, edges), solver(fp, s, edges, rel_first)
    for h in (plain, withf):
        assembled(h, mode)
    _, _, v0 = plain.hsc()
    _, _, v1 = withf.hsc()
    i0, i1 = block_index(plain), block_index(withf)
    assert set(i0) <= set(i1)
    q, t, _ = withf.state()
    Hd, bd = pp.factor_system(s, q, t, fp.Pf)
    have = np.zeros(fp.Pf, dtype=bool)
    pairs = set()
    for i, j in zip(s[0], s[1]):
        i, j = int(i), int(j)
        have[[p for p in (i, j) if p < fp.Pf]] = True
        if i < fp.Pf and j < fp.Pf:
            pairs.add((min(i, j), max(i, j)))
    assert pairs <= set(i1)
    worst, worst_off = 0.0, 0.0
    for key, k1 in i1.items():
        base = v0[i0[key]] if key in i0 else np.zeros((6, 6))
        a, b = key
        want = base + Hd[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        if a == b:
            assert np.array_equal(v1[k1][~UP], base[~UP]), key
            if not have[a]:
                assert np.array_equal(v1[k1], base), key
                continue
            assert not np.array_equal(v1[k1][UP], base[UP]), key
            worst = max(worst, np.abs(v1[k1][UP] - want[UP]).max() / np.abs(want[UP]).max())
        elif mode == 1 and key in pairs:
            assert not np.array_equal(v1[k1], base), key
            worst_off = max(worst_off, np.abs(v1[k1] - want).max() / np.abs(want).max())
        else:
            assert np.array_equal(v1[k1], base), key
    print(label, "mode", mode, "diagonal blocks %.3g, off-diagonal blocks %.3g (bar 1e-12)" % (worst, worst_off))
    assert np.isfinite(v1).all()
    assert worst <= 1e-12 and worst_off <= 1e-12
    for name in ("bp", "bsc")[:mode + 1]:
        a0, a1 = plain.array(name).reshape(-1, 6), withf.array(name).reshape(-1, 6)
        assert np.array_equal(a0[~have], a1[~have])
        want = a0 + bd.reshape(-1, 6)
        err = np.abs(a1 - want).max() / np.abs(want).max()
        print(label, "mode", mode, name, "%.3g (bar 1e-12)" % err)
        assert err <= 1e-12
        assert np.abs(bd).max() >= 1e-6 * np.abs(want).max()          # (the terms are far above the bar: a missing one would show)
    return withf


def assembly_pairs(fp):
    """a block with Schur products, a block without (twice more, once as (j, i): several factors on one block), another block without
    given as (j, i), two more factors on pose near[0][0], a fixed end in either seat"""
    near, far = split_pairs(fp, 4, 3)
    fixed = fp.Pt - 1
    assert fixed >= fp.Pf
    a = near[0][0]
    others = [p for p in range(fp.Pf) if p != a][:2]
    return near, far, [near[0], far[0], (far[1][1], far[1][0]), (far[0][1], far[0][0]), far[0], (a, others[0]), (others[1], a), (5, fixed), (fixed, 9)]


# ---- assembly ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["none", "huber"])
def test_assembled_system_is_the_plain_one_plus_the_factor_terms(fp40, kind, mode):
    """no relative-pose edges: a block without Schur products has this kind's gather as its only writer (the store), one with products is
    added to -- a stale or doubled block, a missing term or a wrong Jacobian stands near 1e-6 of the block"""
    _, far, pairs = assembly_pairs(fp40)
    s = with_kernel(pp.make_factors(fp40, pairs, seed=6, sigma=0.2 if kind == "huber" else 0.05), KINDS[kind])
    if kind == "huber":
        e = pp.factor_chi2(s, *state0(fp40), fp40.Pf)
        assert (e[e > 0] < 4.0).any() and (e > 4.0).any()     # factors on both sides of delta^2
    h = check_assembled(fp40, s, mode, kind)
    assert block_set(h) == block_set(HipSolver(fp40, RK_HUBER)) | {far[0], far[1]}
    # a second linearisation of the same handle: the stored blocks are stored again, not added to
    _, _, v = h.hsc()
    assembled(h, mode)
    assert np.array_equal(h.hsc()[2], v)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rel_first", [True, False])
def test_assembled_system_next_to_relative_pose_edges(fp40, mode, rel_first):
    """relative-pose edges on far[0] (a block without products that both kinds write: the relative-pose gather stores, this kind's adds),
    near[1] and far[2] (a block of the edges alone: it keeps its bits); far[1] stays this kind's alone (the store).  Set before the factors
    and after them: the per-block flag follows the relative-pose set"""
    near, far, pairs = assembly_pairs(fp40)
    edges = make_rel(fp40, [far[0], near[1], (far[2][1], far[2][0])], seed=2)
    s = with_kernel(pp.make_factors(fp40, pairs + [near[1]], seed=7), rb.CAUCHY)
    h = check_assembled(fp40, s, mode, "edges first" if rel_first else "edges last", edges, rel_first)
    assert block_set(h) == block_set(HipSolver(fp40, RK_HUBER)) | set(far[:3])
    # the edges leave: far[0] is this kind's alone now (the store), far[2] leaves the pattern
    h.set_relative_pose_edges(*NO_REL)
    check = check_assembled(fp40, s, mode, "edges gone")
    assembled(h, mode)
    assert np.array_equal(h.hsc()[2], check.hsc()[2]) and block_set(h) == block_set(check)


@pytest.mark.parametrize("mode", [0, 1])
def test_assembled_system_with_shuffled_pose_ids(mode):
    """an active internal reorder: the internal pairs differ from the caller's; two pairs come in both orientations, so whatever the
    internal order some factors have internal i > j and some i < j.  (200 poses: the library renumbers only graphs of 48 free poses or
    more whose blocks lie mostly far off the diagonal -- the 60-pose shuffled graph of the relative-pose tests stays in the caller's order;
    this is the shape at which tests/test_gpu_relative_pose.py sees the renumbering.  Only the factors' part of the model is dense.)"""
    fp = flatten(shuffled_pose_ids(synth_ba(200, 3000, 12000, seed=2), seed=1))
    near, far = split_pairs(fp, 3, 3)
    pairs = [near[0], far[0], (far[0][1], far[0][0]), (far[1][1], far[1][0]), far[2], (near[1][1], near[1][0]), (near[0][1], near[0][0]), (near[2][0], fp.Pt - 1)]
    s = with_kernel(pp.make_factors(fp, pairs, seed=3), rb.HUBER)
    h = check_assembled(fp, s, mode, "shuffled", make_rel(fp, [far[2], near[0]], seed=4))
    pos = internal_position(h, fp.Pf)
    assert not np.array_equal(pos, np.arange(fp.Pf))                  # (the renumbering took place)
    flipped = [pos[i] > pos[j] for i, j in pairs[:-1]]
    assert any(flipped) and not all(flipped)


def test_both_ends_fixed_is_ignored_and_one_fixed_end_acts_on_the_other():
    g = synth_ba(40, 600, 2400, seed=1)
    g.pose_fixed[:2] = True
    fp = flatten(g)
    assert fp.Pt - fp.Pf == 2
    F0, F1 = fp.Pt - 2, fp.Pt - 1
    s = with_kernel(pp.make_factors(fp, [(F0, F1), (2, F0), (F1, 2), (F1, F0)], seed=2), rb.HUBER)
    for mode in (0, 1):
        h = check_assembled(fp, s, mode, "fixed ends")
    chi = h.pose_range_factor_chi_squares()
    assert chi[0] == 0.0 and chi[3] == 0.0 and (chi[1:3] > 0).all()
    assert block_set(h) == block_set(HipSolver(fp, RK_HUBER))
    # only factors between fixed poses: nothing is launched for them, the run is the plain one
    only = tuple(x[[0, 3]] for x in s)
    a, b = solver(fp), solver(fp, only)
    assert not b.pose_range_factor_chi_squares().any()
    assert np.array_equal(a.optimize(6)["chi2"], b.optimize(6)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)


# ---- topology ------------------------------------------------------------------------------------------------------------------------
def test_structure_is_rebuilt_exactly_when_the_union_of_pairs_changes(fp40):
    fp = fp40
    near, far = split_pairs(fp, 3, 1)
    plain = block_set(HipSolver(fp, RK_HUBER))
    h = solver(fp, pp.make_factors(fp, [far[0], near[0], (3, fp.Pt - 1)], seed=15))
    h.optimize(2)
    assert block_set(h) == plain | {far[0]}                                                     # a pair without a common landmark gains a block
    n0 = h.counter("structure_builds")
    h.set_pose_range_factors(*pp.make_factors(fp, [near[0], (far[0][1], far[0][0]), far[0]], seed=16))        # same pairs, new values and order
    h.optimize(2)
    assert h.counter("structure_builds") == n0
    h.set_relative_pose_edges(*make_rel(fp, [far[0]], seed=17))                                   # a pair the union holds already
    h.optimize(2)
    assert h.counter("structure_builds") == n0
    h.set_relative_pose_edges(*make_rel(fp, [far[0], far[1]], seed=18))                           # a new pair, from the other kind
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 1 and block_set(h) == plain | {far[0], far[1]}
    h.set_pose_range_factors(*pp.make_factors(fp, [far[2], near[0]], seed=19))                    # far[0] stays the edges', far[2] is new
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 2 and block_set(h) == plain | set(far[:3])
    h.set_pose_range_factors(*EMPTY)                                                              # clearing this kind keeps the edges' blocks
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 3 and block_set(h) == plain | {far[0], far[1]}
    assert len(h.pose_range_factor_chi_squares()) == 0
    h.set_pose_range_factors(*pp.make_factors(fp, [far[1], far[2]], seed=20))
    h.set_relative_pose_edges(*NO_REL)                                                            # clearing the edges keeps this kind's blocks
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 4 and block_set(h) == plain | {far[1], far[2]}
    h.set_graph(fp)                                                                               # a new graph clears both
    h.optimize(2)
    assert block_set(h) == plain


# ---- objective -----------------------------------------------------------------------------------------------------------------------
def test_objective_and_factor_chi_squares(fp40):
    fp = fp40
    s = main_set(fp, rb.HUBER)
    plain, withf = solver(fp), solver(fp, s)
    q, t, _ = withf.state()
    want = pp.factor_chi2(s, q, t, fp.Pf)
    got = withf.pose_range_factor_chi_squares()
    print("per-factor chi2 %.3g of the largest (bar 1e-10)" % (np.abs(got - want).max() / want.max()))
    assert np.abs(got - want).max() <= 1e-10 * want.max() and (got > 0).all()
    F = withf.compute_errors()
    assert abs(F - (plain.compute_errors() + pp.factor_objective(s, q, t, fp.Pf))) <= 1e-12 * F
    # lambda_0 includes the factors: the maximum diagonal is that of Hpp + their terms
    assert withf.max_diagonal() >= plain.max_diagonal()


# ---- LM parity against the dense reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_lm_follows_the_dense_reference(fp40, kind):
    """the PCG path, under each kernel"""
    s = main_set(fp40, KINDS[kind])
    h = solver(fp40, s)
    follows(h.optimize(10)["chi2"], dense_ref(fp40, KINDS[kind]))
    q, t, _ = h.state()
    want = pp.factor_chi2(s, q, t, fp40.Pf)
    assert np.abs(h.pose_range_factor_chi_squares() - want).max() <= 1e-10 * want.max()
    plain = solver(fp40)
    plain.set_state(*h.state())
    F = h.compute_errors()
    assert abs(F - (plain.compute_errors() + pp.factor_objective(s, q, t, fp40.Pf))) <= 1e-12 * F


OPTIONS = {"exact": {"reduced_solver": 1}, "upper": {"spmv_upper": 1}, "profile": {"profile": 1}}


@pytest.mark.parametrize("case", sorted(OPTIONS))
def test_lm_follows_the_dense_reference_under_options(fp40, case):
    follows(solver(fp40, main_set(fp40, rb.HUBER), **OPTIONS[case]).optimize(10)["chi2"], dense_ref(fp40, rb.HUBER))


def test_host_loop_is_the_device_decision_loop(fp40):
    s = main_set(fp40, rb.HUBER)
    a, b = solver(fp40, s, pcg_tol=1e-11), solver(fp40, s, pcg_tol=1e-11, profile=1)
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    print("host loop against device-decision loop: %.3g (bar 1e-9)" % rel(ca, cb).max())
    assert len(ca) == len(cb) and rel(ca, cb).max() <= 1e-9
    assert a.counters()["lm_trials"] == b.counters()["lm_trials"]


def test_shuffled_pose_ids_follow_the_dense_reference(g40):
    fp = flatten(shuffled_pose_ids(g40, seed=1))
    assert not np.array_equal(fp.eP, flatten(g40).eP)
    s = main_set(fp, rb.HUBER)
    follows(solver(fp, s).optimize(10)["chi2"], pp.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_all_seven_kinds_on_one_handle(fp40):
    """pose priors, relative-pose edges (one on a block of these factors), landmark priors, position, direction and range factors on one
    handle: this kind's launches are the last"""
    fp = fp40
    s = main_set(fp, rb.CAUCHY)
    pri = make_pose_priors(fp, [1, 5, 17], seed=1)
    edges = make_rel(fp, [(3, 20), (9, 3)], seed=2)
    lmp = lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0)
    pos = pfr.make_factors(fp, [5, 8, 22], seed=4, kind=rb.HUBER, delta=2.0)
    dirs = dr.make_factors(fp, [5, 9, 30], seed=5, kind=rb.HUBER, delta=2.0)
    rng = rr.make_factors(fp, [5, 3, 12], seed=6, kind=rb.HUBER, delta=2.0)
    ref = pp.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10, rs=rng, df=dirs, pf=pos, lmp=lmp, priors=pri, rel=edges)["chi2"]
    h = solver(fp, s)
    h.set_pose_priors(*pri)
    h.set_relative_pose_edges(*edges)
    h.set_landmark_priors(*lmp)
    h.set_position_factors(*pos)
    h.set_direction_factors(*dirs)
    h.set_range_factors(*rng)
    follows(h.optimize(10)["chi2"], ref)


# ---- rejected trials, optimality ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rejected_trials_and_a_vanishing_gradient_at_a_non_zero_residual(kind):
    """the case sized on the CPU (tests/test_pose_range_factor_reference.py: optimality_case): synth_ba(12, 96, 400, seed=1), an odometer
    chain, every pose with the one four on and the last free pose with the fixed one, distances of 1.0 ... 4.0 m with half a metre of noise
    and of arm, 120 iterations allowed.  There the dense LM with the right Jacobians ends at 7.8e-12 / 2.5e-11 / 7.7e-13 / 2.2e-11 of the
    start gradient (none / Huber / Tukey / Cauchy) with genuinely rejected trials from trial 10 on (gain ratio below -1e-3), the factors' e
    summing to 306 ... 315; with the world-frame directions it stalls at >= 1.2e-4, without the rotation columns at >= 4.3e-5, with m_i of
    the wrong sign at >= 1.6e-4.  The bar 1e-6 sits 43 x below the wrong Jacobians' best result and 40 000 x above the right ones' worst.
    A restore after a rejected trial linearises the factors at the restored poses: the chi2 series follows the dense LM over the
    iterations both ran."""
    fp, s = optimality_case(KINDS[kind])
    o = OracleSolver(fp, RK_HUBER)
    g0 = np.linalg.norm(pp.gradient(o, fp, s))
    ref = pp.dense_lm(o, fp, s, OPT_ITERATIONS)
    genuine = [i for i, x in enumerate(ref["gains"]) if x < -1e-3]
    assert genuine
    h = solver(fp, s, pcg_tol=1e-12)
    got = h.optimize(OPT_ITERATIONS)["chi2"]
    n = min(len(got), len(ref["chi2"]))
    worst = rel(got[:n], ref["chi2"][:n]).max()
    o.set_state(*h.state())
    g1 = np.linalg.norm(pp.gradient(o, fp, s))
    q, t, _ = h.state()
    e = pp.factor_chi2(s, q, t, fp.Pf)
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
def test_two_points_on_each_other_add_nothing_and_keep_their_residual(fp40, kind):
    """identity quaternions on poses 7 and 12, a_i - t_i = a_j - t_j exactly (dyadic numbers): u is exactly 0.  The rule: m_i = m_j = 0, so
    both J = 0 -- a finite system, the bits of the handle without the factor in every number but the pair's new block, which is stored as
    exact zeros; chi2 = Omega rbar^2 -- under both instantiations of the kernels; a second factor keeps its terms, and a run from there
    stays finite"""
    fp = fp40
    plain = solver(fp)
    q, t, X = plain.state()
    q, t = q.copy(), t.copy()
    q[7] = q[12] = (0.0, 0.0, 0.0, 1.0)
    t[7], t[12] = (0.25, -1.5, 3.0), (1.25, 0.5, -1.0)
    ai, aj = np.array([[0.5, 0.25, 1.0]]), np.array([[1.5, 2.25, -3.0]])
    plain.set_state(q, t, X)
    at_zero = (np.array([7], dtype=np.int32), np.array([12], dtype=np.int32), np.array([0.75]), np.array([16.0]), ai, aj)
    s = with_kernel(at_zero + (None, None), KINDS[kind])
    withf = solver(fp, s)
    withf.set_state(q, t, X)
    chi = withf.pose_range_factor_chi_squares()
    assert chi[0] == 16.0 * 0.75 ** 2
    F0, F1 = plain.compute_errors(), withf.compute_errors()
    assert abs(F1 - (F0 + rb.rho(KINDS[kind], 2.0, 9.0))) <= 1e-12 * F1
    for mode in (0, 1):
        for h in (plain, withf):
            assembled(h, mode)
        i0, i1 = block_index(plain), block_index(withf)
        v0, v1 = plain.hsc()[2], withf.hsc()[2]
        assert np.isfinite(v1).all()
        for key, k1 in i1.items():
            assert np.array_equal(v1[k1], v0[i0[key]] if key in i0 else np.zeros((6, 6))), key
        for name in ("bp", "bsc")[:mode + 1]:
            assert np.array_equal(plain.array(name), withf.array(name)) and np.isfinite(withf.array(name)).all()
    # with a second, ordinary factor on the same block and one elsewhere: those factors' terms, nothing of the first
    other = pp.make_factors(fp, [(12, 7), (3, 30)], seed=3)
    both = tuple(np.concatenate([x, y]) for x, y in zip(at_zero, other[:6]))
    two, one = solver(fp, with_kernel(both + (None, None), KINDS[kind])), solver(fp, with_kernel(other, KINDS[kind]))
    for h in (two, one):
        h.set_state(q, t, X)
        assembled(h, 1)
    assert np.array_equal(two.hsc()[2], one.hsc()[2]) and np.array_equal(two.array("bsc"), one.array("bsc"))
    chi2 = two.optimize(5)["chi2"]
    assert len(chi2) > 0 and np.isfinite(chi2).all() and all(np.isfinite(x).all() for x in two.state())


def test_zero_information_changes_the_pattern_only(fp40):
    """information 0 is valid and is no factor: the run is that of the same handle with the pairs' blocks and factors that weigh nothing --
    compared here with the dense LM of the plain graph"""
    s = main_set(fp40)
    zero = s[:3] + (np.zeros_like(s[3]),) + s[4:]
    b = solver(fp40, zero)
    assert not b.pose_range_factor_chi_squares().any()
    follows(b.optimize(10)["chi2"], pp.dense_lm(OracleSolver(fp40, RK_HUBER), fp40, None, 10)["chi2"])


def test_kinds_all_zero_is_no_kernel(fp40):
    s = main_set(fp40)
    n = len(s[0])
    given = s[:6] + (np.zeros(n, dtype=np.int32), np.full(n, 2.5))
    a, b = solver(fp40, s), solver(fp40, given)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.pose_range_factor_chi_squares(), b.pose_range_factor_chi_squares())


# ---- scale, covariance ---------------------------------------------------------------------------------------------------------------
def test_odometer_distances_hold_the_scale_of_a_monocular_graph():
    """the case sized on the CPU (tests/test_pose_range_factor_reference.py: scale_case, at the graph's initial estimate):
    synth_ba(12, 96, 400, seed=2) as a monocular graph with one fixed pose, an odometer factor on every consecutive pair, information
    1e4 ... 2e4.  The condition number of the dense Hessian there is 5.0e9 whatever the factors' information (the weakest landmark
    direction against the rotations), and the dense inverse's own error, by one step of refinement in extended precision, is 4.8e-12 of a
    block's largest entry: the bar 1e-9 is the reference's to give.  The pose and landmark covariances are the blocks of that inverse, block
    by block within 1e-9 of the block's largest entry, two covariance_pairs within 1e-9 of the inverse's largest entry; the LM run follows
    the dense LM.  Measured on the MI355X: the worst block 2.57e-10 of its largest entry (printed).  The state matters: after three LM iterations the
    same graph's condition number is 1.9e10, where the reference is as good (3.5e-12) but the library's blocks were measured at 1.48e-9 of
    the block's largest entry on the MI355X -- the selected inversion's own rounding at that condition, the figure of the unary range
    factors' gauge case (5.8e-10 at 2.6e10); this test stays at the state the set was sized for."""
    fp, s = scale_case()
    h = solver(fp, s)
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    H = pp.system(o, fp, s, 0.0)[0]
    ev = np.linalg.eigvalsh(H)
    Hi = np.linalg.inv(H)
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
    print("covariance blocks against the dense inverse: %.3g of the block's largest entry (bar 1e-9, condition number %.3g)" % (worst, ev[-1] / ev[0]))
    assert worst <= 1e-9
    pairs = [("pose", 0, "pose", fp.Pf - 1), ("pose", 3, "landmark", 40)]
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    off = {"pose": lambda i: (6 * i, 6), "landmark": lambda i: (n + 3 * i, 3)}
    for k, (ka, a, kb, b) in enumerate(pairs):
        (ra, da), (cb, db) = off[ka](a), off[kb](b)
        want = Hi[ra:ra + da, cb:cb + db]
        assert np.abs(np.asarray(blocks[k])[:da, :db] - want).max() <= 1e-9 * np.abs(Hi).max()
    # (the factors are in it: without them the scale is free and the pose blocks differ far beyond the bar)
    Hplain = pp.system(o, fp, None, 0.0)[0]
    assert np.linalg.eigvalsh(Hplain)[0] <= 1e-6 * ev[0]
    fresh = solver(fp, s)
    follows(fresh.optimize(10)["chi2"], pp.dense_lm(OracleSolver(fp, RK_HUBER), fp, s, 10)["chi2"])


def test_covariance_blocks_include_the_pairs_blocks(fp40):
    """a far pair's block is part of the pattern the covariance works on, under both covariance paths' input: the blocks of the dense
    inverse within 1e-9, and a new set invalidates the cached blocks"""
    fp = fp40
    s = main_set(fp, rb.HUBER)
    h = solver(fp, s)
    h.optimize(3)
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    Hi = np.linalg.inv(pp.system(o, fp, s, 0.0)[0])
    cov = h.covariance(landmarks=False)
    assert not cov["not_positive_definite"]
    worst = max(np.abs(cov["pose"][p] - Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() / np.abs(Hi[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() for p in range(fp.Pf))
    print("pose covariance blocks against the dense inverse: %.3g (bar 1e-9)" % worst)
    assert worst <= 1e-9
    assert len(h.covariance_blocks()) == h.counters()["hsc_blocks"]
    i, j = int(s[0][0]), int(s[1][0])
    blocks, bad = h.covariance_pairs([("pose", i, "pose", j)])
    assert not bad and np.abs(np.asarray(blocks[0]) - Hi[6 * i:6 * i + 6, 6 * j:6 * j + 6]).max() <= 1e-9 * np.abs(Hi).max()
    h.set_pose_range_factors(*main_set(fp, rb.CAUCHY))
    with pytest.raises(CubaHipError, match="status 3"):
        h.covariance_blocks()


# ---- life cycle and refusals ---------------------------------------------------------------------------------------------------------
def test_set_graph_clears_the_factors(fp40):
    h = solver(fp40, main_set(fp40, rb.HUBER))
    h.set_graph(fp40)
    assert len(h.pose_range_factor_chi_squares()) == 0
    assert np.array_equal(h.optimize(5)["chi2"], solver(fp40).optimize(5)["chi2"])


def test_replacing_the_set_depends_on_state_and_set_only(fp40):
    A = main_set(fp40, rb.HUBER)
    B = with_kernel(pp.make_factors(fp40, [(3, 8), (8, 30), (8, 3), (30, fp40.Pt - 1)], seed=11), rb.CAUCHY)
    h = solver(fp40, A, heuristics=0)
    q, t, X = h.state()
    h.optimize(6)
    h.set_pose_range_factors(*B)
    h.set_state(q, t, X)
    ch = h.optimize(6)["chi2"]
    f = solver(fp40, B, heuristics=0)
    assert np.array_equal(ch, f.optimize(6)["chi2"])
    for x, y in zip(h.state(), f.state()):
        assert np.array_equal(x, y)
    # n = 0 clears the set
    h.set_pose_range_factors(*EMPTY)
    h.set_state(q, t, X)
    assert np.array_equal(h.optimize(4)["chi2"], solver(fp40, heuristics=0).optimize(4)["chi2"])


def test_refusals_leave_a_usable_handle(fp40):
    fp = fp40
    good = with_kernel(pp.make_factors(fp, [(4, 11), (11, 25), (25, 4), (30, 36), (36, fp.Pt - 1), (2, 30)], seed=3), rb.HUBER)
    h = solver(fp, good)
    before = h.pose_range_factor_chi_squares()
    n = len(good[0])
    names = ("pose_i", "pose_j", "range", "info", "lever_arm_i", "lever_arm_j", "kind", "delta")

    def variant(**kw):
        d = dict(zip(names, good))
        d.update(kw)
        return tuple(d[k] for k in names)

    def changed(x, at, value):
        x = x.copy()
        x[at] = value
        return x

    bads = [variant(pose_i=changed(good[0], 2, fp.Pt)), variant(pose_i=changed(good[0], 0, -1)), variant(pose_j=changed(good[1], 3, fp.Pt)),
            variant(pose_j=changed(good[1], 1, -1)), variant(pose_j=changed(good[1], 0, good[0][0])),
            variant(lever_arm_i=changed(good[4], (1, 2), np.nan)), variant(lever_arm_j=changed(good[5], (4, 0), np.inf)),
            variant(range=changed(good[2], 3, np.nan)), variant(range=changed(good[2], 3, np.inf)), variant(range=changed(good[2], 5, -1e-3)),
            variant(info=changed(good[3], 0, np.inf)), variant(info=changed(good[3], 1, np.nan)), variant(info=changed(good[3], 2, -1.0)),
            variant(kind=changed(good[6], 1, 4)), variant(kind=changed(good[6], 1, -1)), variant(delta=changed(good[7], 2, 0.0)),
            variant(delta=changed(good[7], 2, -1.0)), variant(delta=changed(good[7], 2, np.nan)), variant(kind=None), variant(delta=None)]
    builds = h.counter("structure_builds")
    for bad in bads:
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_pose_range_factors(*bad)
        assert np.array_equal(h.pose_range_factor_chi_squares(), before)
    assert h.counter("structure_builds") == builds          # (a refused set leaves the pairs as they were)
    # a zero range, a zero information and absent arms are valid
    h.set_pose_range_factors(*variant(range=changed(good[2], 0, 0.0), info=changed(good[3], 1, 0.0), lever_arm_i=None, lever_arm_j=None))
    assert h.pose_range_factor_chi_squares()[1] == 0.0
    h.set_pose_range_factors(*good)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_partition(0, fp.Lt // 2)
    assert np.array_equal(h.pose_range_factor_chi_squares(), before)
    p = solver(fp)
    p.set_partition(0, fp.Lt // 2)
    with pytest.raises(CubaHipError, match="status 3"):
        p.set_pose_range_factors(*good)
    p.set_partition(0, -1)                            # (the whole graph again: the same call is accepted)
    p.set_pose_range_factors(*good)
    assert np.array_equal(p.pose_range_factor_chi_squares(), before)
    assert len(h.optimize(5)["chi2"]) > 0
    assert n == len(h.pose_range_factor_chi_squares())


def test_graph_without_reprojection_edges_is_refused(fp40):
    fp = fp40
    none = dataclasses.replace(fp, eP=fp.eP[:0], eL=fp.eL[:0], eDim=fp.eDim[:0], meas=fp.meas[:0], omega=fp.omega[:0], edge_src=fp.edge_src[:0])
    h = solver(none)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_pose_range_factors(*pp.make_factors(none, [(1, 2)], seed=1))
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
    edges = make_rel(fp40, [tuple(main_pairs(fp40)[0]), (3, 9)], seed=5)
    a, b = solver(fp40, s, edges), solver(fp40, s, edges)
    assert np.array_equal(a.optimize(10)["chi2"], b.optimize(10)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.pose_range_factor_chi_squares(), b.pose_range_factor_chi_squares())


# ---- the smallest shapes where the launch geometry changes ---------------------------------------------------------------------------
def check_chi_squares(fp, s, label):
    """the per-factor chi2 and the objective of a set against the model"""
    plain, withf = solver(fp), solver(fp, s)
    q, t, _ = withf.state()
    terms = pp.factor_terms(s, q, t, fp.Pf)
    want = np.array([x[0] for x in terms])
    got = withf.pose_range_factor_chi_squares()
    print(label, "%d factors: per-factor chi2 %.3g of the largest (bar 1e-10)" % (len(want), np.abs(got - want).max() / want.max()))
    assert len(got) == len(want) and np.abs(got - want).max() <= 1e-10 * want.max()
    assert np.array_equal(got == 0, want == 0)
    F = withf.compute_errors()
    assert abs(F - (plain.compute_errors() + math.fsum(x[1] for x in terms))) <= 1e-12 * F


def distinct_pairs(fp, n, seed):
    """n distinct free-free pairs, in a random order and orientation"""
    rng = np.random.default_rng(seed)
    every = [(a, b) for a in range(fp.Pf) for b in range(a + 1, fp.Pf)]
    return [every[k] if rng.uniform() < 0.5 else every[k][::-1] for k in rng.choice(len(every), n, replace=False)]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_factor_counts_about_one_linearise_workgroup(fp40, n):
    """the linearisation runs 64 lanes per workgroup, one per factor with a free end: 63, 64 and 65 of them, the last with a fixed end"""
    pairs = distinct_pairs(fp40, n - 1, seed=n) + [(fp40.Pt - 1, 6)]
    check_assembled(fp40, with_kernel(pp.make_factors(fp40, pairs, seed=12), rb.HUBER), 1, "%d factors" % n)


@pytest.mark.parametrize("mode,poses,blocks", [(1, 4, 4), (1, 7, 2), (0, 9, 0), (0, 10, 0)])
def test_gather_counts_about_one_workgroup(fp40, mode, poses, blocks):
    """the gather runs 256 lanes per workgroup, one per output number: 36 per block (mode 1) + 27 per free pose with factors -- multiples
    of 9, so the counts next to 256 are 252 (4 poses on a 4-cycle of blocks) and 261 (2 blocks on 4 poses + 3 poses with a fixed-end factor)
    in mode 1, 243 and 270 (9 and 10 poses) in mode 0"""
    fixed = fp40.Pt - 1
    if mode == 1 and blocks == 4:
        pairs = [(2, 11), (11, 20), (29, 20), (29, 2)]
    elif mode == 1:
        pairs = [(2, 11), (29, 20), (5, fixed), (fixed, 8), (14, fixed)]
    else:
        pairs = [(k, k + 1) for k in range(10, 10 + poses - 1)]
    s = pp.make_factors(fp40, pairs, seed=13)
    free = np.unique(np.concatenate([s[0], s[1]]))
    assert (free < fp40.Pf).sum() == poses
    assert (36 * blocks if mode == 1 else 0) + 27 * poses in (243, 252, 261, 270)
    check_assembled(fp40, s, mode, "%d numbers" % ((36 * blocks if mode == 1 else 0) + 27 * poses))


def test_257_factors_make_two_chi2_partials(fp40):
    rng = np.random.default_rng(2)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, fp40.Pt, size=(400, 2)) if a != b][:257]
    s = with_kernel(pp.make_factors(fp40, pairs, seed=13), rb.CAUCHY)
    assert len(s[0]) == 257
    check_chi_squares(fp40, s, "two partials")

"""SE(3) relative-pose edges (cuba_hip_set_relative_pose_edges / HipSolver.set_relative_pose_edges) on the GPU against the numpy model of
tests/relative_pose_reference.py: the block pattern, the assembled system, the objective, LM trajectories against a dense fp64 LM on
every solve path, poses held by relative edges alone, a loop closure with its covariances, optimality at non-zero residuals, scale, the
structure-rebuild rule, batches, the refusals and the other builds.

Bars: the project's own for the same quantities (DESIGN sections 7a-7c): assembly 1e-12 relative, chi2 per iteration 1e-6 against the
dense LM, host loop against device-decision loop 1e-9, covariance against the dense inverse 1e-9, pair against block covariances 1e-12."""
import copy
import dataclasses

import numpy as np
import pytest

import prior_reference as pr
import relative_pose_reference as rr
from conftest import RK_HUBER, RK_NONE, RK_TUKEY
from test_gpu_configs import shuffled_pose_ids
from test_gpu_covariance import _dense_from_upper
from test_gpu_pose_priors import freed, make_priors
from test_relative_pose_reference import gradient_graph

from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba, synth_named
from oracle import oracle
from oracle.oracle import OracleSolver

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6


def make_rel(fp, pairs, seed=0, rot=0.03, trans=0.1, w_rot=4e4, w_trans=1e3, corr=True, exact=False):
    """relative-pose edges on the given (i, j) pairs (solver numbering): measurements a few degrees / a decimetre off the relative pose of
    the initial estimate, information that conflicts with the observations"""
    rng = np.random.default_rng(seed)
    q0, t0 = np.asarray(fp.q).reshape(-1, 4), np.asarray(fp.t).reshape(-1, 3)
    pi = np.array([p[0] for p in pairs], dtype=np.int32)
    pj = np.array([p[1] for p in pairs], dtype=np.int32)
    qz, tz, info = [], [], []
    for i, j in zip(pi, pj):
        z = rr.measurement(q0, t0, i, j)
        if not exact:
            z = rr.pose_mul(oracle.se3_exp(np.concatenate([rot * rng.normal(size=3), trans * rng.normal(size=3)])), z)
        qz.append(z[0]); tz.append(z[1])
        O = np.diag([w_rot] * 3 + [w_trans] * 3)
        if corr:
            A = rng.normal(size=(6, 6)) * 0.1
            O = O + np.sqrt(w_rot * w_trans) * (A @ A.T) * 0.01
        info.append(O)
    return pi, pj, np.array(qz), np.array(tz), np.array(info)


def solver(fp, rk, rel=None, priors=None, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if priors is not None:
        h.set_pose_priors(*priors)
    if rel is not None:
        h.set_relative_pose_edges(*rel)
    return h


def dense_run(fp, rk, priors, rel, niter):
    return rr.dense_lm(OracleSolver(fp, rk), fp, priors, rel, niter)


def relerr(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))


def block_set(h):
    rp, ci = h.hsc_structure()
    return {(r, int(c)) for r in range(len(rp) - 1) for c in ci[rp[r]:rp[r + 1]]}


def block_index(h):
    rp, ci = h.hsc_structure()
    return {(r, int(ci[k])): k for r in range(len(rp) - 1) for k in range(rp[r], rp[r + 1])}


def covisible(fp):
    """the pairs (a < b) of free poses that share a free landmark: the off-diagonal blocks of the plain reduced matrix"""
    eP, eL = np.asarray(fp.eP), np.asarray(fp.eL)
    keep = (eP < fp.Pf) & (eL < fp.Lf)
    order = np.argsort(eL[keep], kind="stable")
    p, l = eP[keep][order], eL[keep][order]
    out = set()
    for seg in np.split(p, np.nonzero(np.diff(l))[0] + 1):
        u = np.unique(seg)
        out |= {(int(a), int(b)) for x, a in enumerate(u) for b in u[x + 1:]}
    return out


def split_pairs(fp, n_far=2, n_near=2):
    """(pairs that share landmarks, pairs that do not) among the free poses of a graph"""
    have = covisible(fp)
    near = sorted(have)
    far = [(a, b) for a in range(fp.Pf) for b in range(a + 1, fp.Pf) if (a, b) not in have]
    assert len(far) >= n_far and len(near) >= n_near
    return near[:: max(1, len(near) // n_near)][:n_near], far[:: max(1, len(far) // n_far)][:n_far]


def drop_edges(fp, poses):
    """the flat problem without the reprojection edges of the given solver poses (tracking lost there): landmarks left with fewer than two
    observations lose theirs too and leave the problem; the poses stay"""
    eP, eL = np.asarray(fp.eP), np.asarray(fp.eL)
    keep = ~np.isin(eP, list(poses))
    while True:
        cnt = np.bincount(eL[keep], minlength=fp.Lt)
        bad = keep & (cnt[eL] < 2)
        if not bad.any():
            break
        keep &= ~bad
    alive = np.bincount(eL[keep], minlength=fp.Lt) > 0
    new_of_old = np.cumsum(alive) - 1
    return dataclasses.replace(fp, Lt=int(alive.sum()), Lf=int(alive[:fp.Lf].sum()), Xw=np.ascontiguousarray(np.asarray(fp.Xw)[alive]),
                               eP=np.ascontiguousarray(eP[keep]), eL=np.ascontiguousarray(new_of_old[eL[keep]].astype(np.int32)),
                               eDim=np.ascontiguousarray(np.asarray(fp.eDim)[keep]), meas=np.ascontiguousarray(np.asarray(fp.meas)[keep]),
                               omega=np.ascontiguousarray(np.asarray(fp.omega)[keep]), lm_src=np.asarray(fp.lm_src)[alive],
                               edge_src=np.asarray(fp.edge_src)[keep])


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


def follows_dense(fp, rk, rel, priors=None, niter=10, **opts):
    ref = dense_run(fp, rk, priors, rel, niter)
    got = solver(fp, rk, rel, priors, **opts).optimize(niter)["chi2"]
    print("chi2 per iteration vs dense LM: %d / %d iterations, max rel %.2e" % (len(got), len(ref["chi2"]), relerr(got[:len(ref["chi2"])], ref["chi2"][:len(got)]).max()))
    assert len(got) == len(ref["chi2"])
    assert relerr(got, ref["chi2"]).max() <= CHI2_TOL


# ---- structure -----------------------------------------------------------------------------------------------------------------------
def test_structure_holds_every_free_pair(g40):
    fp = flatten(g40)
    near, far = split_pairs(fp, 3, 2)
    fixed = fp.Pt - 1
    assert fixed >= fp.Pf
    pairs = [near[0], far[0], (far[1][1], far[1][0]), far[0], (3, fixed), near[1], far[2]]
    plain, h = HipSolver(fp, RK_HUBER), solver(fp, RK_HUBER, make_rel(fp, pairs, seed=1))
    b0, b1 = block_set(plain), block_set(h)
    assert b1 == b0 | set(far[:3])
    assert h.counters()["hsc_blocks"] == plain.counters()["hsc_blocks"] + 3
    assert h.counters()["schur_products"] == plain.counters()["schur_products"]


def test_no_edges_is_the_plain_handle(g40):
    fp = flatten(g40)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 4)), np.zeros((0, 3)), np.zeros((0, 6, 6)))
    runs = []
    for rel in (None, empty):
        h = solver(fp, RK_HUBER, rel)
        h.set_lambda(0.0)
        h.schur()
        rp, ci, v = h.hsc()
        res = h.optimize(10)
        runs.append((rp, ci, v, res["chi2"], h.state(), h.counters(), h.pcg_history()[0], h.counter("structure_builds")))
    a, b = runs
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3]) and a[5] == b[5] and np.array_equal(a[6], b[6]) and a[7] == b[7] == 1
    for x, y in zip(a[4], b[4]):
        assert np.array_equal(x, y)


# ---- assembly and objective ----------------------------------------------------------------------------------------------------------
def check_assembly(fp, rel):
    plain, h = solver(fp, RK_HUBER), solver(fp, RK_HUBER, rel)
    for s in (plain, h):
        s.set_lambda(0.0)
        s.schur()
    _, _, v0 = plain.hsc()
    _, _, v1 = h.hsc()
    i0, i1 = block_index(plain), block_index(h)
    q, t, _ = h.state()
    Hr, br = rr.rel_system(rel, q, t, fp.Pf)
    touched = set()
    for i, j in zip(rel[0], rel[1]):
        i, j = int(i), int(j)
        touched |= {(p, p) for p in (i, j) if p < fp.Pf}
        if i < fp.Pf and j < fp.Pf:
            touched.add((min(i, j), max(i, j)))
    worst = 0.0
    for key, k1 in i1.items():
        base = v0[i0[key]] if key in i0 else np.zeros((6, 6))
        if key not in touched:
            assert np.array_equal(v1[k1], base), key
            continue
        want = base + Hr[6 * key[0]:6 * key[0] + 6, 6 * key[1]:6 * key[1] + 6]
        sel = np.triu_indices(6) if key[0] == key[1] else (slice(None), slice(None))
        worst = max(worst, np.abs(v1[k1][sel] - want[sel]).max() / np.abs(want[sel]).max())
    for name in ("bp", "bsc"):
        a0, a1 = plain.array(name), h.array(name)
        want = a0 + br
        worst = max(worst, np.abs(a1 - want).max() / np.abs(want).max())
    print("assembled hsc / bp / bsc against plain + model: max rel %.2e" % worst)
    assert worst <= 1e-12


def test_assembled_system_is_the_plain_one_plus_the_edge_terms(g40):
    fp = flatten(g40)
    near, far = split_pairs(fp, 2, 2)
    # a co-visible pair, one that is not, two edges on one pair, an edge given as (j, i), an edge to the fixed pose
    pairs = [near[0], far[0], far[0], (far[1][1], far[1][0]), (near[1][1], near[1][0]), (5, fp.Pt - 1), (fp.Pt - 1, 9)]
    check_assembly(fp, make_rel(fp, pairs, seed=2))


def test_assembled_system_with_shuffled_pose_ids():
    fp = flatten(shuffled_pose_ids(synth_ba(60, 900, 3600, seed=2), seed=1))
    near, far = split_pairs(fp, 3, 2)
    pairs = [near[0], far[0], (far[1][1], far[1][0]), far[2], far[2], (near[1][1], near[1][0])]
    check_assembly(fp, make_rel(fp, pairs, seed=3))


def test_objective_and_chi_squares(g40):
    fp = flatten(g40)
    near, far = split_pairs(fp, 2, 1)
    fixed = fp.Pt - 1
    rel = make_rel(fp, [near[0], far[0], (far[1][1], far[1][0]), (4, fixed), (fixed, 7)], seed=4)
    plain, h = solver(fp, RK_HUBER), solver(fp, RK_HUBER, rel)
    q, t, _ = h.state()
    want = rr.rel_chi2(rel, q, t, fp.Pf)
    got = h.relative_pose_chi_squares()
    assert np.abs(got - want).max() <= 1e-10 * want.max()
    assert abs(h.compute_errors() - (plain.compute_errors() + want.sum())) <= 1e-12 * h.compute_errors()
    assert h.max_diagonal() >= plain.max_diagonal()


def test_one_end_fixed_is_the_corresponding_prior(g40):
    fp = flatten(g40)
    fixed = fp.Pt - 1
    rel = make_rel(fp, [(fixed, 3), (fixed, 11), (fixed, 11)], seed=5)
    q, t, _ = HipSolver(fp, RK_HUBER).state()
    qb, tb = [], []
    for k in range(3):
        b = rr.pose_mul((rel[2][k], rel[3][k]), (rr.unit(q[fixed]), t[fixed]))
        qb.append(b[0]); tb.append(b[1])
    pri = (rel[1], np.array(qb), np.array(tb), rel[4])
    a, b = solver(fp, RK_HUBER, rel), solver(fp, RK_HUBER, None, pri)
    assert np.abs(a.relative_pose_chi_squares() - b.prior_chi_squares()).max() <= 1e-12 * b.prior_chi_squares().max()
    for s in (a, b):
        s.set_lambda(0.0)
        s.schur()
    va, vb = a.hsc()[2], b.hsc()[2]
    assert np.abs(va - vb).max() <= 1e-12 * np.abs(vb).max()
    for name in ("bp", "bsc"):
        assert np.abs(a.array(name) - b.array(name)).max() <= 1e-12 * np.abs(b.array(name)).max()
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    assert len(ca) == len(cb) and relerr(ca, cb).max() <= 1e-9


def test_both_ends_fixed_is_ignored():
    g = synth_ba(40, 600, 2400, seed=1)
    g.pose_fixed[[0, 1]] = True
    fp = flatten(g)
    assert fp.Pt - fp.Pf == 2
    rel = make_rel(fp, [(fp.Pt - 1, fp.Pt - 2)], seed=6)
    a, b = solver(fp, RK_HUBER), solver(fp, RK_HUBER, rel)
    assert np.array_equal(b.relative_pose_chi_squares(), [0.0])
    assert a.compute_errors() == b.compute_errors()
    assert np.array_equal(a.optimize(6)["chi2"], b.optimize(6)["chi2"])
    for x, y in zip(a.state(), b.state()):
        assert np.array_equal(x, y)


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


def mixed_pairs(fp, seed):
    near, far = split_pairs(fp, 4, 3)
    rng = np.random.default_rng(seed)
    pairs = near + far + [far[0], (far[1][1], far[1][0])]
    if fp.Pt > fp.Pf:
        pairs.append((fp.Pt - 1, int(rng.integers(0, fp.Pf))))
    return pairs


@pytest.mark.parametrize("case", sorted(CASES))
def test_lm_follows_the_dense_reference(g40, case):
    rk, opts = CASES[case]
    fp = flatten(g40)
    follows_dense(fp, rk, make_rel(fp, mixed_pairs(fp, 7), seed=7), **opts)


def test_shuffled_pose_ids_follow_the_dense_reference():
    fp = flatten(shuffled_pose_ids(synth_ba(60, 900, 3600, seed=2), seed=1))
    follows_dense(fp, RK_HUBER, make_rel(fp, mixed_pairs(fp, 8), seed=8))


def test_motion_only_follows_the_dense_reference(g40):
    from conftest import with_fixed
    fp = flatten(with_fixed(g40, fixed_lm_rows=range(g40.nlandmarks)))
    assert fp.Lf == 0 and not covisible(fp)          # (no free landmark: every off-diagonal block is a relative one)
    follows_dense(fp, RK_HUBER, make_rel(fp, mixed_pairs(flatten(g40), 9), seed=9))


def test_with_priors_and_without_a_fixed_pose(g40):
    fp = flatten(freed(g40))
    assert fp.Pf == fp.Pt
    pri = make_priors(fp, [0, 13], seed=10)          # (the gauge is held by the priors)
    follows_dense(fp, RK_HUBER, make_rel(fp, mixed_pairs(fp, 10), seed=10), pri)


def test_host_loop_is_the_device_decision_loop(g40):
    fp = flatten(g40)
    rel = make_rel(fp, mixed_pairs(fp, 11), seed=11)
    a, b = solver(fp, RK_HUBER, rel, pcg_tol=1e-11), solver(fp, RK_HUBER, rel, pcg_tol=1e-11, profile=1)
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    assert len(ca) == len(cb) and relerr(ca, cb).max() <= 1e-9
    assert a.counters()["lm_trials"] == b.counters()["lm_trials"]


# ---- poses held by relative edges alone ---------------------------------------------------------------------------------------------
def test_pose_without_observations_held_by_two_relative_edges(g40):
    full = flatten(g40)
    p = 20
    fp = drop_edges(full, [p])
    assert p < fp.Pf and not np.any(np.asarray(fp.eP) == p) and fp.Pt == full.Pt
    rel = make_rel(fp, [(p - 1, p), (p, p + 1)], seed=12)
    h = solver(fp, RK_HUBER, rel)
    rp, ci = h.hsc_structure()
    assert set(ci[rp[p]:rp[p + 1]]) == {p, p + 1}
    for opts in ({}, {"reduced_solver": 1}, {"profile": 1}, {"spmv_upper": 1}):
        follows_dense(fp, RK_HUBER, rel, **opts)


def test_graph_whose_only_off_diagonal_blocks_are_relative_ones():
    """three free poses that share no landmark (all other poses fixed): no Schur product connects two free poses"""
    g = synth_ba(40, 600, 2400, seed=1, loop_closure=False)
    base = flatten(freed(g))
    have = covisible(base)
    rows = [0]
    for r in range(1, g.nposes):
        if all((min(int(a), r), max(int(a), r)) not in have for a in rows):
            rows.append(r)
    rows = rows[:3]
    assert len(rows) == 3 and base.Pf == base.Pt          # (all poses free: solver index = row)
    g.pose_fixed[:] = True
    g.pose_fixed[rows] = False
    fp = flatten(g)
    assert fp.Pf == 3 and not covisible(fp)
    plain = HipSolver(fp, RK_HUBER)
    assert len(block_set(plain)) == 3
    rel = make_rel(fp, [(0, 1), (2, 1), (0, 2)], seed=13)
    h = solver(fp, RK_HUBER, rel)
    assert block_set(h) == {(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)}
    for opts in ({}, {"reduced_solver": 1}):
        follows_dense(fp, RK_HUBER, rel, **opts)


# ---- loop closure --------------------------------------------------------------------------------------------------------------------
def test_loop_closure_on_an_open_trajectory():
    P = 120
    g = synth_ba(P, 1800, 7200, seed=6, loop_closure=False)          # (start = poses perturbed off the ground truth)
    fp = flatten(g)
    src = list(np.asarray(fp.pose_src))
    first, last = src.index(1), src.index(P - 1)          # (row 0 is the fixed pose: the closure ties the first free pose to the last)
    plain = solver(fp, RK_HUBER)
    assert (min(first, last), max(first, last)) not in block_set(plain)
    qt, tt = np.asarray(g.truth["q"])[fp.pose_src], np.asarray(g.truth["t"])[fp.pose_src]
    z = rr.measurement(qt, tt, first, last)
    rel = (np.array([first]), np.array([last]), z[0][None], z[1][None], np.array([np.diag([1e6] * 3 + [1e4] * 3)]))
    follows_dense(fp, RK_HUBER, rel)
    h = solver(fp, RK_HUBER, rel)
    assert np.array_equal(h.pcg_config()["pose_order"], plain.pcg_config()["pose_order"])
    h.optimize(10); plain.optimize(10)
    cov, cov0 = h.covariance(landmarks=False), plain.covariance(landmarks=False)
    assert not cov["not_positive_definite"] and not cov0["not_positive_definite"]
    assert np.trace(cov["pose"][last]) < np.trace(cov0["pose"][last])
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    H = rr.system(o, fp, None, rel, 0.0)[0]
    Hi = np.linalg.inv(H)
    n = 6 * fp.Pf
    S_model = H[:n, :n] - H[:n, n:] @ np.linalg.solve(H[n:, n:], H[n:, :n])
    S_own = _dense_from_upper(*h.hsc(), fp.Pf)
    Si_own, Si_model = np.linalg.inv(S_own), np.linalg.inv(S_model)

    def worst_pose(Si):
        return max(np.abs(cov["pose"][p] - Si[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() / np.abs(Si[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() for p in range(fp.Pf))
    print("reduced matrix: library vs model %.2e of its largest entry, condition number %.2e" % (np.abs(S_own - S_model).max() / np.abs(S_model).max(), np.linalg.cond(S_own)))
    print("pose covariances: against the dense inverse of the full model Hessian %.2e, of the model's reduced matrix %.2e, of the library's own reduced matrix %.2e"
          % (worst_pose(Hi), worst_pose(Si_model), worst_pose(Si_own)))
    # The algorithm is held to the issue's bar against the dense inverse of the very matrix it factorised (the library's reduced matrix at
    # lambda = 0, which the covariance call leaves in place; its assembly is checked block by block against the model below).  Against
    # the inverse of the model's independently rounded Hessian the blocks can only agree to what the conditioning of S makes of fp64
    # rounding in its entries: 1e-9 + 10 cond(S) eps (cond(S) = 3.1e7 on this open 120-pose chain held at one end: 6.9e-8).  Measured:
    # 6.8e-12 against the own matrix, 1.6e-8 against the model's (the two reduced matrices differ by 1.4e-11 of the largest entry).
    assert worst_pose(Si_own) <= 1e-9
    assert worst_pose(Hi) <= 1e-9 + 10 * np.linalg.cond(S_own) * np.finfo(np.float64).eps
    check_assembly(fp, rel)
    key = (min(first, last), max(first, last))
    blocks = h.covariance_blocks()
    blk = blocks[block_index(h)[key]]
    want = Si_own[6 * key[0]:6 * key[0] + 6, 6 * key[1]:6 * key[1] + 6]
    assert np.abs(blk - want).max() <= 1e-9 * np.abs(want).max()
    pairs, bad = h.covariance_pairs([("pose", key[0], "pose", key[1])])
    assert not bad
    assert np.abs(pairs[0] - blk).max() <= 1e-12 * np.abs(blk).max()
    ref = None
    for slack in (0, 2, 4, 8):
        c = solver(fp, RK_HUBER, rel, reduced_solver=1, direct_slack=slack).optimize(10)["chi2"]
        ref = c if ref is None else ref
        assert len(c) == len(ref) and relerr(c, ref).max() <= 1e-9


# ---- optimality ----------------------------------------------------------------------------------------------------------------------
def test_gradient_vanishes_at_non_zero_residuals():
    """tests/test_relative_pose_reference.py shows on the CPU that this bar is missed (1e-2 of the start) with Ad(M) = I in dr/dd_i"""
    fp, rel = gradient_graph()
    o = OracleSolver(fp, RK_NONE)
    g0 = np.linalg.norm(rr.gradient(o, fp, None, rel))
    h = solver(fp, RK_NONE, rel, pcg_tol=1e-12)
    h.optimize(40)
    o.set_state(*h.state())
    q, t, _ = h.state()
    assert rr.rel_chi2(rel, q, t, fp.Pf).sum() > 1e-3
    got = np.linalg.norm(rr.gradient(o, fp, None, rel)) / g0
    print("gradient after 40 iterations / start: %.3e" % got)
    assert got <= 1e-6


# ---- scale ---------------------------------------------------------------------------------------------------------------------------
def internal_position(h, Pf):
    """internal index of every free pose (caller's numbering) from pcg_config()["pose_order"]"""
    order = np.asarray(h.pcg_config()["pose_order"])
    pos = np.empty(Pf, dtype=np.int64)
    pos[order] = np.arange(Pf)
    return pos


# odometry on every consecutive pair + long-range closures that no landmark supports, random partners at the pose of the widest row.  Ten
# of them bring that row beyond the fixed width of 60 at the "big" shape (56 entries before) but not at KITTI-07's (46): a third case with
# twenty closures exercises the overflow entries there.
@pytest.mark.parametrize("name,nclosures,overflow", [("kitti07", 10, False), ("big", 10, True), ("kitti07", 20, True)])
def test_pcg_and_exact_solver_agree_at_scale(name, nclosures, overflow):
    g = synth_named("kitti07") if name == "kitti07" else synth_ba(1700, 12000, 60000, seed=3)
    fp = flatten(g)
    src = np.asarray(fp.pose_src)
    row_to_solver = np.empty(len(src), dtype=np.int64)
    row_to_solver[src] = np.arange(len(src))
    rng = np.random.default_rng(14)
    pairs = [(int(row_to_solver[r]), int(row_to_solver[r + 1])) for r in range(g.nposes - 1)]          # odometry
    have = covisible(fp)
    width = np.bincount(np.array([p for pair in have for p in pair]), minlength=fp.Pf)
    hub = int(np.argmax(width))
    far_off = max(24, fp.Pf // 8)
    closures = []
    while len(closures) < nclosures:
        b = int(rng.integers(0, fp.Pf))
        key = (min(hub, b), max(hub, b))
        if abs(hub - b) > far_off and key not in have and key not in closures:
            closures.append(key)
    rel = make_rel(fp, pairs + closures, seed=14, rot=0.002, trans=0.02)
    plain = HipSolver(fp, RK_HUBER)
    a = solver(fp, RK_HUBER, rel, pcg_tol=1e-10)
    ca = a.optimize(10)["chi2"]
    cb = solver(fp, RK_HUBER, rel, reduced_solver=1).optimize(10)["chi2"]
    print("%s: chi2 per iteration PCG vs exact: max rel %.2e" % (name, relerr(ca[:len(cb)], cb[:len(ca)]).max()))
    assert len(ca) == len(cb) and relerr(ca, cb).max() <= CHI2_TOL
    hist, unconverged = a.pcg_history()
    assert unconverged == 0 and np.all(hist >= 0)
    assert set(closures) <= block_set(a)
    assert a.counters()["hsc_blocks"] == len(have) + fp.Pf + nclosures
    # a handful of closures leaves the order of a trajectory-ordered graph alone, so every closure is a far block
    cfg = a.pcg_config()
    assert np.array_equal(cfg["pose_order"], plain.pcg_config()["pose_order"])
    pos = internal_position(a, fp.Pf)
    assert all(abs(pos[x] - pos[y]) > far_off for x, y in closures)
    print("%s: ell_m %d ell_over %d, widest row before %d" % (name, cfg["ell_m"], cfg["ell_over"], width[hub] + 1))
    assert cfg["ell_over"] == (1 if overflow else 0)


def test_pose_order_places_a_pose_with_relative_edges_only_next_to_a_neighbour():
    """shuffled pose ids make the library renumber the poses (strongest-neighbour walk over the block pattern): a pose without any
    reprojection edge is placed through its relative-pose blocks"""
    g = shuffled_pose_ids(synth_ba(200, 3000, 12000, seed=2), seed=1)
    full = flatten(g)
    src = list(np.asarray(full.pose_src))                             # (the graph's rows are in trajectory order)
    p, before, after = src.index(100), src.index(99), src.index(101)
    fp = drop_edges(full, [p])
    rel = make_rel(fp, [(before, p), (p, after)], seed=25)
    h = solver(fp, RK_HUBER, rel)
    h.build_structure()
    pos = internal_position(h, fp.Pf)
    assert not np.array_equal(pos, np.arange(fp.Pf))                  # (the renumbering took place)
    assert min(abs(pos[p] - pos[before]), abs(pos[p] - pos[after])) == 1
    ca = h.optimize(10)["chi2"]
    cb = solver(fp, RK_HUBER, rel, reduced_solver=1).optimize(10)["chi2"]
    assert len(ca) == len(cb) and relerr(ca, cb).max() <= CHI2_TOL


# ---- rebuild rule --------------------------------------------------------------------------------------------------------------------
def test_structure_is_rebuilt_exactly_when_the_pair_set_changes(g40):
    fp = flatten(g40)
    near, far = split_pairs(fp, 3, 1)
    h = solver(fp, RK_HUBER, make_rel(fp, [far[0], near[0], far[1]], seed=15))
    h.optimize(2)
    n0 = h.counter("structure_builds")
    h.set_relative_pose_edges(*make_rel(fp, [far[1], (far[0][1], far[0][0]), far[0], near[0]], seed=16))       # same pairs, new values and order
    h.optimize(2)
    assert h.counter("structure_builds") == n0
    h.set_relative_pose_edges(*make_rel(fp, [far[0], near[0], far[1], far[2]], seed=17))                        # a new pair
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 1
    h.set_graph(fp)                                                                                           # unchanged topology
    h.set_relative_pose_edges(*make_rel(fp, [far[0], near[0], far[1], far[2]], seed=18))
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 1
    h.set_graph(fp)                                                                                           # ... and no edges after it
    h.optimize(2)
    assert h.counter("structure_builds") == n0 + 2
    assert block_set(h) == block_set(HipSolver(fp, RK_HUBER))


# ---- batch ---------------------------------------------------------------------------------------------------------------------------
def test_batch_with_relative_edges_is_the_solo_runs():
    fps = [flatten(synth_ba(40, 600, 2400, seed=s)) for s in (1, 2, 3)]
    rels = [make_rel(fps[0], mixed_pairs(fps[0], 19), seed=19), None, make_rel(fps[2], mixed_pairs(fps[2], 20), seed=20)]
    solo = [solver(f, RK_HUBER, r).optimize(8)["chi2"] for f, r in zip(fps, rels)]
    hs = [solver(f, RK_HUBER, r) for f, r in zip(fps, rels)]
    chi, _ = optimize_batch(hs, 8)
    for k in range(3):
        assert np.array_equal(np.asarray(chi[k])[:len(solo[k])], solo[k])


def test_plain_batch_still_batches():
    fps = [flatten(synth_ba(40, 600, 2400, seed=s)) for s in (1, 2)]
    hs = [solver(f, RK_HUBER) for f in fps]
    _, batched = optimize_batch(hs, 5)
    assert batched > 0


# ---- life cycle and refusals ---------------------------------------------------------------------------------------------------------
def test_set_graph_clears_the_edges(g40):
    fp = flatten(g40)
    _, far = split_pairs(fp, 1, 1)
    h = solver(fp, RK_HUBER, make_rel(fp, [far[0], (1, 2)], seed=21))
    h.set_graph(fp)
    assert len(h.relative_pose_chi_squares()) == 0
    assert np.array_equal(h.optimize(5)["chi2"], solver(fp, RK_HUBER).optimize(5)["chi2"])


def test_refusals_leave_a_usable_handle(g40):
    fp = flatten(g40)
    good = make_rel(fp, [(1, 2), (3, 30)], seed=22)
    h = solver(fp, RK_HUBER, good)
    before = h.relative_pose_chi_squares()
    same = (np.array([1, 4]), np.array([2, 4]), good[2], good[3], good[4])
    out_of_range = (np.array([1, fp.Pt]), good[1], good[2], good[3], good[4])
    negative = (good[0], np.array([-1, 2]), good[2], good[3], good[4])
    for bad in (same, out_of_range, negative):
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_relative_pose_edges(*bad)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_partition(0, fp.Lt // 2)
    assert np.array_equal(h.relative_pose_chi_squares(), before)
    p = solver(fp, RK_HUBER)
    p.set_partition(0, fp.Lt // 2)
    with pytest.raises(CubaHipError, match="status 3"):
        p.set_relative_pose_edges(*good)
    assert len(p.optimize(3)["chi2"]) > 0
    assert len(h.optimize(5)["chi2"]) > 0
    # covariance blocks describe the edge set they were computed on: a new set invalidates them
    h.covariance(landmarks=False)
    assert len(h.covariance_blocks()) == h.counters()["hsc_blocks"]
    h.set_relative_pose_edges(*make_rel(fp, [(1, 2), (3, 30), (4, 35)], seed=26))
    with pytest.raises(CubaHipError, match="status 3"):
        h.covariance_blocks()


def test_graph_without_reprojection_edges_refuses(g40):
    full = flatten(g40)
    none = np.zeros(0, dtype=np.int32)
    fp = dataclasses.replace(full, eP=none, eL=none, eDim=np.zeros(0, np.uint8), meas=np.zeros((0, 3)), omega=np.zeros(0), edge_src=np.zeros(0, np.int64))
    h = HipSolver(fp, RK_HUBER)
    with pytest.raises(CubaHipError, match="status 3"):
        h.set_relative_pose_edges([0], [1], np.array([[0, 0, 0, 1.0]]), np.zeros((1, 3)), np.eye(6)[None])
    h.set_graph(full)
    assert len(h.optimize(3)["chi2"]) > 0


# ---- other builds, reproducibility ---------------------------------------------------------------------------------------------------
def test_fp32_library_and_mixed_precision(g40):
    fp = flatten(g40)
    rel = make_rel(fp, mixed_pairs(fp, 23), seed=23)
    ref = solver(fp, RK_HUBER, rel).optimize(10)["chi2"]
    f32 = solver(fp, RK_HUBER, rel, precision="f32").optimize(10)["chi2"]
    n = min(len(f32), len(ref))
    assert n >= 8 and relerr(f32[:n], ref[:n]).max() <= 1e-5
    mixed = solver(fp, RK_HUBER, rel, mixed_precision=1).optimize(10)["chi2"]
    assert len(mixed) == len(ref) and relerr(mixed, ref).max() <= CHI2_TOL


def test_repeat_runs_are_bit_identical(g40):
    fp = flatten(g40)
    rel = make_rel(fp, mixed_pairs(fp, 24), seed=24)
    runs = []
    for _ in range(2):
        h = solver(fp, RK_HUBER, rel)
        runs.append((h.optimize(10)["chi2"], h.state(), h.relative_pose_chi_squares()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][2], runs[1][2])
    for x, y in zip(runs[0][1], runs[1][1]):
        assert np.array_equal(x, y)

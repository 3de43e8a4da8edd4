"""Robust kernels on the pose factors (cuba_hip_set_pose_factor_robust_kernels / HipSolver.set_pose_factor_robust_kernels) on the GPU
against the numpy model of tests/robust_pose_factor_reference.py: the assembled system, the objective, more than one workgroup, LM
trajectories against a dense fp64 LM on every solve path, the parent path for kinds all 0, the kernels' lifetime, the refusals, an edge to a
fixed pose against the corresponding prior, the other builds, batches and the covariances.

Bars: those of the existing pose-factor tests (tests/test_gpu_pose_priors.py, tests/test_gpu_relative_pose.py) for the same quantities:
assembly 1e-12 of the block's / vector's largest entry, chi2 per iteration 1e-6 against the dense LM, host loop against device-decision
loop 1e-9, covariance against the dense inverse 1e-9.

Tukey's weight cancels near e = delta^2 and Huber's branch flips there, so every assembly case asserts IN THE MODEL that no factor has
e / delta^2 in [0.9, 1.1] and that factors lie on both sides (clear_of_threshold); the seeds below were chosen on the CPU so that it holds."""
import numpy as np
import pytest

import prior_reference as pr
import relative_pose_reference as rr
import robust_pose_factor_reference as rb
from conftest import RK_HUBER, with_fixed
from test_gpu_configs import shuffled_pose_ids
from test_gpu_covariance import _dense_from_upper
from test_gpu_pose_priors import freed, make_priors
from test_gpu_relative_pose import block_index, drop_edges, make_rel, mixed_pairs, relerr, split_pairs

from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle.oracle import OracleSolver

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
PRIORS, EDGES = 0, 1
D95 = float(np.sqrt(rb.CHI2_6DOF_95))


def solver(fp, rk=RK_HUBER, rel=None, priors=None, kr=None, kp=None, precision="f64", **opts):
    h = HipSolver(fp, rk, precision=precision, **opts)
    if priors is not None:
        h.set_pose_priors(*priors)
    if rel is not None:
        h.set_relative_pose_edges(*rel)
    if kp is not None:
        h.set_pose_factor_robust_kernels(PRIORS, *kp)
    if kr is not None:
        h.set_pose_factor_robust_kernels(EDGES, *kr)
    return h


def kernels(kinds, delta2):
    return np.asarray(kinds, dtype=np.int32), np.sqrt(np.asarray(delta2, dtype=np.float64))


def clear_of_threshold(kern, e, active):
    """the model's e / delta^2 of the factors with a kernel: none in [0.9, 1.1], some on either side"""
    kind, delta = kern
    sel = (kind != rb.NONE) & active
    x = e[sel] / delta[sel] ** 2
    print("e / delta^2 of the %d factors with a kernel: %s" % (sel.sum(), np.array2string(np.sort(x), precision=3) if sel.sum() <= 16 else
          "%d below 0.9 (max %.3g), %d above 1.1 (min %.3g)" % ((x < 0.9).sum(), x[x < 0.9].max(), (x > 1.1).sum(), x[x > 1.1].min())))
    assert not np.any((x >= 0.9) & (x <= 1.1))
    assert np.any(x < 0.9) and np.any(x > 1.1)
    for k in (rb.HUBER, rb.TUKEY):
        xk = e[sel & (kind == k)] / delta[sel & (kind == k)] ** 2
        assert np.any(xk < 0.9) and np.any(xk > 1.1), "kind %d needs factors on both sides" % k


@pytest.fixture(scope="module")
def g40():
    return synth_ba(40, 600, 2400, seed=1)


# ---- assembly ------------------------------------------------------------------------------------------------------------------------
def check_assembly(fp, rel, kr, priors=None, kp=None):
    plain, h = solver(fp), solver(fp, RK_HUBER, rel, priors, kr, kp)
    for s in (plain, h):
        s.set_lambda(0.0)
        s.schur()
    _, _, v0 = plain.hsc()
    _, _, v1 = h.hsc()
    i0, i1 = block_index(plain), block_index(h)
    q, t, _ = h.state()
    clear_of_threshold(kr, rr.rel_chi2(rel, q, t, fp.Pf), (rel[0] < fp.Pf) | (rel[1] < fp.Pf))
    Hm, bm = rb.rel_system(rel, kr, q, t, fp.Pf)
    touched = set()
    for i, j in zip(rel[0], rel[1]):
        i, j = int(i), int(j)
        touched |= {(p, p) for p in (i, j) if p < fp.Pf}
        if i < fp.Pf and j < fp.Pf:
            touched.add((min(i, j), max(i, j)))
    if priors is not None:
        clear_of_threshold(kp, pr.prior_chi2(priors, q, t, fp.Pf), priors[0] < fp.Pf)
        Hp, bp = rb.prior_system(priors, kp, q, t, fp.Pf)
        Hm, bm = Hm + Hp, bm + bp
        touched |= {(int(p), int(p)) for p in priors[0] if p < fp.Pf}
    worst = 0.0
    for key, k1 in i1.items():
        base = v0[i0[key]] if key in i0 else np.zeros((6, 6))
        if key not in touched:
            assert np.array_equal(v1[k1], base), key
            continue
        want = base + Hm[6 * key[0]:6 * key[0] + 6, 6 * key[1]:6 * key[1] + 6]
        sel = np.triu_indices(6) if key[0] == key[1] else (slice(None), slice(None))
        worst = max(worst, np.abs(v1[k1][sel] - want[sel]).max() / np.abs(want[sel]).max())
    for name in ("bp", "bsc"):
        a0, a1 = plain.array(name), h.array(name)
        want = a0 + bm
        worst = max(worst, np.abs(a1 - want).max() / np.abs(want).max())
        rows = np.array([6 * p + c for p in range(fp.Pf) if (p, p) not in touched for c in range(6)], dtype=np.int64)
        assert np.array_equal(a1[rows], a0[rows])
    print("assembled hsc / bp / bsc against plain + model's weighted terms: max rel %.2e" % worst)
    assert worst <= 1e-12


# kinds and delta^2 per factor (distinct): make_rel / make_priors give e of the order of 1e2
EDGE_KINDS = [rb.HUBER, rb.TUKEY, rb.CAUCHY, rb.NONE, rb.TUKEY, rb.CAUCHY, rb.HUBER, rb.HUBER, rb.TUKEY]
EDGE_DELTA2 = [40.0, 900.0, 60.0, 1.0, 50.0, 300.0, 800.0, 30.0, 700.0]
PRIOR_KINDS = [rb.HUBER, rb.TUKEY, rb.CAUCHY, rb.NONE, rb.CAUCHY, rb.HUBER, rb.TUKEY, rb.HUBER]
PRIOR_DELTA2 = [120.0, 2500.0, 200.0, 1.0, 90.0, 70.0, 150.0, 3000.0]


def assembly_factors(fp, seed):
    """one set mixing the four kinds with a delta of its own per factor: a co-visible pair, a pair without landmarks with two edges under
    different kernels, reversed edges, edges to the fixed pose (either end); priors with kernels: two on one pose, one on the fixed pose"""
    near, far = split_pairs(fp, 2, 2)
    fixed = fp.Pt - 1
    assert fixed >= fp.Pf
    pairs = [near[0], far[0], far[0], (far[1][1], far[1][0]), (near[1][1], near[1][0]), (5, fixed), (fixed, 9), near[0], (far[1][0], far[1][1])]
    rel = make_rel(fp, pairs, seed=seed)
    pri = make_priors(fp, [1, 5, 5, 17, fp.Pf - 1, fixed, 9, 22], seed=seed + 1)
    return rel, kernels(EDGE_KINDS, EDGE_DELTA2), pri, kernels(PRIOR_KINDS, PRIOR_DELTA2)


def scrambled(factors, kern, seed):
    """the same set (and its kernels) in another order"""
    perm = np.random.default_rng(seed).permutation(len(factors[0]))
    return tuple(np.asarray(a)[perm] for a in factors), tuple(np.asarray(a)[perm] for a in kern)


ASSEMBLY_SEED, ASSEMBLY_SEED_SHUFFLED = 3, 8


def test_assembled_system_is_the_plain_one_plus_the_weighted_terms(g40):
    fp = flatten(g40)
    rel, kr, pri, kp = assembly_factors(fp, ASSEMBLY_SEED)
    check_assembly(fp, rel, kr, pri, kp)


def test_assembled_system_with_shuffled_pose_ids_and_scrambled_factors():
    """a kernel that follows the wrong factor through the sort of the upload fails here: every factor has a kernel of its own"""
    fp = flatten(shuffled_pose_ids(synth_ba(60, 900, 3600, seed=2), seed=1))
    rel, kr, pri, kp = assembly_factors(fp, ASSEMBLY_SEED_SHUFFLED)
    rel, kr = scrambled(rel, kr, 5)
    pri, kp = scrambled(pri, kp, 6)
    check_assembly(fp, rel, kr, pri, kp)


# ---- objective -----------------------------------------------------------------------------------------------------------------------
def check_objective(fp, rel, kr, pri, kp):
    plain, h = solver(fp), solver(fp, RK_HUBER, rel, pri, kr, kp)
    q, t, _ = h.state()
    er, ep = rr.rel_chi2(rel, q, t, fp.Pf), pr.prior_chi2(pri, q, t, fp.Pf)
    # the chi-squares calls keep returning the plain r^T Omega r
    assert np.abs(h.relative_pose_chi_squares() - er).max() <= 1e-10 * er.max()
    assert np.abs(h.prior_chi_squares() - ep).max() <= 1e-10 * ep.max()
    want = plain.compute_errors() + rb.rhos(kr, er).sum() + rb.rhos(kp, ep).sum()
    got = h.compute_errors()
    print("objective %.12g, model %.12g; without kernels %.12g" % (got, want, plain.compute_errors() + er.sum() + ep.sum()))
    assert abs(got - want) <= 1e-12 * want
    assert abs(got - (plain.compute_errors() + er.sum() + ep.sum())) > 1e-3 * want          # (the kernels matter here)


def test_objective_and_chi_squares(g40):
    fp = flatten(g40)
    check_objective(fp, *assembly_factors(fp, ASSEMBLY_SEED))


# ---- more than one workgroup ---------------------------------------------------------------------------------------------------------
def many_factors(fp):
    """7 edges on each of the 38 consecutive free pairs (266: five workgroups of the linearisation, two of the chi2 kernel) and 7 priors on
    each of the 39 free poses (273); kinds in turn, delta^2 far below (4) or far above (4000) the factors' e of the order of 1e2"""
    pairs = [(p, p + 1) if k % 2 == 0 else (p + 1, p) for k in range(7) for p in range(fp.Pf - 1)]
    rel = make_rel(fp, pairs, seed=40)
    pri = make_priors(fp, [p for k in range(7) for p in range(fp.Pf)], seed=41)
    n, m = len(pairs), len(pri[0])
    kr = kernels(np.arange(n) % 4, np.where((np.arange(n) // 4) % 2 == 0, 4.0, 4000.0))
    kp = kernels((np.arange(m) + 1) % 4, np.where((np.arange(m) // 4) % 2 == 0, 4000.0, 4.0))
    return rel, kr, pri, kp


def test_more_than_one_workgroup(g40):
    fp = flatten(g40)
    rel, kr, pri, kp = many_factors(fp)
    assert len(rel[0]) >= 257 and len(pri[0]) >= 257
    check_objective(fp, rel, kr, pri, kp)
    check_assembly(fp, rel, kr, pri, kp)


# ---- LM against the dense model --------------------------------------------------------------------------------------------------------
_dense = {}


def scenario(fp):
    odo, bad = rb.false_closure_scenario(fp)
    return odo, rb.join(odo, bad), len(odo[0])


CLOSURE_KERNELS = {"huber": (rb.HUBER, D95), "cauchy": (rb.CAUCHY, D95), "tukey": (rb.TUKEY, 3 * D95)}


def dense_scenario(fp, name):
    """the dense LM of the false-closure scenario, computed once per kernel"""
    if name not in _dense:
        odo, both, n = scenario(fp)
        rel, kr = (odo, None) if name == "clean" else (both, rb.closure_kernels(n, *CLOSURE_KERNELS[name]))
        _dense[name] = rb.dense_lm(OracleSolver(fp, RK_HUBER), fp, None, rel, 10, kr=kr)["chi2"]
    return _dense[name]


def follows(got, ref):
    print("chi2 per iteration vs dense LM: %d / %d iterations, max rel %.2e" % (len(got), len(ref), relerr(got[:len(ref)], ref[:len(got)]).max()))
    assert len(got) == len(ref)
    assert relerr(got, ref).max() <= CHI2_TOL


LM_CASES = [("huber", {}), ("tukey", {}), ("cauchy", {}), ("cauchy", {"profile": 1}), ("huber", {"reduced_solver": 1}), ("cauchy", {"spmv_upper": 1})]


@pytest.mark.parametrize("name,opts", LM_CASES, ids=["%s%s" % (n, "".join("-" + k for k in o)) for n, o in LM_CASES])
def test_lm_follows_the_dense_model_on_the_false_closures(g40, name, opts):
    fp = flatten(g40)
    _, both, n = scenario(fp)
    h = solver(fp, RK_HUBER, both, kr=rb.closure_kernels(n, *CLOSURE_KERNELS[name]), **opts)
    follows(h.optimize(10)["chi2"], dense_scenario(fp, name))


def test_tukey_switches_the_false_closures_off(g40):
    """F of every iteration is that of the run without the two closures plus 2 delta^2 / 3: in the model (1e-6, the bar against a dense LM)
    and against the library's own clean run (1e-9)"""
    fp = flatten(g40)
    odo, both, n = scenario(fp)
    const = 2 * (3 * D95) ** 2 / 3
    clean = solver(fp, RK_HUBER, odo, pcg_tol=1e-11).optimize(10)["chi2"]
    h = solver(fp, RK_HUBER, both, kr=rb.closure_kernels(n, rb.TUKEY, 3 * D95), pcg_tol=1e-11)
    got = h.optimize(10)["chi2"]
    follows(got, dense_scenario(fp, "clean") + const)
    print("Tukey run vs clean run + 2 delta^2 / 3: max rel %.2e" % relerr(got, clean + const).max())
    assert len(got) == len(clean) and relerr(got, clean + const).max() <= 1e-9
    assert np.array_equal(h.relative_pose_chi_squares()[-2:] > (3 * D95) ** 2, [True, True])


def test_cauchy_keeps_the_trajectory_of_the_clean_run(g40):
    fp = flatten(g40)
    odo, both, n = scenario(fp)
    ends = []
    for rel, kr in ((odo, None), (both, None), (both, rb.closure_kernels(n, rb.CAUCHY, D95))):
        h = solver(fp, RK_HUBER, rel, kr=kr)
        h.optimize(10)
        ends.append(h.state()[1])
    off_none, off_cauchy = np.abs(ends[1] - ends[0]).max(), np.abs(ends[2] - ends[0]).max()
    print("max |t - t_clean|: no kernel %.4g, Cauchy %.4g" % (off_none, off_cauchy))
    assert off_cauchy < 0.1 * off_none


def mixed_kernels(n, seed, lo=30.0, hi=600.0):
    rng = np.random.default_rng(seed)
    return kernels(rng.integers(0, 4, size=n), rng.uniform(lo, hi, size=n))


def test_kernels_on_priors_without_a_fixed_pose(g40):
    fp = flatten(freed(g40))
    assert fp.Pf == fp.Pt
    pri = make_priors(fp, [0, 13, 13, 25], seed=10)          # (the gauge is held by the priors: Cauchy on pose 0 never lets go)
    kp = kernels([rb.CAUCHY, rb.HUBER, rb.TUKEY, rb.NONE], [100.0, 60.0, 2000.0, 1.0])
    rel = make_rel(fp, mixed_pairs(fp, 10), seed=10)
    kr = mixed_kernels(len(rel[0]), 11)
    ref = rb.dense_lm(OracleSolver(fp, RK_HUBER), fp, pri, rel, 10, kp=kp, kr=kr)["chi2"]
    follows(solver(fp, RK_HUBER, rel, pri, kr, kp).optimize(10)["chi2"], ref)


def test_motion_only_follows_the_dense_model(g40):
    fp = flatten(with_fixed(g40, fixed_lm_rows=range(g40.nlandmarks)))
    assert fp.Lf == 0
    rel = make_rel(fp, mixed_pairs(flatten(g40), 9), seed=9)
    kr = mixed_kernels(len(rel[0]), 12)
    pri = make_priors(fp, [4, 4, 30], seed=13)
    kp = kernels([rb.TUKEY, rb.CAUCHY, rb.HUBER], [3000.0, 80.0, 50.0])
    ref = rb.dense_lm(OracleSolver(fp, RK_HUBER), fp, pri, rel, 10, kp=kp, kr=kr)["chi2"]
    follows(solver(fp, RK_HUBER, rel, pri, kr, kp).optimize(10)["chi2"], ref)


def test_host_loop_is_the_device_decision_loop(g40):
    fp = flatten(g40)
    _, both, n = scenario(fp)
    kr = (np.concatenate([np.full(n, rb.HUBER), [rb.CAUCHY, rb.CAUCHY]]).astype(np.int32), np.full(n + 2, D95))
    a, b = solver(fp, RK_HUBER, both, kr=kr, pcg_tol=1e-11), solver(fp, RK_HUBER, both, kr=kr, pcg_tol=1e-11, profile=1)
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    assert len(ca) == len(cb) and relerr(ca, cb).max() <= 1e-9
    assert a.counters()["lm_trials"] == b.counters()["lm_trials"]


# ---- kinds all 0, lifetime, refusals -------------------------------------------------------------------------------------------------
def record(h, niter=8):
    h.set_lambda(0.0)
    h.schur()
    system = (h.hsc()[2], h.array("bp"), h.array("bsc"))
    res = h.optimize(niter)
    return dict(system=system, chi2=res["chi2"], state=h.state(), counters=h.counters(), pcg=h.pcg_history()[0], builds=h.counter("structure_builds"),
                chi=(h.relative_pose_chi_squares(), h.prior_chi_squares()))


def assert_same_run(a, b):
    for x, y in zip(a["system"] + a["state"] + a["chi"], b["system"] + b["state"] + b["chi"]):
        assert np.array_equal(x, y)
    assert np.array_equal(a["chi2"], b["chi2"]) and np.array_equal(a["pcg"], b["pcg"])
    assert a["counters"] == b["counters"] and a["builds"] == b["builds"]


def test_kinds_all_zero_is_the_parent_path(g40):
    fp = flatten(g40)
    rel, _, pri, _ = assembly_factors(fp, ASSEMBLY_SEED)
    never = solver(fp, RK_HUBER, rel, pri)
    zeros = solver(fp, RK_HUBER, rel, pri, kr=(0, 0.0), kp=(np.zeros(len(pri[0]), np.int32), np.full(len(pri[0]), 3.0)))
    cleared = solver(fp, RK_HUBER, rel, pri, kr=(rb.CAUCHY, 2.0), kp=(rb.TUKEY, 5.0))
    for t in (PRIORS, EDGES):
        cleared.set_pose_factor_robust_kernels(t, [], [])
    ref = record(never)
    assert ref["builds"] == 1
    assert_same_run(record(zeros), ref)
    assert_same_run(record(cleared), ref)


def test_kernels_leave_the_structure_and_go_with_their_set(g40):
    fp = flatten(g40)
    rel, kr, pri, kp = assembly_factors(fp, ASSEMBLY_SEED)
    plain = record(solver(fp, RK_HUBER, rel, pri))
    robust = record(solver(fp, RK_HUBER, rel, pri, kr, kp))
    assert not np.array_equal(plain["chi2"], robust["chi2"])
    # setting kernels on a handle that has run: no structure build, and the run is that of a handle that had them from the start
    h = solver(fp, RK_HUBER, rel, pri)
    h.build_structure()
    n0 = h.counter("structure_builds")
    h.set_pose_factor_robust_kernels(EDGES, *kr)
    h.set_pose_factor_robust_kernels(PRIORS, *kp)
    late = record(h)
    assert late["builds"] == n0 == 1
    assert_same_run(late, robust)
    # replacing a set drops its kernels
    h = solver(fp, RK_HUBER, rel, pri, kr, kp)
    h.set_relative_pose_edges(*rel)
    h.set_pose_priors(*pri)
    assert_same_run(record(h), plain)
    # ... one set only: the other keeps its kernels
    h = solver(fp, RK_HUBER, rel, pri, kr, kp)
    h.set_pose_priors(*pri)
    assert_same_run(record(h), record(solver(fp, RK_HUBER, rel, pri, kr, None)))
    # set_graph drops them with the sets
    h = solver(fp, RK_HUBER, rel, pri, kr, kp)
    h.set_graph(fp)
    with pytest.raises(CubaHipError, match="status 1"):
        h.set_pose_factor_robust_kernels(EDGES, *kr)          # (no edges now: the count differs)
    h.set_pose_priors(*pri)
    h.set_relative_pose_edges(*rel)
    again = record(h)
    assert np.array_equal(again["chi2"], plain["chi2"])
    for x, y in zip(again["system"] + again["state"], plain["system"] + plain["state"]):
        assert np.array_equal(x, y)


def test_covariance_blocks_are_invalidated_by_new_kernels(g40):
    fp = flatten(g40)
    rel, kr, _, _ = assembly_factors(fp, ASSEMBLY_SEED)
    h = solver(fp, RK_HUBER, rel)
    h.covariance(landmarks=False)
    assert len(h.covariance_blocks()) == h.counters()["hsc_blocks"]
    h.set_pose_factor_robust_kernels(EDGES, *kr)
    with pytest.raises(CubaHipError, match="status 3"):
        h.covariance_blocks()


def test_refusals_leave_an_unchanged_handle(g40):
    fp = flatten(g40)
    rel, kr, pri, kp = assembly_factors(fp, ASSEMBLY_SEED)
    h, twin = solver(fp, RK_HUBER, rel, pri, kr, kp), solver(fp, RK_HUBER, rel, pri, kr, kp)
    before = h.compute_errors()
    n = len(rel[0])
    kind, delta = kr

    def changed(k, v, arr):
        out = np.array(arr, copy=True)
        out[k] = v
        return out

    bad = [
        (EDGES, kind[:-1], delta[:-1]),                         # wrong n
        (EDGES, np.append(kind, 1), np.append(delta, 2.0)),
        (PRIORS, kind, delta),                                  # (the edges' count on the priors)
        (EDGES, changed(2, 4, kind), delta),                    # bad kinds
        (EDGES, changed(2, -1, kind), delta),
        (EDGES, kind, changed(0, 0.0, delta)),                  # delta <= 0 on a kind != 0
        (EDGES, kind, changed(1, -3.0, delta)),
        (EDGES, kind, changed(4, np.nan, delta)),               # non-finite, on a factor with a kernel and on one without
        (EDGES, kind, changed(3, np.nan, delta)),
        (EDGES, kind, changed(3, np.inf, delta)),
        (2, kind, delta),                                       # bad factor types
        (-1, kind, delta),
    ]
    assert kind[0] != rb.NONE and kind[1] != rb.NONE and kind[4] != rb.NONE and kind[3] == rb.NONE and len(kp[0]) != n
    for args in bad:
        with pytest.raises(CubaHipError, match="status 1"):
            h.set_pose_factor_robust_kernels(*args)
        assert h.compute_errors() == before
    # (a delta <= 0 on a factor without a kernel is no error)
    h.set_pose_factor_robust_kernels(EDGES, kind, changed(3, -1.0, delta))
    assert h.compute_errors() == before
    assert_same_run(record(h), record(twin))


# ---- one end fixed -------------------------------------------------------------------------------------------------------------------
def test_one_end_fixed_is_the_corresponding_prior_with_the_same_kernel(g40):
    fp = flatten(g40)
    fixed = fp.Pt - 1
    rel = make_rel(fp, [(fixed, 3), (fixed, 11), (fixed, 11), (fixed, 20), (fixed, 25)], seed=5)
    kern = kernels([rb.HUBER, rb.TUKEY, rb.HUBER, rb.TUKEY, rb.CAUCHY], [40.0, 900.0, 400.0, 10.0, 100.0])
    q, t, _ = HipSolver(fp, RK_HUBER).state()
    qb, tb = [], []
    for k in range(5):
        b = rr.pose_mul((rel[2][k], rel[3][k]), (rr.unit(q[fixed]), t[fixed]))
        qb.append(b[0]); tb.append(b[1])
    pri = (rel[1], np.array(qb), np.array(tb), rel[4])
    a, b = solver(fp, RK_HUBER, rel, kr=kern), solver(fp, RK_HUBER, None, pri, kp=kern)
    e = b.prior_chi_squares()
    clear_of_threshold(kern, pr.prior_chi2(pri, q, t, fp.Pf), np.ones(5, bool))
    assert np.abs(a.relative_pose_chi_squares() - e).max() <= 1e-12 * e.max()
    assert abs(a.compute_errors() - b.compute_errors()) <= 1e-12 * b.compute_errors()
    for s in (a, b):
        s.set_lambda(0.0)
        s.schur()
    va, vb = a.hsc()[2], b.hsc()[2]
    assert np.abs(va - vb).max() <= 1e-12 * np.abs(vb).max()
    for name in ("bp", "bsc"):
        assert np.abs(a.array(name) - b.array(name)).max() <= 1e-12 * np.abs(b.array(name)).max()
    ca, cb = a.optimize(10)["chi2"], b.optimize(10)["chi2"]
    assert len(ca) == len(cb) and relerr(ca, cb).max() <= 1e-9


# ---- other builds, batches, reproducibility ------------------------------------------------------------------------------------------
def mixed_case(fp, seed):
    rel = make_rel(fp, mixed_pairs(fp, seed), seed=seed)
    pri = make_priors(fp, [2, 2, 19], seed=seed + 1)
    return rel, mixed_kernels(len(rel[0]), seed + 2), pri, kernels([rb.CAUCHY, rb.TUKEY, rb.HUBER], [90.0, 2500.0, 60.0])


def test_fp32_library_and_mixed_precision(g40):
    fp = flatten(g40)
    rel, kr, pri, kp = mixed_case(fp, 23)
    ref = solver(fp, RK_HUBER, rel, pri, kr, kp).optimize(10)["chi2"]
    f32 = solver(fp, RK_HUBER, rel, pri, kr, kp, precision="f32").optimize(10)["chi2"]
    n = min(len(f32), len(ref))
    print("fp32 library vs fp64: %d / %d iterations, max rel %.2e" % (len(f32), len(ref), relerr(f32[:n], ref[:n]).max()))
    assert n >= 8 and relerr(f32[:n], ref[:n]).max() <= 1e-5
    mixed = solver(fp, RK_HUBER, rel, pri, kr, kp, mixed_precision=1).optimize(10)["chi2"]
    assert len(mixed) == len(ref) and relerr(mixed, ref).max() <= CHI2_TOL
    plain = solver(fp, RK_HUBER, rel, pri).optimize(10)["chi2"]
    assert relerr(plain[:1], ref[:1]).max() > 1e-3          # (the kernels matter in this case)


def test_batch_is_the_solo_runs_and_repeat_runs_are_bit_identical():
    fps = [flatten(synth_ba(40, 600, 2400, seed=s)) for s in (1, 2)]
    cases = [mixed_case(fps[0], 19), mixed_case(fps[1], 21)]
    solo = []
    for _ in range(2):
        runs = []
        for f, c in zip(fps, cases):
            h = solver(f, RK_HUBER, c[0], c[2], c[1], c[3])
            runs.append((h.optimize(8)["chi2"], h.state(), h.relative_pose_chi_squares(), h.prior_chi_squares()))
        solo.append(runs)
    for a, b in zip(*solo):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        for x, y in zip(a[1], b[1]):
            assert np.array_equal(x, y)
    hs = [solver(f, RK_HUBER, c[0], c[2], c[1], c[3]) for f, c in zip(fps, cases)]
    chi, _ = optimize_batch(hs, 8)
    for k in range(2):
        assert np.array_equal(np.asarray(chi[k])[:len(solo[0][k][0])], solo[0][k][0])
        for x, y in zip(hs[k].state(), solo[0][k][1]):
            assert np.array_equal(x, y)


# ---- covariance ----------------------------------------------------------------------------------------------------------------------
def test_covariances_are_those_of_the_weighted_hessian(g40):
    fp = flatten(g40)
    _, both, n = scenario(fp)
    kr = (np.concatenate([np.full(n, rb.HUBER), [rb.CAUCHY, rb.CAUCHY]]).astype(np.int32), np.concatenate([np.full(n, 1.0), [D95, D95]]))
    pri = make_priors(fp, [7, 30], seed=14)
    kp = kernels([rb.CAUCHY, rb.HUBER], [50.0, 40.0])
    h = solver(fp, RK_HUBER, both, pri, kr, kp)
    h.optimize(10)
    q, t, _ = h.state()
    w = rb.weights(kr, rr.rel_chi2(both, q, t, fp.Pf))
    assert np.any(w[:n] < 0.9) and np.all(w[-2:] < 0.1)          # (weights far from 1 take part)
    cov = h.covariance(landmarks=False)
    assert not cov["not_positive_definite"]
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    H = rb.system(o, fp, pri, both, kp, kr, 0.0)[0]
    Hi = np.linalg.inv(H)
    S_own = _dense_from_upper(*h.hsc(), fp.Pf)
    Si_own = np.linalg.inv(S_own)

    def worst_pose(Si):
        return max(np.abs(cov["pose"][p] - Si[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() / np.abs(Si[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() for p in range(fp.Pf))
    cond = np.linalg.cond(S_own)
    print("pose covariances: against the dense inverse of the model's weighted Hessian %.2e, of the library's own reduced matrix %.2e; cond(S) %.2e"
          % (worst_pose(Hi), worst_pose(Si_own), cond))
    assert worst_pose(Si_own) <= 1e-9
    assert worst_pose(Hi) <= 1e-9 + 10 * cond * np.finfo(np.float64).eps
    # the other two entry points see the same matrix
    key = (3, fp.Pf - 5)
    blk = h.covariance_blocks()[block_index(h)[key]]
    want = Si_own[6 * key[0]:6 * key[0] + 6, 6 * key[1]:6 * key[1] + 6]
    assert np.abs(blk - want).max() <= 1e-9 * np.abs(want).max()
    pairs, bad = h.covariance_pairs([("pose", key[0], "pose", key[1])])
    assert not bad and np.abs(pairs[0] - blk).max() <= 1e-12 * np.abs(blk).max()


def test_a_graph_held_only_by_a_tukey_zeroed_prior_is_not_positive_definite(g40):
    fp = flatten(freed(g40))
    assert fp.Pf == fp.Pt
    pri = make_priors(fp, [0], seed=11)
    q, t, _ = HipSolver(fp, RK_HUBER).state()
    e = pr.prior_chi2(pri, q, t, fp.Pf)[0]
    held = solver(fp, RK_HUBER, None, pri, kp=kernels([rb.TUKEY], [4 * e]))          # e / delta^2 = 1 / 4: weight 9 / 16
    assert not held.covariance(landmarks=False)["not_positive_definite"]
    loose = solver(fp, RK_HUBER, None, pri, kp=kernels([rb.TUKEY], [e / 4]))         # e / delta^2 = 4: weight 0, the gauge is free
    cov = loose.covariance(landmarks=False)
    assert cov["not_positive_definite"] and not cov["pose"].any()


def test_a_pose_held_only_by_a_tukey_zeroed_prior_is_not_positive_definite(g40):
    """the pose's diagonal block of the reduced matrix is exactly zero: no reprojection edge, and the prior's weight is 0"""
    p = 20
    fp = drop_edges(flatten(g40), [p])
    assert not np.any(np.asarray(fp.eP) == p)
    pri = make_priors(fp, [p], seed=12)
    q, t, _ = HipSolver(fp, RK_HUBER).state()
    e = pr.prior_chi2(pri, q, t, fp.Pf)[0]
    assert not solver(fp, RK_HUBER, None, pri).covariance(landmarks=False)["not_positive_definite"]
    cov = solver(fp, RK_HUBER, None, pri, kp=kernels([rb.TUKEY], [e / 4])).covariance(landmarks=False)
    assert cov["not_positive_definite"] and not cov["pose"].any()

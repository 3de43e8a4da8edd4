"""GPU parity tests on the BASELINE.json configurations and on the branches round 1 left untested.

Stated fp64 tolerances (asserted below, not just quoted):

  quantity                              default pcg_tol = 1e-7          pcg_tol = 1e-10
  per-iteration robust chi2 (relative)  <= 1e-6 (the north star's)      <= 1e-9
  final rotation    (quaternion RMSE)   <= 1e-8                         <= 1e-10
  final translation (RMSE, metres)      <= 1e-6                         <= 1e-9
  final landmarks   (RMSE, metres)      <= 1e-6                         <= 1e-9

RMSE is taken exactly as samples/sample_comparison_with_g2o.cpp:107-131 does (coefficient differences, root of
the mean squared norm per vertex).  The reference reports 7.6e-16 / 4.5e-13 / 4.5e-13 against g2o because both
sides factorise the same reduced matrix; an iterative reduced solve is bounded by its tolerance instead, which
is why the tolerance is stated per pcg_tol.  Repeat runs must be bit-identical (np.array_equal).

Stated fp32 tolerances (the USE_FLOAT32 build, libcuba_hip_f32.so; FP32_TOL below, asserted by test_float32_variant_at_size, and the
bench line's float32.<shape>.chi2_max_rel_diff_vs_fp64_golden must sit under the same numbers -- bench.py reads this table):

  shape     per-iteration robust chi2 vs the fp64 oracle (relative)   measured (round 5, driver's box)
  kitti00   <= 1e-5                                                     3.1e-6
  s2m       <= 5e-5                                                     --
  g4m       <= 5e-5                                                     1.1e-5
  estimates (all shapes): RMSE <= 1e-5 x the scene extent (fp32 resolves a 730 m coordinate of the S2M circuit to 6e-5 m and ten
  iterations accumulate that; measured 2.1e-3 m there), quaternion coefficients 1e-5 -- checked when the run completes all 10 iterations.
  "May stop early": an fp32 run may end after 8 or 9 of the 10 iterations, when the gain of a step falls below the resolution of its fp32
  chi2 sums and the gain ratio comes out <= 0 -- the reference's loop ends the same way (src/cuda_bundle_adjustment.cpp:851); at least 8
  iterations must run and every executed one must meet the chi2 bar.
"""
import copy
import os

import numpy as np
import pytest

from conftest import RK_HUBER, RK_NONE, RK_TUKEY
from cuba_amd.graph import Graph, flatten
from cuba_amd.synth import synth_ba, synth_named

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
EST_TOL = {"default": dict(chi2=1e-6, q=1e-8, t=1e-6, X=1e-6), "tight": dict(chi2=1e-9, q=1e-10, t=1e-9, X=1e-9)}
FP32_TOL = {"kitti00": 1e-5, "s2m": 5e-5, "g4m": 5e-5}          # per-iteration chi2 of the fp32 library vs the fp64 oracle; see the header
FP32_MIN_ITERATIONS = 8


def rmse(a, b):
    d = np.asarray(a) - np.asarray(b)
    return float(np.sqrt((d * d).sum(1).mean())) if len(d) else 0.0


def check_run(hip_chi2, hip_state, ref_chi2, ref_state, tol):
    assert len(hip_chi2) == len(ref_chi2)
    assert np.all(np.abs(hip_chi2 - ref_chi2) <= tol["chi2"] * ref_chi2), np.abs(hip_chi2 / ref_chi2 - 1).max()
    out = {}
    for name, a, b in zip("qtX", hip_state, ref_state):
        out[name] = rmse(a, b)
        assert out[name] <= tol[name], (name, out[name], tol[name])
    out["chi2"] = float(np.abs(hip_chi2 / ref_chi2 - 1).max())
    return out


@pytest.fixture(scope="module")
def solvers():
    from cuba_amd.capi import HipSolver
    from oracle.oracle import OracleSolver
    return HipSolver, OracleSolver


_cache = {}


def named_case(name, iters=10):
    """(FlatProblem, oracle chi2 trajectory, oracle final state) of a BASELINE shape, computed once per session."""
    if name not in _cache:
        from oracle.oracle import OracleSolver
        fp = flatten(synth_named(name))
        o = OracleSolver(fp, RK_HUBER)
        r = o.optimize(iters)
        _cache[name] = (fp, r["chi2"], o.state())
    return _cache[name]


# ---------------------------------------------------------------------------------------------------------
# BASELINE.json configs[1..4] at full size
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitti07", "kitti00", "s2m", "g4m"])
def test_baseline_shape_full_lm_parity(solvers, name):
    """10 LM iterations at full size against the oracle: chi2 per iteration, monotone decrease, final-estimate RMSE
    per quantity at the stated tolerance, PCG converged in every solve, bit-identical repeat."""
    HipSolver, _ = solvers
    fp, ref_chi2, ref_state = named_case(name)
    h = HipSolver(fp, RK_HUBER)
    q0, t0, X0 = h.state()
    got = h.optimize(10)["chi2"]
    assert np.all(np.diff(got) < 0)
    st = h.state()
    res = check_run(got, st, ref_chi2, ref_state, EST_TOL["default"])
    iters, bad = h.pcg_history()
    assert bad == 0 and len(iters) == 10 and np.all(iters > 0)
    print(f"\n[{name}] chi2 rel {res['chi2']:.2e}  RMSE q {res['q']:.2e} t {res['t']:.2e} X {res['X']:.2e}  "
          f"PCG iterations per solve {iters.tolist()}")
    h.set_state(q0, t0, X0)
    again = h.optimize(10)["chi2"]
    assert np.array_equal(again, got)                               # fixed summation order everywhere: bit-identical
    assert all(np.array_equal(a, b) for a, b in zip(h.state(), st))


CONFIG4_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config4_seeds_chi2.json")


@pytest.mark.parametrize("seed", list(range(100, 108)))
def test_config4_graphs_follow_the_oracle(solvers, seed):
    """BASELINE.json configs[3]: the eight independent KITTI-00-sized graphs `bench.py --gpus N` hands to rank 0..7 (seed
    100 + rank).  Protocol of samples/sample_comparison_with_g2o.cpp:89-110 per graph: the same 10 iterations on both sides,
    chi2 per iteration (<= 1e-6 relative, the north star's bar) and final-estimate RMSE per quantity at the stated default
    tolerance, against the live oracle; the committed golden trajectory every bench rank checks itself against
    (tests/golden/config4_seeds_chi2.json) must be that oracle run (<= 1e-12: same code, same thread count)."""
    import json
    HipSolver, OracleSolver = solvers
    fp = flatten(synth_named("kitti00", seed=seed))
    o = OracleSolver(fp, RK_HUBER); r = o.optimize(10)
    h = HipSolver(fp, RK_HUBER)
    got = h.optimize(10)["chi2"]
    res = check_run(got, h.state(), r["chi2"], o.state(), EST_TOL["default"])
    assert h.pcg_history()[1] == 0
    gold = json.load(open(CONFIG4_GOLDEN))["seeds"][str(seed)]
    assert (gold["P"], gold["L"], gold["E"]) == (fp.Pt, fp.Lt, fp.E)
    gchi = np.array(gold["chi2"])
    assert len(gchi) == len(r["chi2"]) and np.all(np.abs(gchi - r["chi2"]) <= 1e-12 * r["chi2"])
    assert gold["trials"] == [int(v) for v in r["trials"]]
    print(f"\n[config 4, seed {seed}] chi2 rel {res['chi2']:.2e}  RMSE q {res['q']:.2e} t {res['t']:.2e} X {res['X']:.2e}  "
          f"PCG iterations {int(h.counters()['pcg_iterations'])}")
    h.close()


@pytest.mark.parametrize("name", ["kitti00", "s2m"])
def test_tight_tolerance_estimates(solvers, name):
    """pcg_tol = 1e-10: the estimates agree with the exact-solve oracle to the nanometre."""
    HipSolver, _ = solvers
    fp, ref_chi2, ref_state = named_case(name)
    h = HipSolver(fp, RK_HUBER, pcg_tol=1e-10)
    got = h.optimize(10)["chi2"]
    res = check_run(got, h.state(), ref_chi2, ref_state, EST_TOL["tight"])
    print(f"\n[{name}, pcg_tol 1e-10] chi2 rel {res['chi2']:.2e}  RMSE q {res['q']:.2e} t {res['t']:.2e} X {res['X']:.2e}")


@pytest.mark.parametrize("name", ["kitti00", "s2m", "g4m"])
def test_float32_variant_at_size(solvers, name):
    """USE_FLOAT32 build (src/scalar.h:25-29) at the BASELINE sizes, G4M (configs[4]'s "plus USE_FLOAT32 variant" on one
    handle) included, against the fp32 bars of this file's header (FP32_TOL per shape, FP32_MIN_ITERATIONS)."""
    HipSolver, _ = solvers
    fp, ref_chi2, ref_state = named_case(name)
    h = HipSolver(fp, RK_HUBER, precision="f32")
    got = h.optimize(10)["chi2"]
    m = min(len(got), len(ref_chi2))
    assert m >= FP32_MIN_ITERATIONS                                  # fp32 may stop early once the gain is below its resolution
    dev = float(np.abs(got[:m] / ref_chi2[:m] - 1).max())
    print(f"\n[{name}, fp32 library] {m} iterations, chi2 vs the fp64 oracle {dev:.2e} (bar {FP32_TOL[name]:.0e})")
    assert dev <= FP32_TOL[name]
    if m == len(ref_chi2):
        for a, b in zip(h.state(), ref_state):
            assert rmse(a, b) < 1e-5 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", ["kitti00", "s2m"])
def test_mixed_precision_mode(solvers, name):
    """Option mixed_precision = 1 of the fp64 library: per-edge records and the per-edge arithmetic
    of the pose / block passes in fp32, every sum over edges, the reduced system and the PCG in fp64.  Stated tolerance:
    per-iteration chi2 <= 1e-6 relative (the fp64 bar -- the objective is evaluated in fp64 and is second-order in the
    linearisation error; measured 2.3e-8), estimates 1e-5 x scene extent RMSE (weakly observed directions move with the
    fp32 rounding of the Jacobians; measured 1.9e-4 m at KITTI-00, 1.1e-3 m at S2M), quaternion coefficients 1e-5."""
    HipSolver, _ = solvers
    fp, ref_chi2, ref_state = named_case(name)
    h = HipSolver(fp, RK_HUBER, mixed_precision=1)
    got = h.optimize(10)["chi2"]
    assert len(got) == len(ref_chi2) and np.all(np.abs(got - ref_chi2) <= CHI2_TOL * ref_chi2)
    for a, b in zip(h.state(), ref_state):
        assert rmse(a, b) < 1e-5 * max(1.0, np.abs(b).max())
    assert h.pcg_history()[1] == 0
    h2 = HipSolver(fp, RK_HUBER, mixed_precision=1)
    assert np.array_equal(h2.optimize(10)["chi2"], got)              # still bit-reproducible


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_g4m_eight_emulated_ranks(solvers, precision):
    """BASELINE configs[4] on one device: 8 solver handles + 8 native drivers (cuba_hip_dist_optimize) act as the 8 ranks
    of the landmark-partitioned mode (in-process communicator instead of RCCL) and must reproduce the oracle trajectory;
    "f32" = the config's USE_FLOAT32 variant (libcuba_hip_dist_f32.so over libcuba_hip_f32.so, chi2 to the fp32 bar 1e-4)."""
    import threading
    from cuba_amd.dist import NativeDist, ThreadComm
    HipSolver, _ = solvers
    fp, ref_chi2, ref_state = named_case("g4m")
    world, iters = 8, 4
    comms = ThreadComm.create(world)
    out, err = [None] * world, []
    tol = CHI2_TOL if precision == "f64" else 1e-4

    def work(c):
        try:
            d = NativeDist(HipSolver(fp, RK_HUBER, precision=precision), fp, c.rank, world, comm=c, precision=precision)
            out[c.rank] = (d.optimize(iters), d.counters(), d.reduction_parts()[0])
            d.close()
        except Exception as e:   # pragma: no cover
            err.append(e)
            c.s.barrier.abort()
    th = [threading.Thread(target=work, args=(c,)) for c in comms]
    [t.start() for t in th]; [t.join() for t in th]
    assert not err, err
    # (a reduced matrix of 16 MiB and more is summed in block-row parts, each under the rest of the Schur pass: parts + 1 all-reduces per trial)
    for chi2, c, parts in out:
        assert len(chi2) == iters and np.all(np.abs(chi2 - ref_chi2[:iters]) <= tol * ref_chi2[:iters])
        assert parts == out[0][2] and (parts >= 2 if precision == "f64" else parts >= 1)
        assert c["large_allreduces"] == iters * (parts + 1 if parts > 1 else 1) + 1 and c["lm_trials"] == iters
    assert all(np.array_equal(out[0][0], o[0]) for o in out[1:])    # replicas stay bit-identical


# ---------------------------------------------------------------------------------------------------------
# branches without a test in round 1
# ---------------------------------------------------------------------------------------------------------
def test_rejected_trials_follow_the_oracle(solvers):
    """A start far enough out that some LM trials are rejected (rho < 0 -> pop, lambda *= nu): the whole trajectory,
    trial count included, must follow the oracle (ref src/cuda_bundle_adjustment.cpp:836-846)."""
    HipSolver, OracleSolver = solvers
    fp = flatten(synth_ba(60, 1500, 6000, seed=3))
    rng = np.random.default_rng(1)
    fp.Xw = fp.Xw + rng.normal(0, 3.0, fp.Xw.shape)
    fp.t = fp.t.copy(); fp.t[:fp.Pf] += rng.normal(0, 0.6, (fp.Pf, 3))
    o = OracleSolver(fp, RK_TUKEY); r = o.optimize(12)
    assert r["trials"].max() > 1                                    # the case really rejects trials
    h = HipSolver(fp, RK_TUKEY, pcg_tol=1e-10)
    got = h.optimize(12)["chi2"]
    assert len(got) == len(r["chi2"]) and np.all(np.abs(got - r["chi2"]) <= CHI2_TOL * r["chi2"])
    assert h.counters()["lm_trials"] == int(r["trials"].sum())


def test_pcg_max_iter_is_reported(solvers):
    """A solve that stops at pcg_max_iter must not pass silently (ref failure path: cuda_linear_solver.cpp:406-410)."""
    HipSolver, OracleSolver = solvers
    fp = flatten(synth_ba(200, 8000, 32000, seed=13))
    o = OracleSolver(fp, RK_HUBER); o.compute_errors(); o.build_system()
    lam = 1e-7 * o.max_diagonal()
    # (with the exact fallback switched off: the failure report of a handle whose reduced system is too large for the dense solver)
    h = HipSolver(fp, RK_HUBER, pcg_max_iter=8, pcg_tol=1e-12, pcg_aggregate=0, direct_fallback=0)
    h.set_lambda(lam)
    assert h.solve() is False                                       # reported as a failed solve
    it, bad = h.pcg_history()
    assert bad == 1 and it[-1] == -8 and h.counter("exact_solve_fallbacks") == 0
    h2 = HipSolver(fp, RK_HUBER, pcg_max_iter=8, pcg_tol=1e-12, pcg_aggregate=0, pcg_accept_unconverged=1)
    h2.set_lambda(lam)
    assert h2.solve() is True and h2.pcg_history()[1] == 1          # opt-in: best iterate, still counted
    # inside optimize() the trial is rejected and lambda raised until the system is easy enough (or the run stops)
    h3 = HipSolver(fp, RK_HUBER, pcg_max_iter=8, pcg_tol=1e-9, pcg_aggregate=0, direct_fallback=0)
    chi2 = h3.optimize(3)["chi2"]
    it3, bad3 = h3.pcg_history()
    assert bad3 >= 1 and (len(chi2) == 0 or np.all(np.diff(chi2) <= 0))
    # the default: the solve that ran out of iterations is finished EXACTLY on the device (csrc/ba_direct.hip; the reference's solve is
    # exact, src/cuda_linear_solver.cpp:386-415) -- same increment as the exact-solve oracle, and the run follows the oracle's
    h5 = HipSolver(fp, RK_HUBER, pcg_max_iter=8, pcg_tol=1e-12, pcg_aggregate=0)
    h5.set_lambda(lam)
    assert h5.solve() is True and h5.counter("exact_solve_fallbacks") == 1 and h5.pcg_history()[0][-1] == -8
    o.set_lambda(lam); assert o.solve()
    assert np.abs(h5.array("xp") - o.array("xp")).max() <= 1e-9 * np.abs(o.array("xp")).max()
    h6 = HipSolver(fp, RK_HUBER, pcg_max_iter=8, pcg_aggregate=0)
    got = h6.optimize(5)["chi2"]
    want = OracleSolver(fp, RK_HUBER).optimize(5)["chi2"]
    assert len(got) == len(want) and np.all(np.abs(got - want) <= 1e-9 * want)
    assert h6.counter("exact_solve_fallbacks") == h6.counters()["lm_trials"] and h6.counter("exact_solve_failures") == 0
    # default settings on the same graph converge everywhere
    h4 = HipSolver(fp, RK_HUBER)
    h4.optimize(5)
    assert h4.pcg_history()[1] == 0


def shuffled_pose_ids(g, seed=0):
    """Same graph, pose ids randomly permuted: solver indices (assigned in id order) no longer follow the trajectory."""
    rng = np.random.default_rng(seed)
    P = g.nposes
    perm = rng.permutation(P)
    perm[perm == 0], perm[0] = perm[0], 0                           # keep id 0 on row 0 (the fixed pose)
    h = copy.deepcopy(g)
    lut = np.zeros(int(g.pose_ids.max()) + 1, dtype=np.int64)
    lut[g.pose_ids] = perm
    h.pose_ids = perm.astype(np.int64)
    h.mono_vp = lut[g.mono_vp]; h.stereo_vp = lut[g.stereo_vp]
    return h


@pytest.mark.parametrize("name", ["kitti07", "kitti00"])
def test_shuffled_pose_ids(solvers, name):
    """The two-level preconditioner's aggregates are runs of consecutive pose indices.  With shuffled pose ids the caller's
    solver order no longer follows the trajectory; the library then renumbers the free poses internally (strongest-neighbour
    walk over the co-visibility counts, option pose_reorder).  Parity must hold, every solve must converge, the iteration
    counts must stay those of the id-ordered graph, and without the renumbering they do not (recorded)."""
    HipSolver, OracleSolver = solvers
    g = synth_named(name)
    fp_ord = flatten(g)
    fp = flatten(shuffled_pose_ids(g, seed=5))
    assert fp.Pt == fp_ord.Pt and not np.array_equal(fp.eP, fp_ord.eP)
    o = OracleSolver(fp, RK_HUBER); r = o.optimize(10)
    h = HipSolver(fp, RK_HUBER)
    got = h.optimize(10)["chi2"]
    check_run(got, h.state(), r["chi2"], o.state(), EST_TOL["default"])
    it, bad = h.pcg_history()
    assert bad == 0
    ho = HipSolver(fp_ord, RK_HUBER); ho.optimize(10)
    it_ord = ho.pcg_history()[0]
    hn = HipSolver(fp, RK_HUBER, pose_reorder=0, direct_fallback=0); hn.optimize(10)      # (the PCG alone: no hand-over to the exact solver)
    it_raw = hn.pcg_history()[0]
    print(f"\n[{name}] PCG iterations per solve: id-ordered {it_ord.tolist()}  shuffled {it.tolist()}  shuffled, pose_reorder=0 {np.abs(it_raw).tolist()}")
    assert it.sum() <= 1.15 * it_ord.sum()                           # the walk recovers the trajectory
    assert np.abs(it_raw).sum() > 3 * it_ord.sum()                   # ... which is what the preconditioner needs
    # the same physical problem: chi2 agrees with the id-ordered run to solver tolerance
    ref_ord = named_case(name)[1]
    assert np.all(np.abs(got - ref_ord) <= CHI2_TOL * ref_ord)


def test_exact_solver_for_every_solve(solvers):
    """Option reduced_solver = 1: EVERY reduced solve is the exact sparse Cholesky (the reference's behaviour: its SparseLinearSolver is the
    only solver it has, src/cuda_linear_solver.cpp:386-415) -- on an id-ordered graph, on shuffled pose ids (the solver's tile order is
    built on the INTERNAL pose order, its increment comes back in the caller's), and with fixed vertices: the oracle's trajectory to 1e-9 (both
    sides solve exactly), estimates to 1e-9 m, no PCG iteration at all, repeat runs bit-identical; one solve's increment against the oracle's."""
    from conftest import with_fixed
    HipSolver, OracleSolver = solvers
    g = synth_ba(200, 8000, 32000, seed=13)
    for label, gg in (("ordered", g), ("shuffled ids", shuffled_pose_ids(g, seed=2)), ("fixed vertices", with_fixed(g, fixed_pose_rows=[3, 4, 20], fixed_lm_rows=list(range(0, 300, 7))))):
        fp = flatten(gg)
        o = OracleSolver(fp, RK_HUBER); ro = o.optimize(8)["chi2"]
        h = HipSolver(fp, RK_HUBER, reduced_solver=1); rh = h.optimize(8)["chi2"]
        assert len(rh) == len(ro) and np.all(np.abs(rh - ro) <= 1e-9 * ro), (label, np.abs(rh / ro - 1).max())
        for a, b in zip(h.state(), o.state()):
            assert np.abs(a - b).max() <= 1e-9, label
        assert h.counter("pcg_iterations") == 0 and h.counter("exact_solve_fallbacks") == h.counters()["lm_trials"] and h.counter("exact_solve_failures") == 0, label
        h2 = HipSolver(fp, RK_HUBER, reduced_solver=1)
        assert np.array_equal(h2.optimize(8)["chi2"], rh), label
        o2 = OracleSolver(fp, RK_HUBER); o2.compute_errors(); o2.build_system(); lam = 1e-6 * o2.max_diagonal(); o2.set_lambda(lam); assert o2.solve()
        h2.set_state(fp.q, fp.t, fp.Xw); h2.max_diagonal(); h2.set_lambda(lam); assert h2.solve()
        assert np.abs(h2.array("xp") - o2.array("xp")).max() <= 1e-9 * np.abs(o2.array("xp")).max(), label


def test_fifty_thousand_poses(solvers):
    """Five times configs[4]'s pose count (50 000 / 250 000 / 1 000 000): beyond round 5's limits in three places -- the dense exact solver
    refused above 10 922 poses (the sparse one factorises this trajectory's 10 000 tile columns), the aggregate size rule of the two-level
    preconditioner doubled without end beyond ~47 000 poses and died in an integer division (it now lands on the footprint-minimising
    aggregate), and the row-update launch of the upper-triangle iteration truncated aggregates above 170 poses.  No oracle at this size in
    the suite's time budget: the two reduced solvers of the library check each other -- the block PCG (default) against an exact solve in
    every trial (reduced_solver = 1) -- over three LM iterations, and one increment to 1e-5."""
    HipSolver, _ = solvers
    fp = flatten(synth_ba(50000, 250000, 1000000, seed=50))
    assert fp.Pf > 49000
    a = HipSolver(fp, RK_HUBER); ra = a.optimize(3)["chi2"]
    c = a.counters()
    b = HipSolver(fp, RK_HUBER, reduced_solver=1); rb = b.optimize(3)["chi2"]
    print(f"\n[50 k poses] chi2 {ra.tolist()} (PCG: iterations per solve {a.pcg_history()[0].tolist()}, coarse dimension {c['coarse_dim']}, "
          f"exact hand-overs {a.counter('exact_solve_fallbacks')}) vs {rb.tolist()} (exact: {b.counter('exact_solve_fallbacks')} solves)")
    assert len(ra) == len(rb) == 3 and np.all(np.diff(ra) < 0)
    assert np.all(np.abs(ra - rb) <= 1e-6 * rb), np.abs(ra / rb - 1).max()
    assert c["coarse_dim"] > 0                                       # the two-level preconditioner is in force at this size
    assert b.counter("exact_solve_fallbacks") == b.counters()["lm_trials"] and b.counter("exact_solve_failures") == 0 and b.counter("pcg_iterations") == 0
    lam = 1e-5 * a.max_diagonal()
    a.set_option("pcg_tol", 1e-11); a.set_option("direct_fallback", 0); a.set_lambda(lam); assert a.solve()
    b.max_diagonal(); b.set_lambda(lam); assert b.solve()
    xa, xb = a.array("xp"), b.array("xp")
    # (the PCG's tolerance bounds its residual in the preconditioned norm; at this size the increment's error is ~1e5 times that)
    assert np.abs(xa - xb).max() <= 1e-5 * np.abs(xb).max(), np.abs(xa - xb).max() / np.abs(xb).max()


def test_shuffled_pose_ids_stage_outputs_keep_the_callers_numbering(solvers):
    """With the internal renumbering active every host-pointer entry point still speaks the caller's pose order: bp, bsc, xp,
    the block pattern and the block values of Hsc, the solution -- all against the oracle in the caller's order; set_state /
    state round-trip; a landmark partition (which runs in the caller's order) after the renumbering."""
    HipSolver, OracleSolver = solvers
    fp = flatten(shuffled_pose_ids(synth_ba(200, 8000, 32000, seed=13), seed=2))
    o = OracleSolver(fp, RK_HUBER); o.compute_errors(); o.build_system()
    md = o.max_diagonal(); lam = 1e-5 * md
    h = HipSolver(fp, RK_HUBER, pcg_tol=1e-11)
    assert h.max_diagonal() == pytest.approx(md, rel=1e-12)
    o.set_lambda(lam); h.set_lambda(lam); o.schur(); h.schur()
    rpo, cio, vo = o.hsc(); rp, ci, v = h.hsc()
    assert np.array_equal(rp, rpo) and np.array_equal(ci, cio)
    diag = np.zeros(len(ci), bool); diag[rp[:-1]] = True
    scale = np.abs(vo).max()
    assert np.abs(v[~diag] - vo[~diag]).max() <= 1e-9 * scale
    iu = np.triu_indices(6)
    assert np.abs((v[diag][:, iu[0], iu[1]] + lam * (iu[0] == iu[1])) - vo[diag][:, iu[0], iu[1]]).max() <= 1e-9 * scale
    for name in ("bp", "bsc"):
        a, b = h.array(name), o.array(name)
        assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max(), name
    assert o.solve() and h.solve_reduced()
    xo = o.array("xp")
    assert np.abs(h.array("xp") - xo).max() <= 1e-6 * np.abs(xo).max()
    q0, t0, X0 = h.state()
    assert np.array_equal(q0, fp.q) and np.array_equal(t0, fp.t)      # untouched estimates come back in the caller's order
    h.set_state(q0 * 1.0, t0 + 0.0, X0)
    assert all(np.array_equal(a, b) for a, b in zip(h.state(), (q0, t0, X0)))
    # the renumbering really was active: at weak damping the caller's order needs several times the iterations
    h.set_lambda(1e-9 * md); assert h.solve()
    hn = HipSolver(fp, RK_HUBER, pcg_tol=1e-11, pose_reorder=0, direct_fallback=0); hn.set_lambda(1e-9 * md); assert hn.solve()
    assert 1.2 * h.pcg_history()[0][-1] < hn.pcg_history()[0][-1], (h.pcg_history()[0], hn.pcg_history()[0])
    # a landmark partition set on a renumbered handle: back to the caller's order, same results as a fresh handle
    ref = OracleSolver(fp, RK_HUBER).optimize(3)["chi2"]
    h2 = HipSolver(fp, RK_HUBER); h2.build_structure()
    h2.set_partition(0, fp.Lt)
    assert np.all(np.abs(h2.optimize(3)["chi2"] - ref) <= CHI2_TOL * ref)


def dense_normal_equations(o, fp, lam):
    """Full (6Pf + 3Lf)^2 system from the oracle's blocks (Hpl per edge, summed per (pose, landmark))."""
    Pf, Lf = fp.Pf, fp.Lf
    n = 6 * Pf + 3 * Lf
    H = np.zeros((n, n))
    Hpp = o.array("Hpp").reshape(Pf, 6, 6).transpose(0, 2, 1)      # col-major blocks -> [row][col]
    Hll = o.array("Hll").reshape(Lf, 3, 3).transpose(0, 2, 1)
    Hpl = o.array("Hpl").reshape(fp.E, 3, 6).transpose(0, 2, 1)    # 6x3 col-major -> [6][3]
    for i in range(Pf):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Hpp[i]
    for l in range(Lf):
        a = 6 * Pf + 3 * l
        H[a:a + 3, a:a + 3] = Hll[l]
    for e in range(fp.E):
        p, l = fp.eP[e], fp.eL[e]
        if p < Pf and l < Lf:
            a = 6 * Pf + 3 * l
            H[6 * p:6 * p + 6, a:a + 3] += Hpl[e]
            H[a:a + 3, 6 * p:6 * p + 6] += Hpl[e].T
    H[np.diag_indices(n)] += lam
    b = np.concatenate([o.array("bp"), o.array("bl")])
    return H, b


def graph_with_duplicate_observations():
    """the 40-pose graph with 80 stereo edges observed again as monocular ones and 40 monocular edges duplicated: 120 second
    observations of a landmark by the same pose"""
    g = copy.deepcopy(synth_ba(40, 600, 2400, seed=1))
    rng = np.random.default_rng(2)
    pick_s = rng.choice(len(g.stereo_vp), 80, replace=False)        # stereo edges observed again as monocular ones
    g.mono_vp = np.concatenate([g.mono_vp, g.stereo_vp[pick_s]]); g.mono_vl = np.concatenate([g.mono_vl, g.stereo_vl[pick_s]])
    g.mono_meas = np.concatenate([g.mono_meas, g.stereo_meas[pick_s, :2] + rng.normal(0, 0.5, (80, 2))])
    g.mono_info = np.concatenate([g.mono_info, g.stereo_info[pick_s]])
    pick_m = rng.choice(len(g.mono_vp) - 80, 40, replace=False)     # and monocular ones duplicated as monocular
    g.mono_vp = np.concatenate([g.mono_vp, g.mono_vp[pick_m]]); g.mono_vl = np.concatenate([g.mono_vl, g.mono_vl[pick_m]])
    g.mono_meas = np.concatenate([g.mono_meas, g.mono_meas[pick_m] + rng.normal(0, 0.5, (40, 2))])
    g.mono_info = np.concatenate([g.mono_info, g.mono_info[pick_m]])
    return g


def test_duplicate_observations_of_one_pose(solvers):
    """Two observations of one landmark by the SAME pose (a monocular and a stereo edge): the diagonal-block branch of
    the block pass (a == b).  Checked against a dense solve of the full normal equations -- the mathematically
    complete Schur complement (T + T^T on the diagonal block; the reference and hence the oracle's literal restatement
    add only T there)."""
    HipSolver, OracleSolver = solvers
    g = graph_with_duplicate_observations()
    fp = flatten(g)
    key = fp.eP.astype(np.int64) * fp.Lt + fp.eL
    assert len(np.unique(key)) == fp.E - 120
    o = OracleSolver(fp, RK_HUBER); o.compute_errors(); o.build_system()
    md = o.max_diagonal(); lam = 1e-5 * md
    H, b = dense_normal_equations(o, fp, lam)
    x = np.linalg.solve(H, b)
    for opts in (dict(), dict(device_setup=0)):
        h = HipSolver(fp, RK_HUBER, pcg_tol=1e-12, **opts)
        assert h.max_diagonal() == pytest.approx(md, rel=1e-12)
        h.set_lambda(lam); assert h.solve()
        xp, xl = h.array("xp"), h.array("xl")
        assert np.abs(xp - x[:6 * fp.Pf]).max() <= 1e-7 * np.abs(x[:6 * fp.Pf]).max()
        assert np.abs(xl - x[6 * fp.Pf:]).max() <= 1e-7 * np.abs(x[6 * fp.Pf:]).max()
        # the reduced matrix itself: Hsc = Hpp + lam - Hpl (Hll + lam)^-1 Hpl^T, upper block triangle
        n6 = 6 * fp.Pf
        S = H[:n6, :n6] - H[:n6, n6:] @ np.linalg.solve(H[n6:, n6:], H[n6:, :n6])
        rp, ci, v = h.hsc()
        for i in range(fp.Pf):
            for k in range(rp[i], rp[i + 1]):
                j = ci[k]
                blk = S[6 * i:6 * i + 6, 6 * j:6 * j + 6].copy()
                got = v[k].copy()
                if i == j:                                             # (the PCG set-up of solve() has already added lambda in place)
                    iu = np.triu_indices(6)
                    assert np.abs(got[iu] - blk[iu]).max() <= 1e-9 * md
                else:
                    assert np.abs(got - blk).max() <= 1e-9 * md
    # and a whole LM run stays a descent
    chi2 = HipSolver(fp, RK_HUBER).optimize(6)["chi2"]
    assert len(chi2) == 6 and np.all(np.diff(chi2) < 0)


def hub_graph():
    """synth_ba(150, ...) plus far landmarks that make pose 75 co-visible with more than 60 others"""
    from scipy.spatial.transform import Rotation
    g = copy.deepcopy(synth_ba(150, 3000, 12000, seed=8))
    rng = np.random.default_rng(3)
    hub = 75     # this pose additionally observes far landmarks (in front of it, anywhere in its image plane) of > 60 other poses
    R = Rotation.from_quat(g.truth["q"][hub]).as_matrix(); t = g.truth["t"][hub]; cam = g.pose_cam[hub]
    Xc = g.truth["Xw"] @ R.T + t
    vis = (Xc[:, 2] > 6) & (Xc[:, 2] < 400)
    row = {int(i): r for r, i in enumerate(g.lm_ids)}
    vp = np.concatenate([g.mono_vp, g.stereo_vp]); vl = np.concatenate([g.mono_vl, g.stereo_vl])
    lrow = np.array([row[int(l)] for l in vl])
    seen_by_hub = set(lrow[vp == hub].tolist())
    covered, pick = set(), []
    for r in np.nonzero(vis)[0]:
        if r in seen_by_hub:
            continue
        ps = set(vp[lrow == r].tolist()) - covered - {hub}
        if len(ps) >= 2 or (len(ps) >= 1 and len(covered) < 70):
            pick.append(r); covered |= ps
        if len(covered) > 90:
            break
    pick = np.array(pick)
    u = cam[0] * Xc[pick, 0] / Xc[pick, 2] + cam[2]; v = cam[1] * Xc[pick, 1] / Xc[pick, 2] + cam[3]
    g.mono_vp = np.concatenate([g.mono_vp, np.full(len(pick), hub)]); g.mono_vl = np.concatenate([g.mono_vl, g.lm_ids[pick]])
    g.mono_meas = np.concatenate([g.mono_meas, np.stack([u, v], 1) + rng.normal(0, 1, (len(pick), 2))])
    g.mono_info = np.concatenate([g.mono_info, np.ones(len(pick))])
    return g


def test_block_rows_wider_than_the_fixed_width_rows(solvers):
    """One pose co-visible with more than 60 others: its block row leaves the fixed-width part of the SpMV
    (DeviceStructure::ell_over).  PCG solution vs the oracle's exact Cholesky, and the LM trajectory."""
    HipSolver, OracleSolver = solvers
    fp = flatten(hub_graph())
    o = OracleSolver(fp, RK_HUBER); o.compute_errors(); o.build_system()
    lam = 1e-6 * o.max_diagonal()
    o.set_lambda(lam); assert o.solve()
    h = HipSolver(fp, RK_HUBER, pcg_tol=1e-11)
    rp, ci = h.hsc_structure()
    width = np.diff(rp).astype(np.int64)
    np.add.at(width, ci, 1)                                         # symmetric adjacency: lower entries
    width -= 1                                                      # the diagonal was counted twice
    assert width.max() > 60, width.max()
    h.set_lambda(lam); assert h.solve()
    xo = o.array("xp")
    assert np.abs(h.array("xp") - xo).max() <= 1e-6 * np.abs(xo).max()
    r = OracleSolver(fp, RK_HUBER).optimize(6)
    got = HipSolver(fp, RK_HUBER).optimize(6)["chi2"]
    assert len(got) == len(r["chi2"]) and np.all(np.abs(got - r["chi2"]) <= CHI2_TOL * r["chi2"])


def test_device_and_host_setup_agree(solvers, small_graph):
    """The set-up built on the GPU (edge sort, block pattern, product lists, adjacency, coarse lists, wave list:
    csrc/ba_structure.hip) against the host pipeline (option device_setup = 0, also what landmark-partitioned handles use):
    same block pattern, bit-identical LM runs -- every list must come out in the same order for that."""
    from conftest import with_fixed
    HipSolver, _ = solvers
    g_big = synth_named("kitti07")
    cases = [flatten(small_graph), flatten(with_fixed(small_graph, fixed_pose_rows=[3, 4, 5, 20], fixed_lm_rows=list(range(0, 300, 7)))),
             flatten(with_fixed(small_graph, fixed_lm_rows=range(small_graph.nlandmarks))),          # pose-only: no landmark is free
             flatten(shuffled_pose_ids(g_big, seed=3)), flatten(g_big)]
    for fp in cases:
        # (pose_reorder = 0, landmark_reorder = 0: the internal renumberings of poses and landmarks exist in the device pipeline only)
        a = HipSolver(fp, RK_HUBER, pose_reorder=0, landmark_reorder=0); b = HipSolver(fp, RK_HUBER, device_setup=0)
        ra, rb = a.optimize(6)["chi2"], b.optimize(6)["chi2"]
        if fp.Pf and fp.Lf:
            (rpa, cia), (rpb, cib) = a.hsc_structure(), b.hsc_structure()
            assert np.array_equal(rpa, rpb) and np.array_equal(cia, cib)
            ca, cb = a.counters(), b.counters()
            assert ca["hsc_blocks"] == cb["hsc_blocks"] and ca["schur_products"] == cb["schur_products"] and ca["coarse_dim"] == cb["coarse_dim"]
        assert np.array_equal(ra, rb)
        assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state()))
        assert np.array_equal(a.chi_squares(), b.chi_squares())               # caller order restored on the device / on the host


def pairwise_graph(P, L, seed=0):
    """Sparsest possible co-visibility: every landmark is seen by exactly two poses and no two landmarks share their pose pair,
    so every Schur product opens its own off-diagonal block (nblk = Pf + L, 2 nblk - Pf adjacency entries > E).  A cluster of
    cameras looking down +z at a cloud of points in front of all of them."""
    from scipy.spatial.transform import Rotation
    from cuba_amd.synth import KITTI00_CAM, IMG_W, IMG_H
    rng = np.random.default_rng(seed)
    cam = KITTI00_CAM
    C = np.stack([rng.uniform(-1.5, 1.5, P), rng.uniform(-0.3, 0.3, P), rng.uniform(-0.5, 0.5, P)], 1)
    Rcw = Rotation.from_rotvec(rng.normal(0, np.deg2rad(1.5), (P, 3))).as_matrix()
    t = -np.einsum("nij,nj->ni", Rcw, C)
    assert L <= (P - 1) * (P - 2) // 2
    iu = np.stack(np.triu_indices(P, 1), 1)
    with0 = iu[iu[:, 0] == 0]; rest = iu[iu[:, 0] != 0]             # only a few pairs with the fixed pose 0 (those open no block)
    n0 = min(20, len(with0))
    pairs = np.concatenate([with0[rng.choice(len(with0), n0, replace=False)], rest[rng.choice(len(rest), L - n0, replace=False)]])
    z = rng.uniform(10, 35, L)
    X = np.stack([rng.uniform(-0.45, 0.45, L) * z, rng.uniform(-0.12, 0.12, L) * z, z], 1)
    ep = pairs.reshape(-1); el = np.repeat(np.arange(L), 2)
    Xc = np.einsum("nij,nj->ni", Rcw[ep], X[el]) + t[ep]
    u = cam[0] * Xc[:, 0] / Xc[:, 2] + cam[2]; v = cam[1] * Xc[:, 1] / Xc[:, 2] + cam[3]
    assert np.all((u > 0) & (u < IMG_W) & (v > 0) & (v < IMG_H) & (Xc[:, 2] > 4))
    meas = np.stack([u, v, u - cam[4] / Xc[:, 2]], 1) + rng.normal(0, 0.7, (2 * L, 3))
    q = Rotation.from_matrix(Rcw).as_quat(); q[q[:, 3] < 0] *= -1
    q0 = (Rotation.from_rotvec(rng.normal(0, np.deg2rad(0.3), (P, 3))) * Rotation.from_matrix(Rcw)).as_quat(); q0[q0[:, 3] < 0] *= -1
    q0[0] = q[0]
    t0 = t + rng.normal(0, 0.03, (P, 3)); t0[0] = t[0]
    fixed = np.zeros(P, bool); fixed[0] = True
    return Graph(pose_ids=np.arange(P, dtype=np.int64), pose_fixed=fixed, pose_q=q0, pose_t=t0, pose_cam=np.tile(cam, (P, 1)),
                 lm_ids=np.arange(P, P + L, dtype=np.int64), lm_fixed=np.zeros(L, bool), lm_X=X + rng.normal(0, 0.1, (L, 3)),
                 mono_vp=np.zeros(0, np.int64), mono_vl=np.zeros(0, np.int64), mono_meas=np.zeros((0, 2)), mono_info=np.zeros(0),
                 stereo_vp=ep.astype(np.int64), stereo_vl=el.astype(np.int64) + P, stereo_meas=meas, stereo_info=np.ones(2 * L))


def test_sparse_covisibility_every_product_its_own_block(solvers):
    """Each landmark observed twice, all pose pairs distinct: the symmetric adjacency (2 nblk - Pf entries) is longer than both the
    edge list and the pattern-entry list, which sized the scratch arrays of the device set-up (round-2 advisor finding: the head-flag /
    scan scratch of the coarse lists was too small for exactly this shape).  Device set-up == host set-up bit for bit, both follow
    the oracle, the block pattern is the oracle's."""
    HipSolver, OracleSolver = solvers
    fp = flatten(pairwise_graph(64, 1900, seed=3))
    assert fp.E == 2 * fp.Lt
    o = OracleSolver(fp, RK_HUBER); r = o.optimize(6)
    a = HipSolver(fp, RK_HUBER, pose_reorder=0, landmark_reorder=0); b = HipSolver(fp, RK_HUBER, device_setup=0)
    ra, rb = a.optimize(6)["chi2"], b.optimize(6)["chi2"]
    c = a.counters()
    assert 2 * c["hsc_blocks"] - fp.Pf > fp.E > fp.Pf + fp.Lt                                # the shape the finding is about
    assert np.array_equal(ra, rb) and all(np.array_equal(x, y) for x, y in zip(a.state(), b.state()))
    assert len(ra) == len(r["chi2"]) and np.all(np.abs(ra - r["chi2"]) <= CHI2_TOL * r["chi2"])
    (rpa, cia), (rpo, cio, _) = a.hsc_structure(), o.hsc()
    assert np.array_equal(rpa, rpo) and np.array_equal(cia, cio)
    # with the automatic pose renumbering on (the default) the run is the same physical problem
    d = HipSolver(fp, RK_HUBER).optimize(6)["chi2"]
    assert np.all(np.abs(d - r["chi2"]) <= CHI2_TOL * r["chi2"])


# ---------------------------------------------------------------------------------------------------------
# known-answer test on the reference's real data, when somebody supplies it
# ---------------------------------------------------------------------------------------------------------
README_CHI2_KITTI00 = [334210.0, 331822.8, 329700.4, 327743.4, 326123.2, 324876.6, 323698.5, 322572.7, 321410.3, 320086.4]


def _kitti_path(name):
    for d in (os.environ.get("CUBA_BA_INPUT_DIR"), os.path.join(os.path.dirname(__file__), "data"),
              os.path.join(os.path.dirname(__file__), "..", "samples", "ba_input")):
        if d and os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return None


@pytest.mark.skipif(_kitti_path("ba_kitti_00.json") is None,
                    reason="samples/ba_input.7z of the reference is not in this image (.MISSING_LARGE_BLOBS); set CUBA_BA_INPUT_DIR")
def test_readme_known_answer_kitti00(solvers):
    """README.md:141-150,176-186 of the reference: chi2 of 10 iterations on ba_kitti_00.json, Huber deltas
    sqrt(5.991) / sqrt(7.815), printed to 0.1.  The README shows the same table for sample_ba_from_file (no warm-up,
    samples/sample_ba_from_file.cpp:53-54) and for sample_comparison_with_g2o (1-iteration warm-up first, :303-307);
    both protocols are tried and one of them must reproduce the table."""
    HipSolver, _ = solvers
    fp = flatten(Graph.from_json(_kitti_path("ba_kitti_00.json")))
    assert (fp.Lt, fp.E) == (133383, 561116)
    ok = []
    for warm in (0, 1):
        h = HipSolver(fp, RK_HUBER, pcg_tol=1e-10)
        if warm:
            h.optimize(1)
        got = h.optimize(10)["chi2"]
        ok.append(len(got) == 10 and np.abs(got - README_CHI2_KITTI00).max() <= 0.051)
    assert any(ok), ok


@pytest.mark.parametrize("seed", range(8))
def test_random_graphs_device_setup_host_setup_oracle(solvers, seed):
    """Small random graphs with the irregularities the set-up code has to survive: random fixed poses / landmarks, landmarks
    and free poses that lost all their edges (empty segments, diagonal-only block rows), mono-only landmarks, shuffled edge
    order.  Device-built and host-built structures must give bit-identical runs, and both must follow the oracle."""
    from conftest import with_fixed
    HipSolver, OracleSolver = solvers
    rng = np.random.default_rng(1000 + seed)
    P = int(rng.integers(10, 70)); L = int(rng.integers(40, 500)); E = int(L * rng.uniform(2.2, min(4.5, max(2.4, P / 3.0))))
    g = synth_ba(P, L, E, seed=int(rng.integers(0, 1 << 30)), stereo_frac=float(rng.uniform(0.3, 1.0)))
    g = with_fixed(g, fixed_pose_rows=rng.choice(P, size=int(rng.integers(0, max(1, P // 5))), replace=False),
                   fixed_lm_rows=rng.choice(L, size=int(rng.integers(0, max(1, L // 6))), replace=False))
    fp = flatten(g)
    # some landmarks (and, for the smaller graphs, one free pose) lose all their edges AFTER the index assignment
    drop_l = rng.choice(fp.Lt, size=max(1, fp.Lt // 20), replace=False)
    dead = np.isin(fp.eL, drop_l)
    if fp.Pf > 3 and seed % 2:
        dead |= fp.eP == int(rng.integers(1, fp.Pf))
    keep = np.nonzero(~dead)[0]
    keep = keep[rng.permutation(len(keep))]                       # and the caller's edge order is arbitrary
    for name in ("eP", "eL", "eDim", "omega", "meas", "edge_src"):
        setattr(fp, name, np.ascontiguousarray(getattr(fp, name)[keep]))
    o = OracleSolver(fp, RK_HUBER); r = o.optimize(5)
    a = HipSolver(fp, RK_HUBER, landmark_reorder=0); b = HipSolver(fp, RK_HUBER, device_setup=0)      # (the landmark renumbering is the device pipeline's)
    ra, rb = a.optimize(5)["chi2"], b.optimize(5)["chi2"]
    assert np.array_equal(ra, rb)
    assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state()))
    assert np.array_equal(a.chi_squares(), b.chi_squares())
    assert len(ra) == len(r["chi2"]) and np.all(np.abs(ra - r["chi2"]) <= CHI2_TOL * np.maximum(r["chi2"], 1e-30))
    if fp.Pf and fp.Lf:
        (rpa, cia), (rpo, cio, _) = a.hsc_structure(), o.hsc()
        assert np.array_equal(rpa, rpo) and np.array_equal(cia, cio)

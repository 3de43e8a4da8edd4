"""Whole Levenberg-Marquardt runs on the smallest graphs that end each way, under the three drivers of the loop -- `chain' (cuba_hip_optimize:
the device-decided run), `profile' (profile = 1: the host loop of cuba_hip_solver::optimize) and `batch' (one of two handles of
cuba_hip_optimize_batch beside a plain 40-pose graph) -- on the fp64 and the fp32 library, held to the reference's loops
(tests/lm_decision_reference.py) and to the oracle.

How the runs ended on the MI355X (chain / profile / batch alike unless noted; every run with late_decision_records == 0):

  case                      fp64                                              fp32
  zero scene, niter 1, 5    1 iteration, 1 trial: rho == 0, rejected, halt    the same
                            (F0 = 0 exactly, lambda0 = 57.816, the increment exactly zero, chi2 = [0.0], estimate = start)
  every solve fails, 1, 3   1 iteration, 10 trials (rho = -1 each): the       the same
                            tenth rejection in a row; chi2 = [F0], estimate = start
  converged start, niter 5  3 iterations, trials 3 + 7 + 10: the tenth        3 iterations, trials 1 + 4 + 10: the tenth
                            rejection (last rho -1.8e-9); the profiled run    rejection (last rho -0.98); the profiled run: 3
                            the same 3 iterations and 20 trials               iterations, 15 trials, chi2 differing in the 7th digit
  Tukey rough start, 12     12 iterations (niter), trials 1 x 9, 2, 1, 1      12 iterations (niter), trials 1 x 5, 3, 1, 3, 2, 2, 1, 4
  Huber, 10 iterations      10 iterations (niter), one trial each             the same
  second run after a halt   4 iterations, 4 trials, bit-equal to a fresh      the same
                            handle's run (after the rho == 0 halt and after ten failed solves)
  niter = 0                 no iteration, no trial, estimate untouched        the same

The converged start's last iteration accepts nothing: the estimate it leaves is bit-equal to that of a fresh handle run for two iterations
(a shorter run IS a bit-exact prefix under all three drivers).  Nothing here needed a fix in the library: a zero right-hand side gives a
zero increment and an unchanged pose, the void trial behind a halt is not counted, a halt does not outlive its run."""
import copy
import functools

import numpy as np
import pytest
from conftest import RK_HUBER, RK_TUKEY

import lm_decision_reference as ref
from lm_decision_reference import reference_run

from cuba_amd.capi import HipSolver, optimize_batch
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba

pytestmark = pytest.mark.gpu

SETTINGS = ("chain", "profile", "batch")
FAILING = dict(pcg_max_iter=1, direct_fallback=0)


@pytest.fixture(params=["f64", "f32"])
def precision(request):
    return request.param


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "zero":
        return flatten(ref.zero_residual_graph())
    if name == "g40":
        return flatten(synth_ba(40, 600, 2400, seed=1))
    if name == "clean":                 # (tests/test_gpu_batch.py)
        return flatten(synth_ba(40, 600, 2400, seed=1, outlier_frac=0.0, perturb=False))
    if name == "tukey60":               # (tests/golden/make_golden_trial_chain.py: rough_start)
        g = copy.deepcopy(synth_ba(60, 1500, 6000, seed=3))
        rng = np.random.default_rng(1)
        g.lm_X = g.lm_X + rng.normal(0, 3.0, g.lm_X.shape)
        free = ~g.pose_fixed
        g.pose_t = g.pose_t.copy(); g.pose_t[free] += rng.normal(0, 0.6, (int(free.sum()), 3))
        return flatten(g)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def converged_start():
    from oracle.oracle import OracleSolver
    o = OracleSolver(graph("clean"), RK_HUBER)
    o.optimize(60)
    return o.state()


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def run(setting, precision, gname, rk, niter, start=None, first=None, **opts):
    """one run of a fresh handle; `first`: (niter, start) of a run on the same handle before it.  What the run left: chi2 series, estimates,
    LM trials, the ring of decision records (device-decided runs), F0 and lambda0 as the stage calls of a second handle give them"""
    if setting == "profile":
        opts = dict(opts, profile=1)
    h = HipSolver(graph(gname), rk, precision=precision, **opts)
    other = HipSolver(graph("g40"), RK_HUBER, precision=precision) if setting == "batch" else None

    def go(n):
        if setting == "batch":
            return optimize_batch([other, h], n)[0][1]
        return h.optimize(n)["chi2"]
    if first is not None:
        if first[1] is not None:
            h.set_state(*first[1])
        go(first[0])
    if start is not None:
        h.set_state(*start)
    begin = h.state()
    trials0 = h.counters()["lm_trials"]
    chi2 = go(niter)
    out = dict(chi2=np.array(chi2), state=h.state(), begin=begin, trials=h.counters()["lm_trials"] - trials0,
               records=h.lm_records() if setting != "profile" else None)
    assert h.counter("late_decision_records") == 0
    h.close()
    if other is not None:
        assert other.counter("late_decision_records") == 0
        other.close()
    return out


def start_numbers(precision, gname, rk, start=None, **opts):
    """F0 and lambda0 = 1e-5 * max diagonal through the stage calls"""
    h = HipSolver(graph(gname), rk, precision=precision, **opts)
    if start is not None:
        h.set_state(*start)
    F0 = h.compute_errors()
    h.build_system()
    lam0 = 1e-5 * h.max_diagonal()
    h.close()
    return F0, lam0


def replay(label, r, F0, lam0, niter):
    """the run's ring records through reference_run, each record's own Fhat and denominator as the script: every record's rho, next damping,
    next F, accepted flag and halt bit for bit, the returned chi2 series and the trial counter exactly.  Returns how the run ended."""
    T = r["trials"]
    assert 0 < T <= 64, (label, T)
    rec = r["records"][:T]
    assert np.array_equal(rec[:, 7] - rec[0, 7], np.arange(T)) and (rec[0, 7] - 1) % 65536 == 0 and rec[0, 7] > 65536, (label, rec[:, 7])
    script = [(0 if (x[2] == -1.0 and x[1] == 1e-3 and x[0] == 0.0) else 1, float(x[0]), float(x[1])) for x in rec]
    want = reference_run(F0, lam0, niter, script + [(0, 0.0, 1e-3)] * 12)
    assert want["used"] == T, (label, want["used"], T, want["counts"])
    for k, (x, w) in enumerate(zip(rec, want["records"])):
        halt = 1.0 if (k == T - 1 and want["ended"] != "niter") else 0.0
        assert (x[2] == w["rho"] or (x[2] != x[2] and w["rho"] != w["rho"])) and x[3] == w["lam"] and x[4] == w["F"] \
            and (x[5] == 1.0) == w["accepted"] and x[6] == halt, (label, k, x.tolist(), w, halt)
    assert r["chi2"].tolist() == want["chi2"], (label, r["chi2"], want["chi2"])
    print(f"\n[lm ending] {label}: {len(want['chi2'])} iterations, trials per iteration {want['counts']}, ends on {want['ended']}, "
          f"last rho {want['records'][-1]['rho']:.3e}")
    return want


# ---- exact-zero residuals ------------------------------------------------------------------------------------------------------------
def test_zero_scene_intermediate_results(precision):
    """what the zero-scene test relies on: F0 exactly 0, and a zero right-hand side gives a zero increment"""
    fp = graph("zero")
    h = HipSolver(fp, RK_HUBER, precision=precision)
    assert h.compute_errors() == 0.0
    h.close()
    h = HipSolver(fp, RK_HUBER, precision=precision)
    h.compute_errors()
    h.build_system()
    lam = 1e-5 * h.max_diagonal()
    assert lam > 0 and np.isfinite(lam)
    assert not np.any(h.array("bp")) and not np.any(h.array("lm_sys").reshape(-1, 9)[:, 6:])       # (bp; bl behind each landmark's Hll)
    h.set_lambda(lam)
    ok = h.solve()
    xp, xl = h.array("xp"), h.array("xl")
    print(f"\n[lm ending] zero scene {precision}: lambda0 {lam:.6e}, solve ok {ok}, |xp| {np.abs(xp).max()}, |xl| {np.abs(xl).max()}")
    assert ok and not np.any(xp) and not np.any(xl), (ok, xp, xl)
    h.update()
    assert same(h.state(), (fp.q, fp.t, fp.Xw))
    h.close()


@pytest.mark.parametrize("niter", [1, 5])
@pytest.mark.parametrize("setting", SETTINGS)
def test_zero_scene_ends_after_one_trial(setting, niter, precision):
    """every residual exactly 0: the oracle's run -- one iteration, chi2 = [0.0], one trial (rho == 0: rejected, the run ends), the estimate
    bit-equal to the start"""
    fp = graph("zero")
    r = run(setting, precision, "zero", RK_HUBER, niter)
    assert r["chi2"].tolist() == [0.0] and r["trials"] == 1, (r["chi2"], r["trials"])
    assert same(r["state"], (fp.q, fp.t, fp.Xw))
    if r["records"] is not None:
        x = r["records"][0]
        assert x[0] == 0.0 and x[1] == 1e-3 and x[2] == 0.0 and x[4] == 0.0 and x[5] == 0.0 and x[6] == 1.0, x
        F0, lam0 = start_numbers(precision, "zero", RK_HUBER)
        assert F0 == 0.0 and x[3] == 2 * lam0
    print(f"\n[lm ending] zero scene {setting} {precision} niter {niter}: 1 iteration, 1 trial, rho == 0 -> halt")


# ---- every solve fails ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [1, 3])
@pytest.mark.parametrize("setting", SETTINGS)
def test_every_solve_fails(setting, niter, precision):
    """pcg_max_iter = 1 without the exact fallback on the 40-pose graph: one iteration, ten trials, chi2 = [F0], nothing moved"""
    F0, lam0 = start_numbers(precision, "g40", RK_HUBER, **FAILING)
    r = run(setting, precision, "g40", RK_HUBER, niter, **FAILING)
    assert r["chi2"].tolist() == [F0] and r["trials"] == 10, (r["chi2"], F0, r["trials"])
    assert same(r["state"], r["begin"])
    if r["records"] is not None:
        want = replay(f"every solve fails {setting} {precision} niter {niter}", r, F0, lam0, niter)
        assert want["ended"] == "maxq" and want["counts"] == [10] and np.all(r["records"][:10, 2] == -1.0)


# ---- converged start, rough start, plain run: the records replayed ---------------------------------------------------------------------
CASES = dict(converged=("clean", RK_HUBER, 5), tukey_rough=("tukey60", RK_TUKEY, 12), huber10=("g40", RK_HUBER, 10))


@pytest.mark.parametrize("setting", ["chain", "batch"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_recorded_decisions_replay_through_the_reference(case, setting, precision):
    """however the run ends: its own records, replayed through the reference's loops, give its decisions, its chi2 series and its trial
    count.  And the estimate a run leaves whose last iteration accepted nothing is the estimate of the run one iteration shorter"""
    gname, rk, niter = CASES[case]
    start = converged_start() if case == "converged" else None
    F0, lam0 = start_numbers(precision, gname, rk, start)
    r = run(setting, precision, gname, rk, niter, start)
    want = replay(f"{case} {setting} {precision}", r, F0, lam0, niter)
    if case == "tukey_rough":
        assert max(want["counts"]) > 1                      # rejections inside the run
    last = [x for x in want["records"] if x["iteration"] == len(want["chi2"]) - 1]
    if not any(x["accepted"] for x in last):
        n = len(want["chi2"]) - 1
        shorter = run(setting, precision, gname, rk, n, start)
        print(f"   the last iteration accepted nothing: the estimate against a run of {n} iterations")
        assert same(r["state"], shorter["state"]) and r["chi2"][:n].tolist() == shorter["chi2"].tolist()


@pytest.mark.parametrize("setting", SETTINGS)
def test_converged_start_leaves_a_consistent_estimate(setting, precision):
    """the converged start under every driver: the chi2 series never increases, and an iteration that left the objective where it was left
    the estimate where it was (a rejected trial is undone)"""
    start = converged_start()
    r = run(setting, precision, "clean", RK_HUBER, 5, start)
    F0, _ = start_numbers(precision, "clean", RK_HUBER, start)
    series = [F0] + r["chi2"].tolist()
    assert all(b <= a for a, b in zip(series, series[1:])), series
    n = len(r["chi2"])
    print(f"\n[lm ending] converged start {setting} {precision}: {n} iterations, {r['trials']} trials, chi2 {series}")
    if series[-1] == series[-2]:
        shorter = run(setting, precision, "clean", RK_HUBER, n - 1, start)
        assert same(r["state"], shorter["state"] if n > 1 else r["begin"])


# ---- a second run on a handle whose first run halted ---------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS)
def test_second_run_after_a_halt(setting, precision):
    """the zero scene halts on its first trial (rho == 0); the same handle then starts from a rough estimate: the run of a fresh handle, bit
    for bit -- the halt does not outlive its run"""
    fp = graph("zero")
    rng = np.random.default_rng(4)
    t = fp.t.copy(); t[:fp.Pf] += rng.normal(0, 0.05, (fp.Pf, 3))
    rough = (fp.q, t, fp.Xw + rng.normal(0, 0.1, fp.Xw.shape))
    fresh = run(setting, precision, "zero", RK_HUBER, 4, rough)
    again = run(setting, precision, "zero", RK_HUBER, 4, rough, first=(5, None))
    print(f"\n[lm ending] second run {setting} {precision}: chi2 {again['chi2'].tolist()}, {again['trials']} trials")
    assert len(fresh["chi2"]) > 1 and fresh["chi2"][-1] < fresh["chi2"][0] and fresh["trials"] >= len(fresh["chi2"])
    assert again["chi2"].tolist() == fresh["chi2"].tolist() and again["trials"] == fresh["trials"] and same(again["state"], fresh["state"])
    # and after ten failed solves in a row
    f2 = run(setting, precision, "g40", RK_HUBER, 1, **FAILING)
    a2 = run(setting, precision, "g40", RK_HUBER, 1, first=(2, None), **FAILING)
    assert a2["chi2"].tolist() == f2["chi2"].tolist() and a2["trials"] == f2["trials"] == 10 and same(a2["state"], f2["state"])


# ---- niter = 0 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTINGS)
def test_no_iterations(setting, precision):
    r = run(setting, precision, "g40", RK_HUBER, 0)
    assert len(r["chi2"]) == 0 and r["trials"] == 0 and same(r["state"], r["begin"])

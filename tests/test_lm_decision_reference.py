"""The decision reference itself (tests/lm_decision_reference.py), on the CPU: its scripts tell it apart from subtly wrong loops, the
Python multi-GPU driver (dist.partitioned_optimize) follows it when driven by a scripted backend, and the oracle's optimize() counts the
trials of an iteration as it does."""
import math

import numpy as np
import pytest
from conftest import RK_HUBER, RK_TUKEY

import lm_decision_reference as ref
from lm_decision_reference import SCRIPTS, reference_run

MUTANTS = ("accept_ge", "loop_le", "clamp_to_one", "nu_not_reset", "nu_times_3", "stop_on_nan", "no_zero_stop", "maxq_9", "maxq_11")


def mutant_run(kind, F0, lam0, niter, trials):
    """reference_run with ONE thing wrong.  Returns what a caller can observe of a run: chi2 series, final damping, trials used."""
    maxq = {"maxq_9": 9, "maxq_11": 11}.get(kind, 10)
    nu, lam, F = 2.0, lam0, F0
    chi2, used = [], 0
    for _ in range(niter):
        q, rho = 0, -1.0
        while q < maxq and (rho <= 0 if kind == "loop_le" else rho < 0):
            if used >= len(trials):
                return dict(chi2=chi2, lam=lam, used="exhausted")
            ok, Fhat, sumLm, sumPose = trials[used]
            used += 1
            scale = ((sumLm + sumPose) if ok else 0.0) + 1e-3
            rho = (F - Fhat) / scale if ok else -1.0
            if (rho >= 0 if kind == "accept_ge" else rho > 0):
                t = 2 * rho - 1
                a = 1 - t * t * t
                lam *= max(1. / 3, min(a, 1.0 if kind == "clamp_to_one" else 2. / 3))
                if kind != "nu_not_reset":
                    nu = 2.0
                F = Fhat
                break
            lam *= nu
            nu *= 3 if kind == "nu_times_3" else 2
            q += 1
        chi2.append(F)
        stop = q == maxq or not math.isfinite(lam)
        if kind != "no_zero_stop":
            stop = stop or rho <= 0
        if kind == "stop_on_nan":
            stop = stop or rho != rho
        if stop:
            break
    return dict(chi2=chi2, lam=lam, used=used)


def _same(a, b):
    return a["used"] == b["used"] and len(a["chi2"]) == len(b["chi2"]) and all(x == y for x, y in zip(a["chi2"], b["chi2"])) \
        and (a["lam"] == b["lam"] or (a["lam"] != a["lam"] and b["lam"] != b["lam"]))


def test_the_scripts_end_as_intended():
    """what each script is for really happens in it (so that a test which runs `every script' runs every ending)"""
    r = {k: reference_run(*v) for k, v in SCRIPTS.items()}
    want = dict(accepted_only=(4, 4, "niter"), clamp_edges=(5, 5, "niter"), reject_then_accept=(6, 3, "niter"), nine_then_accept=(11, 2, "niter"),
                ten_rejections=(10, 1, "maxq"), six_accept_six_accept=(15, 3, "niter"), zero_after_accept=(2, 2, "rho<=0"),
                zero_first_trial=(1, 1, "rho<=0"), nan_fhat=(5, 4, "niter"), failed_mixed=(8, 3, "niter"), all_failed=(10, 1, "maxq"),
                infinite_damping=(10, 1, "maxq"), niter0=(0, 0, "niter"), niter1_rejections=(4, 1, "niter"), longer_than_the_ring=(90, 30, "niter"),
                beyond_float_range=(7, 3, "niter"))
    assert set(want) == set(SCRIPTS)
    for k, (used, iters, ended) in want.items():
        assert (r[k]["used"], len(r[k]["chi2"]), r[k]["ended"]) == (used, iters, ended), (k, r[k]["used"], len(r[k]["chi2"]), r[k]["ended"])
        assert len(r[k]["records"]) == used and sum(r[k]["counts"]) == used
    # the attenuation on both sides of either clamp bound, and below zero
    lams = [3.0] + [x["lam"] for x in r["clamp_edges"]["records"]]
    fac = [b / a for a, b in zip(lams, lams[1:])]
    assert fac[0] == pytest.approx(2 / 3, rel=1e-15) and 1 / 3 < fac[1] < 2 / 3 and 1 / 3 < fac[2] < 2 / 3 and fac[2] < 0.37 and fac[1] > 0.65
    assert fac[3] == pytest.approx(1 / 3, rel=1e-15) and fac[4] == pytest.approx(1 / 3, rel=1e-15) and r["clamp_edges"]["records"][4]["rho"] > 1
    # rho is EXACTLY zero in the two zero scripts, NaN ends an iteration with nu still doubling, the damping overflows at the 7th rejection
    assert r["zero_first_trial"]["records"][0]["rho"] == 0.0 and r["zero_after_accept"]["records"][1]["rho"] == 0.0
    assert r["zero_first_trial"]["chi2"] == [0.0]
    n = r["nan_fhat"]["records"]
    assert n[0]["rho"] != n[0]["rho"] and [x["nu"] for x in n[:3]] == [4.0, 8.0, 16.0] and [x["iteration"] for x in n] == [0, 1, 1, 2, 3]
    inf = [x["lam"] for x in r["infinite_damping"]["records"]]
    assert math.isfinite(inf[5]) and all(math.isinf(v) for v in inf[6:]) and r["infinite_damping"]["chi2"] == [2000.0]
    assert r["six_accept_six_accept"]["counts"] == [7, 7, 1] and r["nine_then_accept"]["counts"] == [10, 1]
    b = r["beyond_float_range"]["records"]
    assert max(x["lam"] for x in b) > 3.5e38 and all(math.isfinite(x["lam"]) for x in b)
    assert r["niter0"]["chi2"] == [] and r["niter0"]["lam"] == 1.0 and r["all_failed"]["chi2"] == [3000.0]


@pytest.mark.parametrize("kind", MUTANTS)
def test_every_mutant_is_caught(kind):
    caught = [k for k, v in SCRIPTS.items() if not _same(mutant_run(kind, *v), reference_run(*v))]
    print(f"\n[lm mutant] {kind}: caught by {caught}")
    assert caught, kind
    if kind in ("accept_ge", "loop_le", "no_zero_stop"):
        assert set(caught) <= {"zero_after_accept", "zero_first_trial"}, caught       # (why the two rho == 0 scripts exist)


def test_the_unmutated_copy_is_the_reference():
    for k, v in SCRIPTS.items():
        assert _same(mutant_run("none", *v), reference_run(*v)), k


# ---- dist.partitioned_optimize over a scripted backend ---------------------------------------------------------------------------------
class _Comm:
    def sum(self, v): return v
    def max(self, v): return v
    def min(self, v): return v


class _ScriptedBackend:
    """the estimate is one number, its objective: push / pop save and restore it, a trial whose solve succeeded moves it to the script's Fhat"""
    def __init__(self, F0, lam0, trials):
        self.F, self.bak, self.lam0, self.trials, self.k, self.log, self.lams = F0, None, lam0, trials, 0, [], []

    def compute_errors(self): return self.F
    def assemble(self): pass
    def allreduce_system(self, comm): pass
    def max_diagonal_parts(self): return self.lam0, 0.0
    def push(self): self.bak = self.F; self.log.append("trial")
    def set_lambda(self, lam): self.lams.append(lam)
    def schur(self): pass

    def solve_reduced(self):
        self.cur = self.trials[self.k]; self.k += 1
        return bool(self.cur[0])

    def bcast_increments(self, comm): pass
    def back_substitute(self): pass
    def update(self): self.F = self.cur[1]
    def compute_scale_parts(self, lam): return self.cur[3], self.cur[2]
    def pop(self): self.F = self.bak; self.log.append("pop")


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_partitioned_optimize_follows_the_reference(name):
    """The Python driver of the landmark-partitioned run, fed the script through a fake backend: the chi2 series EQUAL, one pop per rejected
    trial and none after an accepted one, every damping it sets (and so the damping each trial ran with) within 4 ulp of the reference's --
    the driver writes the cube as ** 3, which may round differently from t * t * t.  The damping after the last trial never leaves the
    driver; the damping before every trial does."""
    from cuba_amd import dist
    F0, lam0, niter, trials = SCRIPTS[name]
    want = reference_run(F0, lam0, niter, trials)
    b = _ScriptedBackend(F0, lam0, trials)
    chi2 = dist.partitioned_optimize(b, _Comm(), niter, tau=1.0)
    assert len(chi2) == len(want["chi2"]) and all(a == w for a, w in zip(chi2.tolist(), want["chi2"])), (chi2, want["chi2"])
    assert b.k == want["used"] == len(b.lams)
    log = []
    for r in want["records"]:
        log += ["trial"] if r["accepted"] else ["trial", "pop"]
    assert b.log == log
    before = [lam0] + [r["lam"] for r in want["records"][:-1]] if want["used"] else []
    for got, w in zip(b.lams, before):
        assert got == w or abs(got - w) <= 4 * math.ulp(w), (name, got, w)
    assert b.F == want["F"] or name == "niter0"


# ---- the oracle's trial count --------------------------------------------------------------------------------------------------------
def _oracle_script(fp, rk, niter):
    """the run of optimize(niter) made of the oracle's own stage calls, its trials as a script (sumPose = 0: the oracle adds the two parts)"""
    from oracle.oracle import OracleSolver
    o = OracleSolver(fp, rk)
    o.build_structure()
    script, lam, nu, F0, lam0 = [], 0.0, 2.0, None, None
    for it in range(niter):
        F = o.compute_errors()
        o.build_system()
        if it == 0:
            F0, lam0 = F, 1e-5 * o.max_diagonal()
            lam = lam0
        q, rho = 0, -1.0
        while q < 10 and rho < 0:
            o.push(); o.set_lambda(lam)
            ok = o.solve()
            o.update()
            Fhat = o.compute_errors()
            scale = o.compute_scale(lam)
            script.append((1 if ok else 0, Fhat, scale, 0.0))
            lam = reference_run(F0, lam0, niter, script + [(0, 0.0, 0.0, 0.0)] * 12)["records"][len(script) - 1]["lam"]
            rho = (F - Fhat) / (scale + 1e-3) if ok else -1.0
            if rho > 0:
                break
            o.restore_diagonal(); o.pop()
            q += 1
        if q == 10 or rho <= 0 or not math.isfinite(lam):
            break
    return F0, lam0, script


def _rough(P, L, E):
    """the rough start of tests/golden/make_golden_trial_chain.py on a smaller graph"""
    import copy
    from cuba_amd.graph import flatten
    from cuba_amd.synth import synth_ba
    g = copy.deepcopy(synth_ba(P, L, E, seed=3))
    rng = np.random.default_rng(1)
    g.lm_X = g.lm_X + rng.normal(0, 3.0, g.lm_X.shape)
    free = ~g.pose_fixed
    g.pose_t = g.pose_t.copy(); g.pose_t[free] += rng.normal(0, 0.6, (int(free.sum()), 3))
    return flatten(g)


def test_oracle_counts_one_trial_on_the_zero_scene():
    """every residual exactly 0: F0 = 0, the first trial's rho is exactly 0 -- rejected, and the run ends.  ONE trial ran"""
    from cuba_amd.graph import flatten
    from oracle.oracle import OracleSolver
    fp = flatten(ref.zero_residual_graph())
    assert (fp.Pt, fp.Pf, fp.Lt, fp.E) == (6, 5, 24, 72) and 0 < fp.E2 < fp.E
    o = OracleSolver(fp, RK_HUBER)
    assert o.compute_errors() == 0.0
    for niter in (1, 5):
        o = OracleSolver(fp, RK_HUBER)
        r = o.optimize(niter)
        want = reference_run(0.0, 1.0, niter, [(1, 0.0, 0.0, 0.0)] * 3)
        assert r["chi2"].tolist() == [0.0] == want["chi2"] and r["trials"].tolist() == [1] == want["counts"], (r, want)
        q, t, X = o.state()
        assert np.array_equal(q, fp.q) and np.array_equal(t, fp.t) and np.array_equal(X, fp.Xw)


@pytest.mark.parametrize("shape", [(30, 400, 1600), (60, 1500, 6000), (20, 200, 800)])
def test_oracle_counts_the_trials_of_a_rejecting_start(shape):
    """Tukey rough starts: the 30- and the 60-pose run reject a trial in the middle (two trials in that iteration: the rejected one AND the
    accepted one), the 20-pose run ends early.  Per iteration, the oracle's optimize() reports the count -- and the chi2 -- of the reference
    loop run over the oracle's own stage results"""
    from oracle.oracle import OracleSolver
    fp = _rough(*shape)
    F0, lam0, script = _oracle_script(fp, RK_TUKEY, 12)
    want = reference_run(F0, lam0, 12, script)
    assert want["used"] == len(script)
    r = OracleSolver(fp, RK_TUKEY).optimize(12)
    print(f"\n[oracle trials] {shape}: trials per iteration {want['counts']}, run ended on {want['ended']}")
    # (chi2 to 1e-9, not to the bit: the stage run above takes its dampings from t * t * t, optimize() from std::pow)
    assert r["trials"].tolist() == want["counts"] and np.allclose(r["chi2"], want["chi2"], rtol=1e-9, atol=0), (r, want["counts"], want["chi2"])
    assert abs(r["lambdas"][-1] - want["lam"]) <= 4 * math.ulp(want["lam"])            # (the oracle writes the cube as std::pow)
    if shape[0] != 20:
        assert max(want["counts"]) > 1, want["counts"]            # the start really rejects
    else:
        assert len(want["counts"]) < 12, want["counts"]           # the run really ends early


# ---- the hook's argument checks (no device needed: every one of them returns before the device is touched) ---------------------------
def test_the_decision_hook_refuses_bad_arguments():
    from cuba_amd import capi
    lib = capi.load_library("f64")
    start, out = np.zeros(10), np.zeros(32 * 4)
    ok = np.ones(2, dtype=np.int32)
    good, a = np.array([0, 1, 2], dtype=np.int32), np.ones(4)

    def call(niter=1, n=2, ok=ok, a=a, a_off=good, b_off=good, c_off=good, scratch=1, start=start, out=out, mode=0, tag=0.0):
        return lib.cuba_hip_debug_lm_script(0, mode, 1.0, 1.0, None, None, 1e-5, tag, niter, n, capi._i(ok), capi._d(a), capi._i(a_off), capi._d(a), capi._i(b_off),
                                            capi._d(a), capi._i(c_off), scratch, capi._d(start), capi._d(out))
    bad = [dict(n=-1), dict(n=513), dict(niter=-1), dict(niter=513), dict(ok=None), dict(a_off=None), dict(start=None), dict(out=None),
           dict(a=None), dict(a_off=np.array([1, 1, 2], dtype=np.int32)), dict(b_off=np.array([0, 2, 1], dtype=np.int32)),
           dict(c_off=np.array([0, 1, 70000], dtype=np.int32)), dict(scratch=2 ** 20 + 1), dict(mode=1), dict(mode=2), dict(tag=-1.0),
           dict(tag=float("nan"))]
    for kw in bad:
        assert call(**kw) == 1, kw                     # CUBA_HIP_ERR_INVALID_ARGUMENT

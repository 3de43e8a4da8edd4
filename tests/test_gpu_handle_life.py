"""A reused solver handle against a fresh one, through every state change: one test per script (tests/handle_life_scripts.py) and setting.

The live handle makes every call of the script.  At every Check a TWIN is built from the model's Spec alone (tests/handle_life_model.py):
a fresh handle with the options and robust kernels given at construction, one one-call set_graph, the factor sets, set_edge_active(mask),
the partition, and set_state with the model's estimates -- never anything read from the live handle.  The same sequence then runs on both:

  before the run   state(), compute_errors(), max_diagonal(), set_lambda(1e-5 max diagonal) + schur() -> hsc_structure(), hsc(), bsc, bp
                   (a stale structure or stale values show here, before any solve), the covariance blocks and pairs where the script asks
  optimize(k)      chi2 per iteration, state(), the LM trials and the PCG history the run added, chi_squares(), every factor kind's
                   chi squares, edge_active(), and no late decision records on either

Settings:
  f64      fp64 library, heuristics = 0 on both handles: everything above bit for bit (np.array_equal), and the twin's chi2 per iteration
           within CHI2_TOL = 1e-6 of the fp64 reference of the Spec (the project's bar: DESIGN section 5, tests/test_gpu_configs.py header)
  f32      fp32 library, heuristics = 0: bit for bit against the twin only
  default  fp64 library with the options users run (heuristics = 1).  A reused handle legitimately differs from a fresh one in bits here
           (it starts with the previous run's coarse inverse and iteration counts), so no twin: chi2 per iteration within 1e-6 of the
           reference, as many iterations as the reference, and no unconverged PCG solve, failed exact solve or late decision record.

A landmark-partitioned handle evaluates its own landmarks only: its Check compares the stage outputs with a twin in the same partition
(state, compute_errors, assemble + max_diagonal_parts, schur -> hsc, bsc, bp, chi_squares) and runs nothing.

The batch test sends three handles that have lived through the first half of windows, factors_all and gate into cuba_hip_optimize_batch,
lets them go on alone, and sends them into a second batch in another order; each is compared with a twin that runs alone.

What the scripts found on the MI355X (script, check, first quantity that differed from the twin), all fixed in csrc/:
  windows_refusals  check 1  compute_errors 239317.7 against 259999.9: a promise was not consumed by a call refused for its counts or its
                             landmark range, and the next upload of other edges with the same counts ran on the previous edges.  The
                             promise is now consumed at the top of setGraph.
  reorder_options   check 1  hsc in the last bits (33857 of 100836 entries): "landmark_reorder" did not take effect with an upload of the
                             same index arrays; check 5: neither did "pose_reorder" = 0 (the kept order stayed).  The kept sort is now
                             reused only while the landmark order in force is the one a fresh upload would choose, the kept pose order
                             only while "pose_reorder" is on.
  factors_all       check 4  compute_errors 76241.65 against 76244.01: a set_graph refused for a bad edge index had already dropped all
                             seven factor sets.  Settled in the header (a refused upload consumes a pending promise and nothing else);
                             the factors are now cleared after the validation.
  orders            check 4  compute_errors 5.1e13 against 3.1e6: "device_setup" = 0 on a handle whose graph had been sorted on the
                             device, a run, then an upload of the same index arrays: the host pipeline reused a host topology read back
                             in the internal landmark order for landmark rows it uploads in the caller's.  It now sorts afresh.
  partition         check 5  hsc in the last bits (4196 of 11700): a whole upload after a ranged one (or under a set partition) was
                             sorted while the old range was still in force and lost the internal landmark order.  The range is now
                             lifted before the sort.
  windows_refusals  check 5  compute_errors 239926.68 against 240058.67 (read from the code, then shown by the twin): a _begin alone, then
                             an upload refused for its counts, then a run.  The refused call had already closed the open two-step
                             upload -- values no longer pending, never gathered -- so the begun graph ran on the sorted values of the
                             upload before it.  The bookkeeping of an open upload now sits below every refusal of setGraph.
  factors_all                (the test's own plumbing) HipSolver.set_graph recorded a REFUSED problem as the one in force, so the next
                             chi_squares() handed the library a buffer one edge short.  It records the problem after a successful call.
  Not a defect, now written into the header: "device_setup" changed on a handle that holds a graph switches the analysis at once and the
  edge sort with the next upload; until then sums differ from a fresh handle's in the last bit (orders: compute_errors 3134224.218354888
  against ...8883), so the scripts compare after that upload.

Mutants of the host code (one line each, built on a scratch copy, never committed, run once in the f64 setting; restricted to ones that
change which values or which cached result is reused at unchanged sizes), and the script and quantity that caught each:
  clearFactors() skipped when the counts are unchanged      factors_all, check 3 (the identical upload under a promise): compute_errors
  keepValues true whenever edges are promised               windows, check 9 (promised edges, new values): compute_errors
  clearGate() skipped when the counts are unchanged         gate, check 5 (other edges): compute_errors
  "direct_slack" not resetting directPlanValid              options_solver_150, check 7 (an exact solve under another slack): chi2 per iteration
  dropSnapshots() skipped in setGraph                       orders: the restore after the upload was accepted (status 3 expected)
  set_robust_kernel not reaching a live handle              ten tests, each at its first check with kernels set: compute_errors
  no startRunHistory() / coarseValid = false in setGraph    SURVIVES, and no script step can catch it through cuba_hip_optimize: every run
                                                            resets both itself at its start (ba_lm.hip, both loops).  The line matters to
                                                            hand-driven stage solves alone, and there a kept coarse inverse is a valid
                                                            preconditioner: a stage solve on a reused handle differs from a fresh one's
                                                            at the PCG tolerance with or without the mutant (tried: xp after
                                                            solve_reduced differed in 27 of 58 tests on the unmutated library), so it
                                                            is not among the compared quantities.
"""
import numpy as np
import pytest

import handle_life_model as m
import handle_life_scripts as sc
from handle_life_model import CHI2_GETTER, KINDS, Batch, Spec

from cuba_amd.capi import HipSolver, optimize_batch

pytestmark = pytest.mark.gpu

CHI2_TOL = 1e-6
SETTINGS = {"f64": dict(precision="f64", heuristics=0), "f32": dict(precision="f32", heuristics=0), "default": dict(precision="f64")}


def new_spec(setting):
    opts = dict(SETTINGS[setting])
    return Spec(precision=opts.pop("precision"), options=opts)


def new_handle(spec):
    return HipSolver(None, spec.rk, precision=spec.precision, **{k: v for k, v in spec.options.items() if v is not None})


def make_twin(spec):
    """a fresh handle in the Spec's state, from the Spec alone"""
    h = new_handle(spec)
    fp = spec.problem()
    h.set_graph(fp, landmark_range=spec.partition if spec.ranged else None)
    for kind in KINDS:
        if kind in spec.factors:
            getattr(h, "set_" + kind)(*spec.factors[kind])
    for factor_type, (kind, delta) in spec.kernels.items():
        h.set_pose_factor_robust_kernels(factor_type, kind, delta)
    if spec.mask is not None:
        h.set_edge_active(spec.mask)
    if spec.partition is not None and not spec.ranged:
        h.set_partition(*spec.partition)
    h.set_state(*spec.est)
    return h


def same(label, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: %s against the twin's %s" % (label, a.shape, b.shape)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a.ravel() != b.ravel())
        raise AssertionError("%s differs from the twin's in %d of %d entries, first at %d: %r against %r"
                             % (label, len(bad), a.size, bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]]))


def solve_counts(h):
    return {k: h.counter(k) for k in ("pcg_unconverged_solves", "exact_solve_failures", "late_decision_records")}


def before_the_run(spec, live, twin, where):
    for k, (a, b) in enumerate(zip(live.state(), twin.state())):
        same(where + " state[%d]" % k, a, b)
    same(where + " compute_errors", live.compute_errors(), twin.compute_errors())
    if spec.partition is not None:
        for h in (live, twin):
            h.build_system(); h.assemble()
        parts = live.max_diagonal_parts()
        same(where + " max_diagonal_parts", parts, twin.max_diagonal_parts())
        lam = 1e-5 * max(parts)
    else:
        for h in (live, twin):
            h.build_system()
        lam = live.max_diagonal()
        same(where + " max_diagonal", lam, twin.max_diagonal())
        lam *= 1e-5
    assert np.isfinite(lam) and lam > 0
    for h in (live, twin):
        h.set_lambda(lam); h.schur()
    for k, (a, b) in enumerate(zip(live.hsc_structure(), twin.hsc_structure())):
        same(where + " hsc_structure[%d]" % k, a, b)
    same(where + " hsc", live.array("hsc"), twin.array("hsc"))
    same(where + " bsc", live.array("bsc"), twin.array("bsc"))
    same(where + " bp", live.array("bp"), twin.array("bp"))
    for h in (live, twin):
        h.restore_diagonal()


def covariances(spec, step, live, twin, where):
    a, b = live.covariance(), twin.covariance()
    assert not a["not_positive_definite"] and not b["not_positive_definite"], where
    same(where + " covariance pose", a["pose"], b["pose"])
    same(where + " covariance landmark", a["landmark"], b["landmark"])
    same(where + " covariance_blocks", live.covariance_blocks(), twin.covariance_blocks())
    assert np.abs(a["pose"]).max() > 0
    pa, pb = live.covariance_pairs(list(step.covariance_pairs)), twin.covariance_pairs(list(step.covariance_pairs))
    assert not pa[1] and not pb[1]
    for k, (x, y) in enumerate(zip(pa[0], pb[0])):
        same(where + " covariance_pairs[%d]" % k, x, y)


def after_the_run(spec, live, twin, where):
    for k, (a, b) in enumerate(zip(live.state(), twin.state())):
        same(where + " state[%d] after the run" % k, a, b)
    same(where + " chi_squares", live.chi_squares(), twin.chi_squares())
    for kind in spec.factors:
        same(where + " " + CHI2_GETTER[kind], getattr(live, CHI2_GETTER[kind])(), getattr(twin, CHI2_GETTER[kind])())
    same(where + " edge_active", live.edge_active(), twin.edge_active())
    if spec.mask is not None:
        same(where + " edge_active against the model's mask", live.edge_active(), spec.mask)


def against_the_reference(spec, step, chi2, where):
    ref = m.reference(spec, step.niter)
    print("%s: chi2 %s, reference %s" % (where, chi2, ref))
    assert len(chi2) == len(ref), (where, chi2, ref)
    worst = np.abs(chi2 - ref) / ref
    assert worst.max() <= CHI2_TOL, (where, worst)


class Comparison:
    """on_check of run_script for one live handle"""

    def __init__(self, setting, live):
        self.setting, self.live, self.n = setting, live, 0

    def __call__(self, spec, step):
        self.n += 1
        where = "check %d" % self.n
        live, setting = self.live, self.setting
        if setting == "default":
            if spec.partition is not None:
                return
            was = solve_counts(live)
            chi2 = live.optimize(step.niter)["chi2"]
            if step.reference:
                against_the_reference(spec, step, chi2, where)
            assert solve_counts(live) == was and was["late_decision_records"] == 0, (where, was, solve_counts(live))
            return
        twin = make_twin(spec)
        try:
            before_the_run(spec, live, twin, where)
            if spec.partition is not None:
                same(where + " chi_squares", live.chi_squares(), twin.chi_squares())
                return
            if step.covariance_pairs is not None:
                covariances(spec, step, live, twin, where)
            trials = [h.counters()["lm_trials"] for h in (live, twin)]
            solves = [len(h.pcg_history()[0]) for h in (live, twin)]
            a, b = live.optimize(step.niter)["chi2"], twin.optimize(step.niter)["chi2"]
            same(where + " chi2 per iteration", a, b)
            assert len(a) and np.isfinite(a).all()
            after_the_run(spec, live, twin, where)
            # (both run from the handle's last upload: the run's own part is what it added)
            same(where + " lm_trials", live.counters()["lm_trials"] - trials[0], twin.counters()["lm_trials"] - trials[1])
            same(where + " pcg_history", live.pcg_history()[0][solves[0]:], twin.pcg_history()[0][solves[1]:])
            assert twin.counters()["lm_trials"] > trials[1]
            assert live.counter("late_decision_records") == 0 and twin.counter("late_decision_records") == 0
            if setting == "f64" and step.reference:
                against_the_reference(spec, step, b, where)
        finally:
            twin.close()


def batch_and_solo(setting, lives, specs, niter, order):
    """the handles in `order` through one cuba_hip_optimize_batch; each against its twin's solo run"""
    names = [list(lives)[i] for i in order]
    step = Batch(niter)
    for n in names:
        m.apply(step, specs[n])
    twins = {n: make_twin(specs[n]) for n in names} if setting != "default" else {}
    was = {n: solve_counts(lives[n]) for n in names}
    chi2, _ = optimize_batch([lives[n] for n in names], niter)
    for n, got in zip(names, chi2):
        where = "batch %s (%s)" % ("-".join(names), n)
        if setting == "default":
            against_the_reference(specs[n], step, got, where)
            assert solve_counts(lives[n]) == was[n] and was[n]["late_decision_records"] == 0, where
        else:
            solo = twins[n].optimize(niter)["chi2"]
            same(where + " chi2 per iteration", got, solo)
            after_the_run(specs[n], lives[n], twins[n], where)
            if setting == "f64":
                against_the_reference(specs[n], step, solo, where)
            twins[n].close()
        m.ran(specs[n], niter)


# (the fp32 library refuses the covariance calls: the scripts that make them exist for the fp64 library only)
CASES = [(name, setting) for setting in sorted(SETTINGS) for name in sorted(sc.SCRIPTS) if not (setting == "f32" and name in sc.FP64_ONLY)]


@pytest.mark.parametrize("name,setting", CASES, ids=["%s-%s" % c for c in CASES])
def test_a_reused_handle_is_a_fresh_one(name, setting):
    spec = new_spec(setting)
    live = new_handle(spec)
    try:
        check = Comparison(setting, live)
        m.run_script(sc.script(name, spec.precision), spec, live, on_check=check)
        assert check.n == sum(isinstance(s, m.Check) for s in sc.script(name, spec.precision)) >= 3
    finally:
        live.close()


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_handles_with_a_past_in_two_batches(setting):
    parts = sc.batch_lives()
    specs = {n: new_spec(setting) for n in parts}
    lives = {n: new_handle(specs[n]) for n in parts}
    try:
        for n, (first, _) in parts.items():
            m.run_script(first, specs[n], lives[n], on_check=Comparison(setting, lives[n]))
        batch_and_solo(setting, lives, specs, sc.BATCH_ITERATIONS[0], (0, 1, 2))
        for n, (_, between) in parts.items():
            m.run_script(between, specs[n], lives[n])
        batch_and_solo(setting, lives, specs, sc.BATCH_ITERATIONS[1], (2, 0, 1))
    finally:
        for h in lives.values():
            h.close()

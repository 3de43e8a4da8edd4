"""The model of the handle's state rules (tests/handle_life_model.py) and the scripts (tests/handle_life_scripts.py), without a GPU:
a literal case for every rule (the wrong variant of the rule must change the predicted Spec), the coverage of the transition table by the
scripts, and -- the condition that keeps a GPU comparison from being two empty or constant arrays -- the fp64 reference alone at every
checkpoint: it runs all the iterations asked for, its chi2 is finite and strictly decreasing over the first two."""
import dataclasses

import numpy as np
import pytest

import handle_life_model as m
import handle_life_scripts as sc
from handle_life_model import (ERR_ARGUMENT, ERR_STATE, Check, Hint, Optimize, Refused, Restore, Rules, SetFactors, SetMask, SetOption,
                               SetRobustKernel, SetState, Snapshot, Spec, Upload)


def run(steps, **wrong):
    return m.run_script(steps, Spec(rules=Rules(**wrong)))


@pytest.fixture(scope="module")
def A():
    return sc.problem("w40")


@pytest.fixture(scope="module")
def A2(A):
    return sc.other_edges(A, 1)


@pytest.fixture(scope="module")
def priors():
    return sc.factor_sets("a")["pose_priors"]


# ---- the rules, one literal case each ---------------------------------------------------------------------------------------------------
def test_every_successful_upload_clears_the_factor_sets(A, priors):
    steps = [Upload(A), SetFactors("pose_priors", priors), m.SetPoseFactorKernels(0, np.full(3, 1), np.full(3, 2.0)), Upload(A)]
    right, wrong = run(steps), run(steps, upload_clears_factors=False)
    assert right.factors == {} and right.kernels == {}
    assert set(wrong.factors) == {"pose_priors"} and right.key() != wrong.key()


def test_every_successful_upload_clears_the_snapshots(A):
    steps = [Upload(A), Snapshot(3), Upload(A)]
    right, wrong = run(steps), run(steps, upload_clears_snapshots=False)
    assert right.snapshots == {} and set(wrong.snapshots) == {3} and right.key() != wrong.key()
    with pytest.raises(AssertionError):          # the model holds no such slot: the script must expect the refusal
        m.apply(Restore(3), right)
    m.apply(Refused(Restore(3), ERR_STATE), right)


def test_the_mask_survives_the_same_edges_and_nothing_else(A, A2):
    mask = np.arange(A.E) % 7 != 0
    for label, steps in (("compared", [Upload(A), SetMask(mask), Upload(sc.other_values(A, 1))]),
                         ("promised", [Upload(A), SetMask(mask), Hint(True, False), Upload(A)])):
        right, wrong = run(steps), run(steps, mask_survives_same_edges=False)
        assert np.array_equal(right.mask, mask), label
        assert wrong.mask is None and right.key() != wrong.key(), label
    assert run([Upload(A), SetMask(mask), Upload(A2)]).mask is None                       # other edges, same counts
    assert run([Upload(A), SetMask(mask), Upload(sc.problem("w12"))]).mask is None        # other counts


def test_a_promise_covers_exactly_one_call(A, A2):
    steps = [Upload(A), Hint(True, True), Upload(A), Upload(A2)]
    right, wrong = run(steps), run(steps, promise_one_call=False)
    assert right.promise == (False, False) and np.array_equal(right.fp.eL, A2.eL)
    assert np.array_equal(wrong.fp.eL, A.eL) and right.key() != wrong.key()          # (a wrong promise is not detected: the previous edges)


def test_a_refused_upload_consumes_the_promise_and_nothing_else(A, A2, priors):
    mask = np.arange(A.E) % 5 != 0
    before = [Upload(A), SetFactors("pose_priors", priors), SetMask(mask), Snapshot(0)]
    for bad in (Upload(sc.broken(A, "counts")), Upload(A, "ranged", (5, A.Lt + 3)), Upload(sc.broken(A, "edge_index"))):
        kept = run(before)
        steps = before + [Hint(True, True), Refused(bad, ERR_ARGUMENT)]
        right = run(steps)
        assert right.promise == (False, False) and right.key() == kept.key()
        assert run(steps, refusal_consumes_promise=False).promise == (True, True)
        assert run(steps, refusal_keeps_the_rest=False).key() != kept.key()
        after, after_wrong = run(steps + [Upload(A2)]), run(steps + [Upload(A2)], refusal_consumes_promise=False)
        assert np.array_equal(after.fp.eL, A2.eL) and np.array_equal(after_wrong.fp.eL, A.eL) and after.key() != after_wrong.key()
    with pytest.raises(AssertionError):          # the model refuses the call: a script that expects it to pass is wrong
        run(before + [Upload(sc.broken(A, "counts"))])
    with pytest.raises(AssertionError):
        run(before + [Refused(Upload(A2), ERR_ARGUMENT)])


def test_a_promised_upload_is_not_looked_at(A):
    """"the library then skips its own comparison of the index arrays": a bad index under a promise of the same counts is not seen"""
    bad = sc.broken(A, "counts"); bad.Pf = A.Pf; bad.eP = A.eP.copy(); bad.eP[3] = A.Pt + 5
    got = run([Upload(A), Hint(True, False), Upload(bad)])
    assert np.array_equal(got.fp.eP, A.eP)
    with pytest.raises(AssertionError):
        run([Upload(A), Upload(bad)])


def test_a_ranged_upload_ignores_a_promise_of_values(A):
    Av = sc.other_values(A, 3)
    steps = [Upload(A), Hint(True, True), Upload(Av, "ranged", (0, A.Lt // 2))]
    right, wrong = run(steps), run(steps, ranged_ignores_values=False)
    assert np.array_equal(right.fp.meas, Av.meas) and np.array_equal(wrong.fp.meas, A.meas) and right.key() != wrong.key()
    assert right.partition == (0, A.Lt // 2) and right.ranged
    whole = run([Upload(A), Hint(True, True), Upload(Av)])          # a whole upload keeps the promised values
    assert np.array_equal(whole.fp.meas, A.meas) and np.array_equal(whole.est[2], Av.Xw)
    after = run(steps + [Hint(True, True), Upload(A)])              # ... but not after a ranged one: the device held a part of them
    assert np.array_equal(after.fp.meas, A.meas) and not after.ranged and after.partition is None


def test_a_promise_of_values_after_a_begin_only_upload_is_not_kept(A):
    Av = sc.other_values(A, 3)
    got = run([Upload(A), Upload(Av, "begin"), Hint(True, True), Upload(A)])
    assert np.array_equal(got.fp.meas, A.meas)


def test_a_restore_returns_the_saved_estimates_or_fails(A):
    moved = (A.q, A.t + 0.25, A.Xw)
    steps = [Upload(A), Snapshot(1), SetState(moved), Restore(1)]
    right, wrong = run(steps), run(steps, restore_or_state_error=False)
    assert all(np.array_equal(a, b) for a, b in zip(right.est, (A.q, A.t, A.Xw)))
    assert np.array_equal(wrong.est[1], moved[1]) and right.key() != wrong.key()
    s = run([Upload(A), Snapshot(1), Optimize(2)])
    assert s.est is None
    m.apply(Restore(1), s)
    assert np.array_equal(s.est[1], A.t)
    s = run([Upload(A), Optimize(2), Snapshot(1), SetState(moved), Restore(1)])          # a copy of estimates a run had moved
    assert s.est is None
    with pytest.raises(AssertionError):
        m.apply(Check(2), s)


def test_options_and_robust_kernels_keep_their_last_value(A, A2):
    steps = [SetOption("heuristics", 0), Upload(A), SetOption("pcg_aggregate", 6), SetRobustKernel(1, 2, 5.0), SetOption("pcg_aggregate", 4),
             Upload(A2), Optimize(1)]
    right, wrong = run(steps), run(steps, options_keep=False)
    assert right.options == dict(heuristics=0, pcg_aggregate=4) and right.rk == ((0, 0.0), (1 * 2, 5.0))
    assert wrong.options == {} and right.key() != wrong.key()


def test_the_estimates_are_the_models_own(A):
    s = run([Upload(A)])
    assert all(np.array_equal(a, b) for a, b in zip(s.est, (A.q, A.t, A.Xw)))
    for step in (Optimize(2), m.Stages()):
        t = run([Upload(A), step])
        assert t.est is None
    assert run([Upload(A), Optimize(0)]).est is not None
    t = run([Upload(A), m.Push(), m.Stages(), m.Pop()])
    assert np.array_equal(t.est[1], A.t)
    t = run([Upload(A), m.Push(), Optimize(1), m.Pop()])          # the LM loop's own push overwrote the copy
    assert t.est is None


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dry_runs():
    out = {name: m.run_script(sc.script(name), Spec(options=dict(heuristics=0))) for name in sc.SCRIPTS}
    out.update({"batch:" + name: m.run_script(sc.batch_script(name), Spec(options=dict(heuristics=0))) for name in sc.batch_lives()})
    return out


def test_every_transition_is_taken_by_a_script(dry_runs):
    taken = set()
    for spec in dry_runs.values():
        taken |= set(spec.trace)
    assert taken <= set(m.TRANSITIONS)
    missing = sorted(set(m.TRANSITIONS) - taken)
    assert not missing, missing


def test_scripts_are_of_the_stated_size(dry_runs):
    """at most about 30 small handles a test: one twin per check"""
    for name in sc.SCRIPTS:
        checks = sum(isinstance(s, Check) for s in sc.script(name))
        assert 3 <= checks <= 18, (name, checks)


@pytest.mark.parametrize("name", sorted(sc.SCRIPTS) + ["batch:" + n for n in sorted(sc.batch_lives())])
def test_the_reference_alone_at_every_checkpoint(name):
    seen = []
    steps = sc.batch_script(name[6:]) if name.startswith("batch:") else sc.script(name)

    def on_check(spec, step):
        if spec.partition is not None:
            return
        chi2 = m.reference(spec, step.niter)
        seen.append(chi2)
        assert len(chi2) == step.niter >= 2, (name, len(seen), chi2)
        assert np.isfinite(chi2).all() and chi2[1] < chi2[0] and (chi2 > 0).all(), (name, len(seen), chi2)
    spec = m.run_script(steps, Spec(options=dict(heuristics=0)), on_check=on_check)
    assert len(seen) == len(spec.checks) >= 2
    # the references are cached by the Spec's key: a second pass computes nothing
    n = len(m._references)
    m.run_script(steps, Spec(options=dict(heuristics=0)), on_check=on_check)
    assert len(m._references) == n


def test_the_reference_key_ignores_what_the_reference_does_not_see(A):
    a = run([Upload(A)])
    b = run([SetOption("pcg_aggregate", 6), Upload(A), Snapshot(2)])
    assert a.key() != b.key() and a.reference_key() == b.reference_key()
    c = run([Upload(A), SetMask(np.arange(A.E) % 9 != 0)])
    assert c.reference_key() != a.reference_key()
    assert dataclasses.replace(a, precision="f32").reference_key() == a.reference_key()

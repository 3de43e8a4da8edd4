"""Pose refinement on the device with the landmarks held (cuba_hip_refine_poses) against tests/pose_refinement_reference.py.

Exact part: statuses, counts, inliers and edge_inlier are compared exactly.  Every such comparison first asserts ON THE REFERENCE ALONE that
no decision lies within 1e-6 (relative) of its decision point: a classification's omega |r|^2 against its threshold, a depth against 0, a
trial's F - F' (relative to F) against 0, an LDL^T pivot (relative to its diagonal entry) against 0.  LM converges quadratically, so from
the third trial of a round on F - F' is rounding noise: the exact runs are short -- 3 rounds of 1 trial, 2 of 1, 1 of 2 -- and start 5
degrees and 0.5 m off (the zoo: 2 degrees and 0.2 m).  The smallest margins found on the CPU
(classification, depth, gain, pivot):
  small graph      3 x 1: 2.7e-4, 1.0, 1.4e-5, 0.10 (robust_rounds 0); 7.3e-4, 1.0, 5.4e-5, 0.098 (robust_rounds 2 and 3); 2 x 1: 5.4e-2 (gain);
                   1 x 2: 5.6e-2 (gain); Tukey 3 x 1: 4.9e-4, 1.0, 1.4e-5, 0.10; float-rounded inputs: 7.5e-4, 1.0, 5.4e-5, 0.098
  wide poses       1.5e-4, 1.0, 2.5e-2, 0.065;   zoo: 9.0e-3, 1.0, 7.2e-6, 6.2e-3 (the smallest margin of all: the zoo's gain)
Refined poses, fp64 library: pose distance (the larger of |dt|_inf / max(1, |t|_inf) and the rotation angle of dR) <= 8 D, D = the
reference's own largest distance from its 60-digit twin ON THE SAME POSES; 8 for the other summation order (lane-strided, butterfly) and
fma contraction.  fp32 library: the reference is fed the float-rounded state, cameras, measurements, information and kernel widths the
handle holds; the same bound plus one float rounding of the stored result (2^-24 per translation component, 2^-23 of rotation angle:
every quaternion component moves by at most 2^-24, the angle by twice the quaternion's change).
chi2: rtol 1e-9 (1e-6 with the fp32 library, whose stored pose the sum is not taken at) -- the sum changes by 2 b . d for a pose change d,
|b| <= 1e7 and |d| <= 8 D ~ 1e-11 on these graphs, against sums of 10 ... 1e5.

Long runs (4 x 10 trials) reach convergence, where the gain is rounding noise: statuses and final poses only, within 8 D with D from the
twin run at the same counts (the twin's own decisions already carry that noise)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_refinement_reference as R  # noqa: E402

from conftest import RK_HUBER, RK_TUKEY  # noqa: E402
from cuba_amd.capi import POSEREF_STATUS_NAMES, CubaHipError, HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 1e-6
F32_EPS = 2.0 ** -24
D_POSES = range(6)         # the poses D is measured on (and the device's poses are bounded on)


@pytest.fixture(scope="module")
def true_fp():
    """the suite's small graph at the true poses and points"""
    from cuba_amd.synth import synth_ba
    return flatten(synth_ba(40, 600, 2400, seed=1, perturb=False))


@pytest.fixture(scope="module")
def start(true_fp):
    """the small graph's state with the poses 5 degrees and 0.5 m off, the true points"""
    q, t = R.perturbed_poses(true_fp, 11, rot_deg=5.0, trans=0.5)
    return q, t, true_fp.Xw.copy()


@pytest.fixture(scope="module")
def wide_fp():
    """5 poses of 129 ... 300 edges each: the lane-strided loop runs more than twice"""
    fp = R.wide_problem()
    assert list(np.bincount(fp.eP, minlength=fp.Pt)) == [129, 150, 200, 257, 300] and fp.Pf == 5
    return fp


@pytest.fixture(scope="module")
def zoo():
    return R.zoo_problem()


_refs = {}


def reference(key, fp, state, poses, f32=False, rk=RK_HUBER, omega=None, **args):
    """(reference result, D over `poses`, the twin's steps), computed once per key; f32: on the float-rounded inputs"""
    if key not in _refs:
        if f32:
            fp, state = R.float_rounded(fp, state)
            rk = R.float_rounded_kernels(rk)
            omega = None if omega is None else np.asarray(omega, dtype=np.float32).astype(np.float64)
        ref = R.refine(fp, state=state, rk=rk, omega=omega, **args)
        D, statuses, twin = R.model_distance(ref, poses)
        assert all(ref["status"][p] == s for p, s in statuses.items())
        _refs[key] = (ref, D, twin)
    return _refs[key]


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def check_poses(got, ref, D, poses, what, f32=False):
    ok = [p for p in poses if ref["status"][p] == R.OK]
    assert len(ok) >= 1
    dist = [R.pose_distance(got["q"][p], got["t"][p], ref["q"][p], ref["t"][p]) for p in ok]
    bound = 8 * D + (2 * F32_EPS if f32 else 0.0)
    print(f"[pose refinement] {what}: largest pose distance device - reference {max(dist):.2e}, D {D:.2e}, bound {bound:.2e}")
    assert max(dist) <= bound, (max(dist), bound)
    rest = ref["status"] != R.OK
    assert bits_equal(got["q"][rest], ref["q"][rest]) and bits_equal(got["t"][rest], ref["t"][rest])       # the unchanged pose of every other


def check(got, ref, D, poses, what, f32=False):
    """statuses, counts, inliers and edge_inlier exactly (under the margin condition), the poses of `poses` within the bound"""
    margin = R.decision_margin(ref)
    print(f"\n[pose refinement] {what}: margins (classification, depth, gain, pivot) {', '.join('%.2e' % m for m in margin)}, counts {ref['counts']}")
    assert min(margin) > MARGIN, margin
    assert np.array_equal(got["status"], ref["status"]), np.flatnonzero(got["status"] != ref["status"])
    assert [got[k] for k in POSEREF_STATUS_NAMES] == [ref["counts"][k] for k in POSEREF_STATUS_NAMES] and sum(ref["counts"].values()) == len(ref["status"])
    assert np.array_equal(got["inliers"], ref["inliers"]), np.flatnonzero(got["inliers"] != ref["inliers"])
    assert np.array_equal(got["edge_inlier"], ref["edge_inlier"]), np.flatnonzero(got["edge_inlier"] != ref["edge_inlier"])
    assert np.allclose(got["chi2"], ref["chi2"], rtol=1e-6 if f32 else 1e-9, atol=0)
    check_poses(got, ref, D, poses, what, f32)


# ---- 1. the exact part --------------------------------------------------------------------------------------------------------------------
SHORT = dict(rounds=3, iterations=1, robust_rounds=2, min_inliers=10)


@pytest.mark.parametrize("opts", [dict(), dict(landmark_reorder=0, pose_reorder=0), dict(device_setup=0)], ids=["default", "caller_order", "host_setup"])
def test_small_graph_over_options(true_fp, start, opts):
    ref, D, _ = reference(("small", 3, 1, 2), true_fp, start, D_POSES, **SHORT)
    assert ref["counts"]["ok"] == true_fp.Pf and ref["counts"]["fixed"] == 1 and not ref["edge_inlier"].all()
    h = HipSolver(true_fp, RK_HUBER, **opts)
    h.set_state(*start)
    got = h.refine_poses(**SHORT)
    check(got, ref, D, D_POSES, f"small graph {opts}")
    q, t, X = h.state()
    assert bits_equal(q, got["q"]) and bits_equal(t, got["t"]) and bits_equal(X, start[2])


@pytest.mark.parametrize("rounds,iterations,robust_rounds", [(3, 1, 0), (3, 1, 3), (2, 1, 2), (1, 2, 1)])
def test_small_graph_over_counts(true_fp, start, rounds, iterations, robust_rounds):
    args = dict(rounds=rounds, iterations=iterations, robust_rounds=robust_rounds, min_inliers=10)
    ref, D, _ = reference(("small", rounds, iterations, robust_rounds), true_fp, start, D_POSES, **args)
    h = HipSolver(true_fp, RK_HUBER)
    h.set_state(*start)
    check(h.refine_poses(**args), ref, D, D_POSES, f"small graph, {rounds} x {iterations}, robust_rounds {robust_rounds}")
    if (rounds, iterations) == (3, 1):
        # robust_rounds 0 against 2: another answer.  3 against 2: the same one -- an edge that is in at round 2 has omega |r|^2 below the
        # threshold, which is the Huber width squared, so the kernel is the identity on the round's edges where it is linearised
        other = reference(("small", 3, 1, 2), true_fp, start, D_POSES, **SHORT)[0]
        assert np.array_equal(ref["q"], other["q"]) == (robust_rounds == 3)


def test_tukey(true_fp, start):
    ref, D, _ = reference(("small-tukey",), true_fp, start, D_POSES, rk=RK_TUKEY_WIDE, **SHORT)
    assert not np.array_equal(ref["q"], reference(("small", 3, 1, 2), true_fp, start, D_POSES, **SHORT)[0]["q"])
    h = HipSolver(true_fp, RK_TUKEY_WIDE)
    h.set_state(*start)
    check(h.refine_poses(**SHORT), ref, D, D_POSES, "small graph, Tukey")


# Tukey widths at which the start's residuals (tens of px) still carry weight; conftest's 4 / 5 px give every edge of the start the weight 0:
# H = 0, SINGULAR everywhere (test_tukey_narrow_is_singular)
RK_TUKEY_WIDE = ((2, 300.0), (2, 400.0))


def test_tukey_narrow_is_singular(true_fp, start):
    """every edge of a pose outside the Tukey width: H = 0 exactly, lambda = 0, the first pivot is 0 in any summation order"""
    ref = R.refine(true_fp, state=start, rk=RK_TUKEY, poses=range(true_fp.Pt), **SHORT)
    sing = ref["status"] == R.SINGULAR
    zero_h = np.array([st is not None and st["status"] == R.SINGULAR and st["m_pivot"] and np.isnan(st["m_pivot"][0]) for st in ref["steps"]])
    assert zero_h.sum() >= 5
    h = HipSolver(true_fp, RK_TUKEY)
    h.set_state(*start)
    got = h.refine_poses(**SHORT)
    assert (got["status"][zero_h] == R.SINGULAR).all() and sing[zero_h].all()
    assert bits_equal(got["q"][zero_h], start[0][zero_h]) and bits_equal(h.state()[0][zero_h], start[0][zero_h])


def test_select_mask(true_fp, start):
    select = np.arange(true_fp.Pt) % 3 != 1
    ref, D, _ = reference(("small-select",), true_fp, start, D_POSES, select=select, **SHORT)
    assert ref["counts"]["not_selected"] == (~select).sum() and ref["status"][true_fp.Pt - 1] == (R.FIXED if select[-1] else R.NOT_SELECTED)
    h = HipSolver(true_fp, RK_HUBER)
    h.set_state(*start)
    got = h.refine_poses(select=select, **SHORT)
    check(got, ref, D, D_POSES, "select mask")
    assert bits_equal(h.state()[0][~select], start[0][~select]) and (got["inliers"][~select] == 0).all()
    live = np.asarray(true_fp.omega) > 0
    assert np.array_equal(got["edge_inlier"][~select[true_fp.eP]], live[~select[true_fp.eP]])


def test_wide_poses(wide_fp):
    fp = wide_fp
    q, t = R.perturbed_poses(fp, 12, rot_deg=5.0, trans=0.5)
    state = (q, t, fp.Xw.copy())
    poses = range(fp.Pf)
    ref, D, _ = reference(("wide",), fp, state, poses, **SHORT)
    assert ref["counts"]["ok"] == fp.Pf
    h = HipSolver(fp, RK_HUBER)
    h.set_state(*state)
    check(h.refine_poses(**SHORT), ref, D, poses, "poses of more than 128 edges")


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_zoo(zoo, precision):
    fp, idx, select, edge_mask, planted = zoo
    f32 = precision == "f32"
    args = SHORT
    poses = [p for p in range(fp.Pt)]
    omega = np.where(edge_mask, fp.omega, 0.0)
    ref, D, _ = reference(("zoo", precision), fp, None, poses, f32=f32, select=select, omega=omega, **args)
    want = dict(no_edges=R.FEW_OBSERVATIONS, two_edges=R.FEW_OBSERVATIONS, three_edges=R.FEW_INLIERS, n64=R.OK, n65=R.OK, n150=R.OK, mono_only=R.OK,
                stereo_only=R.OK, fixed_landmarks=R.OK, fixed_pose=R.FIXED, gated=R.OK, outliers=R.OK, behind=R.FEW_OBSERVATIONS,
                min_inliers=R.FEW_INLIERS, fill0=R.NOT_SELECTED)
    assert {k: int(ref["status"][idx[k]]) for k in want} == want
    n = np.bincount(fp.eP, minlength=fp.Pt)
    assert [int(n[idx[k]]) for k in ("no_edges", "two_edges", "three_edges", "n64", "n65", "n150")] == [0, 2, 3, 64, 65, 150]
    # the planted outliers: all seven are out at round 1, the near one is back at round 2 and stays
    hist = ref["steps"][idx["outliers"]]["history"]
    assert all(e in hist[0] for e in planted["far"] + [planted["near"]])
    assert not any(e in hist[1] for e in planted["far"] + [planted["near"]])
    assert planted["near"] in hist[2] and planted["near"] in hist[-1] and not any(e in hist[-1] for e in planted["far"])
    assert ref["inliers"][idx["gated"]] == 30 and not ref["edge_inlier"][~edge_mask].any()
    h = HipSolver(fp, RK_HUBER, precision=precision)
    h.set_edge_active(edge_mask)
    got = h.refine_poses(select=select, **args)
    check_zoo = [p for p in poses if p != idx["fill0"]]
    check(got, ref, D, check_zoo, f"zoo, {precision}", f32=f32)
    assert np.array_equal(h.edge_active(), edge_mask)
    if not f32:
        relaxed = h.refine_poses(select=select, dry_run=True, **dict(args, min_inliers=0))
        assert relaxed["status"][idx["min_inliers"]] == R.OK and relaxed["status"][idx["three_edges"]] == R.OK


def test_fp32_library_on_the_small_graph(true_fp, start):
    ref, D, _ = reference(("small-f32",), true_fp, start, D_POSES, f32=True, **SHORT)
    h = HipSolver(true_fp, RK_HUBER, precision="f32")
    h.set_state(*start)
    got = h.refine_poses(**SHORT)
    check(got, ref, D, D_POSES, "small graph, fp32 library", f32=True)
    assert bits_equal(h.state()[0], got["q"]) and bits_equal(h.state()[1], got["t"])


# ---- 2. long runs ---------------------------------------------------------------------------------------------------------------------------
LONG = dict(rounds=4, iterations=10, robust_rounds=2, min_inliers=10)
# D of a long run is no smooth number.  The third or fourth trial of a round is a step of about 1e-10 that changes F by 1e-20 of itself, so
# whether it is taken is rounding noise, in the reference and in the twin alike, and a pose ends one such step away or not.  Pose by pose the
# reference's distance from its own twin is 1.5e-16 ... 9.3e-10 on this graph (poses 0 ... 9, on the CPU: 1.2e-11, 8.7e-15, 5.9e-16, 7.4e-16,
# 1.5e-16, 9.3e-10, 5.5e-14, 1.5e-16, 1.4e-11, 9.6e-16): "the twin's own decisions already carry that noise" holds for the set, not pose by pose,
# and a pose whose twin happened to decide alike says nothing about where another summation order ends.  So the distance is bounded by 8 D with D
# the LARGEST over D_POSES (the poses of every other test here), which is a weak bound for the quiet poses; what holds every pose to its answer
# is the second assertion: at the device's pose the gradient of the last round's cost is as small as at the reference's.
LONG_POSES = D_POSES


def test_long_run(true_fp, start):
    ref, D, twin = reference(("small-long",), true_fp, start, LONG_POSES, **LONG)
    h = HipSolver(true_fp, RK_HUBER)
    h.set_state(*start)
    got = h.refine_poses(**LONG)
    print(f"\n[pose refinement] long run: counts {ref['counts']}")
    assert np.array_equal(got["status"], ref["status"])
    check_poses(got, ref, D, LONG_POSES, "long run 4 x 10")
    # pose by pose: the last round minimises the plain cost (robust_rounds = 2) over its own inliers; the 60-digit gradient of that cost at
    # the device's pose, relative to the size of its terms, is at most 8 x the largest the reference's own poses have
    assert R.decision_margin(ref)[0] > MARGIN                   # (the rounds' inlier sets are not in doubt)
    rel = {}
    for p in LONG_POSES:
        last = ref["steps"][p]["history"][LONG["rounds"] - 1]
        for k, res in enumerate((got, ref)):
            g, _, size = R.gradient_check(true_fp, start, true_fp.omega, p, last, res["q"][p], res["t"][p], RK_HUBER, False)
            rel[p, k] = float(np.abs(g).max() / 2 / size)
        own = R.pose_distance(ref["q"][p], ref["t"][p], twin[p]["q"], twin[p]["t"])
        print(f"[pose refinement] long run, pose {p}: device - reference {R.pose_distance(got['q'][p], got['t'][p], ref['q'][p], ref['t'][p]):.2e}, "
              f"reference - twin {own:.2e}, relative gradient device {rel[p, 0]:.2e} reference {rel[p, 1]:.2e}")
    assert all(rel[p, 0] <= 8 * max(rel[r, 1] for r in LONG_POSES) for p in LONG_POSES)


def test_minimiser(true_fp, start):
    """At the device's result of a long run with robust_rounds = rounds: the central-difference gradient of the 60-digit robust cost over
    the final inliers, relative to the size of its terms (sum over the edges of |w' J^T r|_inf), at most 8 x what the reference's own
    result gives.  Measured on the MI355X: 5.1e-10 at the device's result, 2.1e-9 at the reference's."""
    args = dict(LONG, robust_rounds=4)
    ref, _, _ = reference(("small-long-robust",), true_fp, start, [], **args)
    h = HipSolver(true_fp, RK_HUBER)
    h.set_state(*start)
    got = h.refine_poses(**args)
    assert np.array_equal(got["status"], ref["status"])
    lists = R.pose_edges(true_fp)
    worst = [0.0, 0.0]
    for p in LONG_POSES:
        assert ref["status"][p] == R.OK
        for k, res in enumerate((got, ref)):
            inl = [e for e in lists[p] if res["edge_inlier"][e]]
            g, _, size = R.gradient_check(true_fp, start, true_fp.omega, p, inl, res["q"][p], res["t"][p], RK_HUBER, True)
            worst[k] = max(worst[k], float(np.abs(g).max() / 2 / size))
    print(f"\n[pose refinement] minimiser: relative gradient at the device's result {worst[0]:.2e}, at the reference's {worst[1]:.2e}")
    assert worst[0] <= 8 * worst[1]


# ---- 3. what a call touches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_dry_run_changes_nothing(true_fp, start, precision):
    h = HipSolver(true_fp, RK_HUBER, precision=precision)
    h.set_state(*start)
    before = h.state()
    dry = h.refine_poses(dry_run=True, **SHORT)
    assert all(bits_equal(a, b) for a, b in zip(h.state(), before))
    real = h.refine_poses(**SHORT)
    for k in ("status", "inliers", "edge_inlier"):
        assert np.array_equal(dry[k], real[k])
    assert all(bits_equal(dry[k], real[k]) for k in ("q", "t", "chi2")) and dry["ok"] == real["ok"] > 0
    assert bits_equal(h.state()[0], real["q"]) and bits_equal(h.state()[1], real["t"]) and not bits_equal(h.state()[0], before[0])


def test_a_second_identical_call_is_bit_identical(true_fp, start):
    h = HipSolver(true_fp, RK_HUBER)
    runs = []
    for _ in range(2):
        h.set_state(*start)
        runs.append(h.refine_poses(**LONG))
    for k in ("status", "inliers", "edge_inlier"):
        assert np.array_equal(runs[0][k], runs[1][k])
    assert all(bits_equal(runs[0][k], runs[1][k]) for k in ("q", "t", "chi2"))


def test_what_stays(true_fp, start):
    """landmarks, unselected / fixed / rejected poses, edge_active(), the snapshot slots and the counters: bit-equal to before"""
    fp = true_fp
    h = HipSolver(fp, RK_HUBER)
    h.set_state(*start)
    h.optimize(1)
    mask = np.arange(fp.E) % 7 != 0
    mask[fp.eP == 3] = np.arange((fp.eP == 3).sum()) < 5           # pose 3 keeps 5 edges: FEW_INLIERS with min_inliers = 10
    mask[fp.eP == 4] = np.arange((fp.eP == 4).sum()) < 2           # pose 4 keeps 2: FEW_OBSERVATIONS
    h.set_edge_active(mask)
    h.snapshot_state(0)
    select = np.arange(fp.Pt) % 4 != 2
    q0, t0, X0 = h.state()
    counters = h.counters()
    got = h.refine_poses(select=select, **SHORT)
    q1, t1, X1 = h.state()
    ok = got["status"] == R.OK
    assert got["status"][3] == R.FEW_INLIERS and got["status"][4] == R.FEW_OBSERVATIONS and got["status"][fp.Pt - 1] == R.FIXED
    assert (got["status"][~select] == R.NOT_SELECTED).all() and ok.sum() > 20
    assert bits_equal(X1, X0) and bits_equal(q1[~ok], q0[~ok]) and bits_equal(t1[~ok], t0[~ok])
    assert bits_equal(q1[ok], got["q"][ok]) and not np.array_equal(q1[ok], q0[ok])
    assert np.array_equal(h.edge_active(), mask) and h.counters() == counters
    assert not got["edge_inlier"][~mask].any()
    h.restore_state(0)
    assert all(bits_equal(a, b) for a, b in zip(h.state(), (q0, t0, X0)))


def test_covariance_is_dropped_after_a_change(true_fp, start):
    fp = true_fp
    h = HipSolver(fp, RK_HUBER)
    h.optimize(3)
    h.covariance(landmarks=False)
    before = h.covariance_blocks()
    h.refine_poses(dry_run=True, **SHORT)
    assert bits_equal(h.covariance_blocks(), before)               # (a dry run keeps it)
    h.set_state(*start)
    h.covariance(landmarks=False)
    assert h.refine_poses(**SHORT)["ok"] > 0
    with pytest.raises(CubaHipError):
        h.covariance_blocks()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_optimize_after_refinement_equals_a_handle_set_to_that_state(true_fp, start, precision):
    fp = true_fp
    h = HipSolver(fp, RK_HUBER, precision=precision)
    h.set_state(*start)
    assert h.refine_poses(**LONG)["ok"] == fp.Pf
    twin = HipSolver(fp, RK_HUBER, precision=precision)
    twin.set_state(*h.state())
    assert all(bits_equal(a, b) for a, b in zip(h.state(), twin.state()))
    assert bits_equal(h.chi_squares(), twin.chi_squares())
    a, b = h.optimize(5)["chi2"], twin.optimize(5)["chi2"]
    assert len(a) == len(b) > 0 and bits_equal(a, b) and all(bits_equal(x, y) for x, y in zip(h.state(), twin.state()))
    assert bits_equal(h.chi_squares(), twin.chi_squares()) and np.array_equal(h.edge_active(), twin.edge_active())


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(CubaHipError) as e:
        call()
    return int(re.match(r"status (\d+)", str(e.value)).group(1))


def test_errors_and_the_handle_afterwards(small_fp):
    fp = small_fp
    STATE, ARG = 3, 1
    assert status_of(HipSolver(None, RK_HUBER).refine_poses) == STATE
    for part in (lambda s: s.set_partition(0, fp.Lt // 2), lambda s: s.set_graph(fp, landmark_range=(0, fp.Lt // 2))):
        p = HipSolver(fp, RK_HUBER)
        part(p)
        assert status_of(p.refine_poses) == STATE
    h = HipSolver(fp, RK_HUBER)
    before = h.state()
    for bad in (dict(rounds=0), dict(rounds=5), dict(iterations=0), dict(iterations=33), dict(robust_rounds=-1), dict(rounds=2, robust_rounds=3),
                dict(min_inliers=-1), dict(chi2_max=(np.nan, 7.815)), dict(chi2_max=(5.991, np.nan))):
        assert status_of(lambda: h.refine_poses(**bad)) == ARG
    assert h.lib.cuba_hip_refine_poses(h.h, None, 4, 10, 2, None, 10, 0, None, None, None, None, None, None, None) == ARG        # chi2_max NULL
    with pytest.raises(ValueError):
        h.refine_poses(select=np.ones(fp.Pt + 1, bool))
    assert all(bits_equal(a, b) for a, b in zip(h.state(), before))
    # every output is optional, 4 x 32 trials are allowed, and the handle goes on
    assert h.lib.cuba_hip_refine_poses(h.h, None, 4, 32, 4, (2 * C.c_double)(np.inf, np.inf), 0, 1, None, None, None, None, None, None, None) == 0
    got = h.refine_poses(rounds=4, iterations=32, chi2_max=(np.inf, np.inf), dry_run=True)
    assert got["ok"] > fp.Pf // 2 and sum(got[k] for k in POSEREF_STATUS_NAMES) == fp.Pt and all(bits_equal(a, b) for a, b in zip(h.state(), before))
    chi2 = h.optimize(5)["chi2"]
    assert len(chi2) > 1 and chi2[-1] < chi2[0]

"""The fp64 reference of pose refinement (tests/pose_refinement_reference.py) against its own 60-digit mpmath twin, which runs the same numeric
steps and takes its own accept / reject decisions, and an independent check of the Jacobian convention.  No GPU.

D = the largest pose distance between the two -- the larger of |dt|_inf / max(1, |t|_inf) and the rotation angle of dR -- is the yardstick
of tests/test_gpu_pose_refinement.py (8 D for the device); it is printed here.  Measured: 4.7e-16 on the small graph
after 3 rounds of 1 trial from a start 5 degrees and 0.5 m off, 1.5e-15 on the poses of 129 ... 300 edges, 2.8e-14 on the zoo, and
1.2e-11 after 4 x 10 trials, where the late trials' decisions are rounding noise in both."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_refinement_reference as R  # noqa: E402

from conftest import RK_HUBER  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402

SHORT = dict(rounds=3, iterations=1, robust_rounds=2, min_inliers=10)
POSES = range(6)


@pytest.fixture(scope="module")
def true_fp():
    from cuba_amd.synth import synth_ba
    return flatten(synth_ba(40, 600, 2400, seed=1, perturb=False))


@pytest.fixture(scope="module")
def start(true_fp):
    q, t = R.perturbed_poses(true_fp, 11, rot_deg=5.0, trans=0.5)
    return q, t, true_fp.Xw.copy()


@pytest.fixture(scope="module")
def short_ref(true_fp, start):
    return R.refine(true_fp, state=start, rk=RK_HUBER, **SHORT)


def test_reference_against_its_60_digit_twin(short_ref):
    ref = short_ref
    margin = R.decision_margin(ref)
    D, statuses, twin = R.model_distance(ref, POSES)
    print(f"\n[pose refinement reference] small graph 3 x 1: margins {margin}, D = {D:.2e}")
    assert min(margin) > 1e-6
    for p in POSES:
        a, b = ref["steps"][p], twin[p]
        # with every decision clear of its decision point the twin decides alike: statuses, inlier sets at every classification, accepted trials
        assert statuses[p] == ref["status"][p] == R.OK and a["history"] == b["history"] and a["accepted"] == b["accepted"]
        assert abs(a["chi2"] - b["chi2"]) <= 1e-9 * b["chi2"]
    assert 0 < D < 1e-12


def test_the_refinement_moves_the_poses_to_the_truth(true_fp, start):
    """4 x 10 trials from 5 degrees and 0.5 m off end where the measurements put the poses: within the noise of the true ones"""
    ref = R.refine(true_fp, state=start, rk=RK_HUBER, rounds=4, iterations=10, robust_rounds=2, min_inliers=10, poses=POSES)
    for p in POSES:
        before = R.pose_distance(start[0][p], start[1][p], true_fp.q[p], true_fp.t[p])
        after = R.pose_distance(ref["q"][p], ref["t"][p], true_fp.q[p], true_fp.t[p])
        assert ref["status"][p] == R.OK and before > 0.02 and after < 0.02 and after < before / 3


def test_long_run_against_the_twin(true_fp, start):
    ref = R.refine(true_fp, state=start, rk=RK_HUBER, rounds=4, iterations=10, robust_rounds=2, min_inliers=10, poses=range(2))
    D, statuses, _ = R.model_distance(ref, range(2))
    print(f"\n[pose refinement reference] small graph 4 x 10: D = {D:.2e}")
    assert all(s == R.OK for s in statuses.values()) and D < 1e-8


def test_jacobian_convention_by_central_differences(true_fp, start):
    """dF / dd at d = 0 of F(exp(d) T), by central differences of the 60-digit robust cost, is -2 b: J = -dr / dd for the LEFT update"""
    lists = R.pose_edges(true_fp)
    for p in (0, 7):
        edges = [e for e in lists[p] if true_fp.omega[e] > 0]
        eds = R.load_edges(true_fp, start, true_fp.omega, edges, R.Arith)
        Rm = R.rotation([float(v) for v in start[0][p]])
        edges = [e for e, ed in zip(edges, eds) if R.edge_residual(ed, Rm, [float(v) for v in start[1][p]], R.Arith)[0][2] > 0]
        for use_robust in (True, False):
            g, b, size = R.gradient_check(true_fp, start, true_fp.omega, p, edges, start[0][p], start[1][p], RK_HUBER, use_robust)
            err = np.abs(g + 2 * b).max() / np.abs(b).max()
            print(f"\n[pose refinement reference] pose {p}, robust {use_robust}: |grad + 2 b| / |b| = {err:.2e}")
            assert np.abs(b).max() > 1 and err < 1e-10
    # a right-multiplicative update would not pass: the same cost differentiated along T exp(d)
    import mpmath
    p = 0
    edges = [e for e in lists[p] if true_fp.omega[e] > 0][:20]
    with mpmath.workdps(60):
        eds = R.load_edges(true_fp, start, true_fp.omega, edges, R.ArithMp)
        q, t = [R.ArithMp.num(v) for v in start[0][p]], [R.ArithMp.num(v) for v in start[1][p]]
        ident_q, ident_t = [mpmath.mpf(0)] * 3 + [mpmath.mpf(1)], [mpmath.mpf(0)] * 3
        grad = []
        for k in range(6):
            f = []
            for sgn in (1, -1):
                d = [mpmath.mpf(0)] * 6
                d[k] = sgn * mpmath.mpf(10) ** -15
                qe, te = R.exp_update(d, ident_q, ident_t, R.ArithMp)          # exp(d)
                # T exp(d): rotation q * qe, translation R(q) te + t
                qq, tt = R.exp_update([mpmath.mpf(0)] * 6, q, t, R.ArithMp)
                Rq = R.rotation(qq)
                t2 = [sum(Rq[i][j] * te[j] for j in range(3)) + tt[i] for i in range(3)]
                q2 = [qq[3] * qe[0] + qq[0] * qe[3] + qq[1] * qe[2] - qq[2] * qe[1],
                      qq[3] * qe[1] + qq[1] * qe[3] + qq[2] * qe[0] - qq[0] * qe[2],
                      qq[3] * qe[2] + qq[2] * qe[3] + qq[0] * qe[1] - qq[1] * qe[0],
                      qq[3] * qe[3] - qq[0] * qe[0] - qq[1] * qe[1] - qq[2] * qe[2]]
                f.append(R.cost(eds, range(len(edges)), q2, t2, RK_HUBER, True, R.ArithMp))
            grad.append(float((f[0] - f[1]) / (2 * mpmath.mpf(10) ** -15)))
    _, b, _ = R.gradient_check(true_fp, start, true_fp.omega, p, edges, start[0][p], start[1][p], RK_HUBER, True)
    assert np.abs(np.array(grad) + 2 * b).max() / np.abs(b).max() > 1e-3


def test_zoo_statuses_and_the_returning_outlier():
    fp, idx, select, edge_mask, planted = R.zoo_problem()
    ref = R.refine(fp, select=select, omega=np.where(edge_mask, fp.omega, 0.0), rk=RK_HUBER, **SHORT)
    want = dict(no_edges=R.FEW_OBSERVATIONS, two_edges=R.FEW_OBSERVATIONS, three_edges=R.FEW_INLIERS, n64=R.OK, n65=R.OK, n150=R.OK, mono_only=R.OK,
                stereo_only=R.OK, fixed_landmarks=R.OK, fixed_pose=R.FIXED, gated=R.OK, outliers=R.OK, behind=R.FEW_OBSERVATIONS,
                min_inliers=R.FEW_INLIERS, fill0=R.NOT_SELECTED)
    assert {k: int(ref["status"][idx[k]]) for k in want} == want and sum(ref["counts"].values()) == fp.Pt
    hist = ref["steps"][idx["outliers"]]["history"]
    seven = planted["far"] + [planted["near"]]
    assert all(e in hist[0] for e in seven) and not any(e in hist[1] for e in seven)
    assert planted["near"] in hist[2] and planted["near"] in hist[-1] and not any(e in hist[-1] for e in planted["far"])
    assert min(R.decision_margin(ref)) > 1e-6
    D, statuses, _ = R.model_distance(ref, [idx["outliers"], idx["n150"], idx["mono_only"]])
    print(f"\n[pose refinement reference] zoo: D = {D:.2e}")
    assert all(s == R.OK for s in statuses.values()) and D < 1e-11


def test_pose_distance():
    q = np.array([0.0, 0.0, 0.0, 1.0])
    a = 1e-13
    q2 = np.array([0.0, 0.0, np.sin(a / 2), np.cos(a / 2)])
    assert abs(R.pose_distance(q, [0, 0, 0], q2, [0, 0, 0]) - a) < 1e-3 * a            # an angle far below sqrt(eps)
    assert R.pose_distance(q, [10.0, 0, 0], q, [10.0, 0, 1e-9]) == pytest.approx(1e-10, rel=1e-6)
    assert R.pose_distance(q2, [0, 0, 0], -q2, [0, 0, 0]) == 0                        # (q and -q are one rotation)

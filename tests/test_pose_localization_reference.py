"""The reference for pose localisation (tests/pose_localization_reference.py) on its own, without a GPU: the hash's constants, the P3P solver
on exact data in fp64 and in its 60-digit twin, the degenerate samples, the independence of the caller's edge order, and the margin
condition of every input that tests/test_gpu_pose_localization.py compares the device on."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_localization_reference as L  # noqa: E402
import pose_refinement_reference as PR  # noqa: E402


# ---- the hash ---------------------------------------------------------------------------------------------------------------------------
def test_hash_golden_values():
    """splitmix64's finaliser (shifts 30, 27, 31; multipliers bf58476d1ce4e5b9, 94d049bb133111eb), four rounds over seed + golden ratio,
    p, h, e; values from the definition worked by hand in python integers"""
    assert L.mix(0) == 0 and L.mix(1) == 0x5692161d100b05e5
    assert L.key(0, 0, 0, 0) == 0x1957a7604e215178
    assert L.key(1, 2, 3, 4) == 0x1d4407ef703b1906
    assert L.key(2 ** 64 - 1, 5, 4095, 2399) == 0x2f9cd49d24d6911d
    assert L.key(12345, 39, 256, 100000) == 0x7634fccfa52272c6


def test_samples_follow_the_keys():
    usable = [3, 17, 4, 99, 250, 12]
    got = L.samples(7, 2, 5, usable)
    for h in range(5):
        want = sorted(usable, key=lambda e: (L.key(7, 2, h, e), e))[:3]
        assert list(got[h]) == want
    # the caller's index of an edge decides, not its position
    ids = np.arange(300)[::-1].copy()
    moved = L.samples(7, 2, 5, [int(np.flatnonzero(ids == e)[0]) for e in usable], edge_ids=ids)
    assert np.array_equal(ids[moved], got)


# ---- P3P on exact data ----------------------------------------------------------------------------------------------------------------------
def exact_triples(n, seed=0):
    """n random poses with three points in front of the camera: (R, t, bearings, points), the bearings computed from the true pose"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        R = Rotation.from_rotvec(2.0 * rng.uniform(-1, 1, 3)).as_matrix()
        t = rng.uniform(-1, 1, 3)
        Xc = np.column_stack([rng.uniform(-4, 4, 3), rng.uniform(-3, 3, 3), rng.uniform(4, 20, 3)])
        X = (Xc - t) @ R                          # X = R^T (Xc - t)
        out.append((R, t, X))
    return out


def pose_error(Rc, tc, R, t, depth):
    """(rotation angle of Rc^T R, |tc - t| / depth) in floats"""
    Rc, tc = np.array([[float(x) for x in row] for row in Rc]), np.array([float(x) for x in tc])
    c = (np.trace(Rc.T @ R) - 1) / 2
    s = np.linalg.norm(Rc.T @ R - (Rc.T @ R).T) / (2 * np.sqrt(2))          # sin of the angle: exact for small angles
    return max(float(np.arctan2(s, c)), float(np.abs(tc - t).max() / depth))


def real_roots(X, f):
    k = L.quartic(f, X, L.Arith)
    return 2 * int(k["disc"][0] >= 0) + 2 * int(k["disc"][1] >= 0)


def test_p3p_recovers_the_pose_on_exact_data_fp64():
    counts = []
    for R, t, X in exact_triples(60):
        Xc = X @ R.T + t
        f = [[float(v) for v in x / np.linalg.norm(x)] for x in Xc]
        Xl = [[float(v) for v in x] for x in X]
        cands = L.p3p(f, Xl)
        counts.append(real_roots(Xl, f))
        assert cands and min(pose_error(Rc, tc, R, t, Xc[:, 2].mean()) for _, Rc, tc in cands) < 1e-9
    # quartics of two and of four real roots are both met
    assert 2 in counts and 4 in counts, np.bincount(counts)


def test_p3p_recovers_the_pose_on_exact_data_in_the_twin():
    import mpmath
    with mpmath.workdps(60):
        for R, t, X in exact_triples(12, seed=1):
            # the true pose and the points as 60-digit numbers; the bearings from them with 60 digits
            Rm = [[mpmath.mpf(float(v)) for v in row] for row in R]
            # (R from floats is orthonormal to 1e-16 only: orthonormalise with 60 digits through the quaternion)
            q = L.quaternion(Rm, L.ArithMp)
            Rm = [[mpmath.mpf(v) for v in row] for row in PR.rotation(q)]
            tm = [mpmath.mpf(float(v)) for v in t]
            Xm = [[mpmath.mpf(float(v)) for v in x] for x in X]
            Xc = [[sum(Rm[i][j] * x[j] for j in range(3)) + tm[i] for i in range(3)] for x in Xm]
            f = [L.unit(x, L.ArithMp) for x in Xc]
            cands = L.p3p(f, Xm, L.ArithMp)
            depth = sum(x[2] for x in Xc) / 3
            err = []
            for _, Rc, tc in cands:
                dR = max(abs(Rc[i][j] - Rm[i][j]) for i in range(3) for j in range(3))
                err.append(max(dR * 2, max(abs(tc[i] - tm[i]) for i in range(3)) / depth))      # (angle <= 2 max |dR_ij| for small angles)
            assert cands and min(err) < mpmath.mpf("1e-40"), min(err)


def test_degenerate_triples_leave_no_candidate():
    R, t, X = exact_triples(1, seed=2)[0]
    line = np.array([1.0, 0.5, 9.0])[None, :] + np.array([0.0, 1.3, 2.9])[:, None] * np.array([0.7, -0.2, 1.1])[None, :]
    twice = np.array([[1.0, 0.5, 9.0], [1.0, 0.5, 9.0], [-2.0, 1.0, 12.0]])
    for Xc in (line, twice, twice[[0, 2, 1]], twice[[2, 0, 1]]):
        Xw = (Xc - t) @ R
        f = [[float(v) for v in x / np.linalg.norm(x)] for x in Xc]
        assert L.p3p(f, [[float(v) for v in x] for x in Xw]) == []
    import mpmath
    with mpmath.workdps(60):
        f = [[mpmath.mpf(float(v)) for v in x / np.linalg.norm(x)] for x in line]
        assert L.p3p(f, [[mpmath.mpf(float(v)) for v in x] for x in (line - t) @ R], L.ArithMp) == []


# ---- the caller's edge order ------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_order_of_the_callers_edges():
    fp, ref, _, _ = L.gpu_case("wide", 64)
    rng = np.random.default_rng(5)
    perm = rng.permutation(fp.E)                      # position i of the shuffled graph holds the caller's edge perm[i]
    sh = copy.copy(fp)
    sh.eP, sh.eL, sh.eDim = np.asarray(fp.eP)[perm], np.asarray(fp.eL)[perm], np.asarray(fp.eDim)[perm]
    sh.meas, sh.omega = np.asarray(fp.meas)[perm], np.asarray(fp.omega)[perm]
    got = L.localize(sh, hypotheses=64, seed=L.SEED["wide"], edge_ids=perm)
    for k in ("status", "winner", "inliers"):
        assert np.array_equal(got[k], ref[k])
    assert np.array_equal(got["edge_inlier"], ref["edge_inlier"][perm])
    # the pose is a function of the three points in key order: bit for bit; the score's sum runs in another order
    assert np.array_equal(got["q"], ref["q"]) and np.array_equal(got["t"], ref["t"])
    assert np.allclose(got["cost"], ref["cost"], rtol=1e-12, atol=0)


# ---- the definition's statuses on the tiny graph -----------------------------------------------------------------------------------------
def test_statuses_on_the_tiny_graph():
    fp, idx, edges = L.tiny_problem()
    omega = np.array(fp.omega, dtype=np.float64)
    omega[edges["gated"]] = 0
    select = np.ones(fp.Pt, bool); select[idx["four"]] = False
    ref = L.localize(fp, hypotheses=8, seed=3, omega=omega, min_inliers=5, select=select)
    want = dict(three=L.FEW_OBSERVATIONS, four=L.NOT_SELECTED, five=L.OK, collinear=L.NO_SOLUTION, gated=L.FEW_OBSERVATIONS, fixed=L.FIXED)
    assert {k: int(ref["status"][idx[k]]) for k in want} == want
    assert ref["inliers"][idx["five"]] == 5 and ref["inliers"][idx["three"]] == 3 and ref["inliers"][idx["gated"]] == 0
    assert sum(ref["counts"].values()) == fp.Pt
    ref = L.localize(fp, hypotheses=8, seed=3, omega=omega, min_inliers=6)
    assert ref["status"][idx["five"]] == L.FEW_INLIERS and ref["status"][idx["four"]] == L.FEW_INLIERS and ref["winner"][idx["five"]] == -1
    # the winner of an exact graph is the true pose
    ref = L.localize(fp, hypotheses=8, seed=3, omega=omega, min_inliers=0)
    for k in ("four", "five"):
        assert PR.pose_distance(ref["q"][idx[k]], ref["t"][idx[k]], fp.q[idx[k]], fp.t[idx[k]]) < 1e-9


# ---- decision_margin, and the condition of the GPU tests' inputs ---------------------------------------------------------------------------
def test_decision_margin_sees_a_near_tie_and_a_near_threshold():
    fp, ref, margins, _ = L.gpu_case("wide", 64)
    p = 2
    st = ref["steps"][p]
    a, b = margins[p]
    C = [c for c, _, _ in st["candidates"]]
    assert a == pytest.approx((C[1] - C[0]) / C[0]) and a > 0
    # (b): the closest chi2 to its threshold at the winner, as fp64 sees it, agrees with the twin's figure to fp64 accuracy
    _, depth, chi, _ = L.score(st["pe"], st["R"], st["t"], ref["args"]["chi2_max"])
    cap = np.where(st["pe"].stereo > 0, L.CHI2_STEREO, L.CHI2_MONO)
    assert b == pytest.approx(min(float(np.min(np.abs(chi - cap) / cap)), float(np.min(np.abs(depth) / np.maximum(np.abs(depth), 1)))), rel=1e-6)


@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("hypotheses", L.HYPOTHESES)
def test_margin_condition_of_the_gpu_inputs(name, hypotheses):
    """for the reference alone: every pose with a winner has margin (a) > 1e-6 and margin (b) > 1e-6, on exactly the inputs and seeds of
    tests/test_gpu_pose_localization.py"""
    fp, ref, margins, D = L.gpu_case(name, hypotheses)
    assert set(margins) == {p for p in range(fp.Pt) if ref["status"][p] in (L.OK, L.FEW_INLIERS)}
    print(f"\n[pose localisation] {name}, {hypotheses} hypotheses: counts {ref['counts']}, smallest margins (a) "
          f"{min(v[0] for v in margins.values()):.2e} (b) {min(v[1] for v in margins.values()):.2e}, largest D {max(D.values(), default=0):.2e}")
    assert all(a > L.MARGIN and b > L.MARGIN for a, b in margins.values()), margins
    if hypotheses >= 64:
        assert ref["counts"]["ok"] == fp.Pf
        # with one edge in five a gross outlier the winner still lies at the true pose to the noise
        assert max(PR.pose_distance(ref["q"][p], ref["t"][p], fp.q[p], fp.t[p]) for p in range(fp.Pf)) < 0.1
        n = np.bincount(fp.eP, minlength=fp.Pt)[:fp.Pf]
        assert (ref["inliers"][:fp.Pf] >= 10).all() and (ref["inliers"][:fp.Pf] < n).all()


def test_margin_condition_of_the_other_gpu_cases():
    """the fp32 library's case (the reference on float-rounded inputs), the subset and the second seed of test 6"""
    for name in ("small", "wide"):
        for args in (dict(f32=True), dict(seed=L.SEED[name] + 100)):
            _, ref, margins, _ = L.gpu_case(name, 256, **args)
            assert all(a > L.MARGIN and b > L.MARGIN for a, b in margins.values()), (name, args, margins)

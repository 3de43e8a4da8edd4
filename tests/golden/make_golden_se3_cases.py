"""Generates tests/golden/se3_cases.npz: the case table of tests/test_se3_mp_reference.py and tests/test_gpu_factor_regimes.py -- the inputs
of pose priors, relative-pose edges, position factors and landmark priors on the 60-pose synthetic graph, in every branch of the SE(3)
kernels, and what tests/se3_mp_reference.py (mpmath, 60 digits) makes of them.  Data only; needs mpmath and no GPU.  Run from the repo
root: `python tests/golden/make_golden_se3_cases.py`.

Each SE(3) case is a residual prescribed as a tangent r = (theta * axis, upsilon), |upsilon| ~ 1: the measurement is exp(-r) T (priors) or
exp(-r) T_j T_i^-1 (edges) at 60 digits, rounded to fp64; the expected outputs are then computed from the ROUNDED numbers.  Two scenes:
"near", the graph as synthesised, and "moved", the same graph moved rigidly by c = (800, -500, 300) (landmarks X + c, poses t - R c: the
projections are unchanged, the pose translations become ~1e3).  Keys of the file: "<scene>/q", "<scene>/t" (the pose estimates, a few
quaternions negated), and per factor kind "<scene>/<kind>/<name>" with the inputs as the HipSolver setters take them, kind / delta of the
robust kernel of each case (0: none), theta and ratio (the prescribed angle and e / delta^2; NaN where it does not apply), and the outputs
r, e, rho, w = rho', flip (the relative quaternion has a negative scalar part), H / g (J^T Omega J, J^T Omega r per end, UNWEIGHTED) and for
the edges Hij = J_i^T Omega J_j."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import se3_mp_reference as ref  # noqa: E402
from test_gpu_relative_pose import covisible  # noqa: E402

from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "se3_cases.npz")
SCENES = ("near", "moved")
SHIFT = np.array([800.0, -500.0, 300.0])
THETAS = (0.0, 1e-9, 1e-6, 1.9e-4, 2.1e-4, 1e-3, 0.05, 0.2499, 0.2501, 0.5, 2.0, 3.1, float(np.pi) - 1e-6)
REL_THETAS = (0.0, 1e-3, 0.2499, 0.5, 2.0, 3.1)
RATIOS = (0.0, 0.25, 1 - 1e-9, 1 + 1e-9, 4.0, 1e6)
KERNELS = (ref.HUBER, ref.TUKEY, ref.CAUCHY)
NEGATED = (3, 9, 14, 22, 31, 40, 52)          # poses whose estimate is given as -q (w < 0)
PAIR_NEAR, PAIR_FAR, PAIR_FLIP, PAIR_FIXED, PAIR_DOUBLE = 0, 1, 2, 3, 4
NAN = float("nan")


def graph():
    return flatten(synth_ba(60, 900, 3600, seed=2))


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rotate(R, v):
    """R v as explicit sums in index order (the table must not depend on a BLAS)"""
    return np.array([R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)])


def norm(v):
    s = 0.0
    for x in v:
        s += float(x) * float(x)
    return s ** 0.5


def scene_state(fp, scene):
    """(q, t, Xw) of a scene: the synthesised estimates, the quaternions of NEGATED negated; "moved": landmarks X + c, poses t - R c"""
    q, t, X = np.array(fp.q, dtype=np.float64), np.array(fp.t, dtype=np.float64), np.array(fp.Xw, dtype=np.float64)
    if scene == "moved":
        t = np.array([t[p] - rotate(quat_to_rot(q[p]), SHIFT) for p in range(len(q))])
        X = X + SHIFT
    q[list(NEGATED)] *= -1.0
    return q, t, X


def tangent(rng, theta):
    axis = rng.normal(size=3)
    axis /= norm(axis)
    u = rng.normal(size=3)
    u *= (0.7 + 0.6 * rng.random()) / norm(u)
    return np.concatenate([theta * axis, u])


def information(rng, dim, scale=1000.0):
    A = rng.normal(size=(dim, dim))
    M = np.zeros((dim, dim))
    for i in range(dim):
        for j in range(i, dim):          # A A^T as explicit sums in index order, symmetric by construction
            m = 0.0
            for k in range(dim):
                m += float(A[i, k]) * float(A[j, k])
            M[i, j] = M[j, i] = m
    return scale * (np.eye(dim) + 0.25 / dim * M)


def floats(v):
    return np.array([float(x) for x in v])


def measurement(r, T):
    """exp(-r) T at 60 digits, T = (unit quaternion, t): (quaternion, translation) rounded to fp64"""
    q, t = T
    w = [-ref.mpf(x) for x in r[:3]]
    dq = ref.quat_exp(w)
    dR, dt = ref.exp6([-ref.mpf(x) for x in r])
    qm = ref.quat_mul(dq, q)
    tm = dR * t + dt
    return floats(qm), floats(tm)


def mp_pose(q, t):
    return ref.quat_unit([ref.mpf(x) for x in q]), ref.column(t)


def mp_relative(qi, ti, qj, tj):
    """T_j T_i^-1 as (unit quaternion, t) at 60 digits"""
    a, ta = mp_pose(qi, ti)
    b, tb = mp_pose(qj, tj)
    qm = ref.quat_mul(b, ref.quat_conj(a))
    return qm, tb - ref.quat_rot(qm) * ta


def kernel_plan(n_regime):
    """(kind, ratio) per case: none on the first n_regime cases, then RATIOS under each of KERNELS"""
    return [(ref.NONE, NAN)] * n_regime + [(k, x) for k in KERNELS for x in RATIOS]


def delta_for(e, ratio):
    """delta with e / delta^2 = ratio (ratio 0: a zero residual, any delta)"""
    return 1.0 if ratio == 0.0 else float(ref.mp.sqrt(e / ref.mpf(ratio)))


def robust_outputs(kind, delta, e):
    return float(ref.rho(kind, delta, e)), float(ref.weight(kind, delta, e))


def pick_pairs(fp):
    """disjoint pairs of free poses: (near pairs, far pairs), the far ones led by (0, Pf - 1)"""
    have = covisible(fp)
    assert (0, fp.Pf - 1) not in have
    used, near, far = {0, fp.Pf - 1}, [], [(0, fp.Pf - 1)]
    for lo in range(1, fp.Pf):
        for hi in range(fp.Pf - 2, lo + 20, -1):          # the farthest unused partner that shares no landmark
            if len(far) < 13 and lo not in used and hi not in used and (lo, hi) not in have:
                far.append((lo, hi))
                used |= {lo, hi}
    for a, b in sorted(have):
        if a not in used and b not in used and len(near) < 8:
            near.append((a, b))
            used |= {a, b}
    singles = [p for p in range(fp.Pf) if p not in used]
    assert len(far) == 13 and len(near) == 8 and len(singles) >= 16
    return near, far, singles


def prior_cases(q, t, rng):
    out = {k: [] for k in ("pose", "qb", "tb", "info", "kind", "delta", "theta", "ratio", "r", "e", "rho", "w", "flip", "H", "g")}
    plan = [(th, sign, 1.0) for th in THETAS for sign in (1.0, -1.0)] + [(0.5, 1.0, 1.001)]
    kernels = kernel_plan(len(plan))
    for p, (kind, ratio) in enumerate(kernels):
        theta, sign, scale = plan[p] if p < len(plan) else ((0.1, 0.7)[p % 2], (1.0, -1.0)[(p // 2) % 2], 1.0)
        r = np.zeros(6) if ratio == 0.0 else tangent(rng, theta)
        if ratio == 0.0:
            qb, tb = q[p].copy(), t[p].copy()
        else:
            qb, tb = measurement(r, mp_pose(q[p], t[p]))
        qb = sign * scale * qb
        info = information(rng, 6)
        rr, e, H, g = ref.prior_terms(q[p], t[p], qb, tb, info)
        delta = 0.0 if kind == ref.NONE else delta_for(e, ratio)
        rho, w = robust_outputs(kind, delta, e)
        for k, v in zip(out, (p, qb, tb, info, kind, delta, theta, ratio, floats(rr), float(e), rho, w, bool(ref.prior_flip(q[p], qb)), ref.to_array(H), floats(g))):
            out[k].append(v)
    return out


def relative_cases(fp, q, t, rng):
    names = ("i", "j", "qz", "tz", "info", "kind", "delta", "theta", "ratio", "pair", "r", "e", "rho", "w", "flip", "Hii", "Hjj", "Hij", "gi", "gj")
    out = {k: [] for k in names}
    near, far, singles = pick_pairs(fp)
    fixed = fp.Pt - 1
    assert fixed >= fp.Pf
    near, far, flips = list(near), list(far[:8]), list(far[8:])
    ends = [(fixed, p) if x % 2 == 0 else (p, fixed) for x, p in enumerate(singles)]

    def pair_of(pk):
        """the next unused pair of a kind: far pairs from (0, Pf - 1) on, the (j, i) ones from the far pairs set aside for them"""
        if pk == PAIR_FLIP:
            a, b = flips.pop(0)
            return b, a
        return near.pop(0) if pk == PAIR_NEAR else far.pop(0) if pk in (PAIR_FAR, PAIR_DOUBLE) else ends.pop(0)

    kinds = (PAIR_NEAR, PAIR_FAR, PAIR_FLIP, PAIR_FIXED)
    plan = []          # (i, j, pair kind, theta, sign of qz)
    # every angle with both signs, the pair kind rotated against the angle: each kind meets the series and the closed form under both signs
    for x, theta in enumerate(REL_THETAS):
        for y, sign in enumerate((1.0, -1.0)):
            pk = kinds[(x + 2 * y) % 4]
            plan.append(pair_of(pk) + (pk, theta, sign))
    # ... and theta = 0.5, 2 and 3.1 on the kinds the rotation left out: the closed form at all three through every store
    have = {(pk, theta) for _, _, pk, theta, _ in plan}
    for x, (theta, pk) in enumerate((th, pk) for th in (0.5, 2.0, 3.1) for pk in kinds):
        if (pk, theta) not in have:
            plan.append(pair_of(pk) + (pk, theta, (1.0, -1.0)[x % 2]))
    i, j = pair_of(PAIR_DOUBLE)
    plan += [(i, j, PAIR_DOUBLE, 0.5, 1.0), (i, j, PAIR_DOUBLE, 0.05, -1.0)]
    kernels = kernel_plan(len(plan))
    # under each kernel: whole pairs at e / delta^2 = 0.25 and 4 (a near and a far one: the weight on a cross block), one fixed end otherwise
    for c in range(len(plan), len(kernels)):
        ratio = kernels[c][1]
        theta, sign = (0.1, 0.7)[c % 2], (1.0, -1.0)[(c // 2) % 2]
        pk = PAIR_NEAR if ratio == 0.25 else PAIR_FAR if ratio == 4.0 else PAIR_FIXED
        plan.append(pair_of(pk) + (pk, theta, sign))
    for c, ((i, j, pk, theta, sign), (kind, ratio)) in enumerate(zip(plan, kernels)):
        r = np.zeros(6) if ratio == 0.0 else tangent(rng, theta)
        qz, tz = measurement(r, mp_relative(q[i], t[i], q[j], t[j]))
        qz = sign * qz
        info = information(rng, 6)
        fi, fj = i < fp.Pf, j < fp.Pf
        rr, e, H, g, X = ref.relative_terms(q[i], t[i], q[j], t[j], qz, tz, info, fi, fj)
        delta = 0.0 if kind == ref.NONE else delta_for(e, ratio)
        rho, w = robust_outputs(kind, delta, e)
        z6, z1 = np.zeros((6, 6)), np.zeros(6)
        vals = (i, j, qz, tz, info, kind, delta, theta, ratio, pk, floats(rr), float(e), rho, w, bool(ref.relative_flip(q[i], q[j], qz)),
                ref.to_array(H[0]) if fi else z6, ref.to_array(H[1]) if fj else z6, ref.to_array(X) if fi and fj else z6,
                floats(g[0]) if fi else z1, floats(g[1]) if fj else z1)
        for k, v in zip(out, vals):
            out[k].append(v)
    return out


def position_cases(q, t, rng):
    out = {k: [] for k in ("pose", "z", "arm", "info", "kind", "delta", "ratio", "r", "e", "rho", "w", "H", "g")}
    kernels = kernel_plan(4)
    for p, (kind, ratio) in enumerate(kernels):
        arm = np.zeros(3) if p % 2 == 0 else 0.5 * rng.normal(size=3)
        r = np.zeros(3) if ratio == 0.0 else 0.5 * rng.normal(size=3)
        R, tt = ref.pose(q[p], t[p])
        z = floats(R.T * (ref.column(arm) - tt) - ref.column(r))
        info = information(rng, 3)
        rr, e, H, g = ref.position_terms(q[p], t[p], arm, z, info)
        delta = 0.0 if kind == ref.NONE else delta_for(e, ratio)
        rho, w = robust_outputs(kind, delta, e)
        for k, v in zip(out, (p, z, arm, info, kind, delta, ratio, floats(rr), float(e), rho, w, ref.to_array(H), floats(g))):
            out[k].append(v)
    return out


def landmark_cases(fp, X, rng):
    out = {k: [] for k in ("lm", "xyz", "X", "info", "kind", "delta", "ratio", "r", "e", "rho", "w", "H", "g")}
    kernels = kernel_plan(4)
    lms = rng.choice(fp.Lf, len(kernels), replace=False)
    for l, (kind, ratio) in zip(lms, kernels):
        r = np.zeros(3) if ratio == 0.0 else 0.3 * rng.normal(size=3)
        xyz = floats(ref.column(X[l]) - ref.column(r))
        info = information(rng, 3)
        rr, e, H, g = ref.landmark_terms(X[l], xyz, info)
        delta = 0.0 if kind == ref.NONE else delta_for(e, ratio)
        rho, w = robust_outputs(kind, delta, e)
        for k, v in zip(out, (int(l), xyz, X[l].copy(), info, kind, delta, ratio, floats(rr), float(e), rho, w, ref.to_array(H), floats(g))):
            out[k].append(v)
    return out


INT_NAMES = ("pose", "i", "j", "lm", "kind", "pair")


def generate():
    fp = graph()
    out = {}
    for scene in SCENES:
        q, t, X = scene_state(fp, scene)
        out[scene + "/q"], out[scene + "/t"] = q, t
        sets = {"prior": prior_cases(q, t, np.random.default_rng(11)), "relative": relative_cases(fp, q, t, np.random.default_rng(12)),
                "position": position_cases(q, t, np.random.default_rng(13)), "landmark": landmark_cases(fp, X, np.random.default_rng(14))}
        for kind, cases in sets.items():
            for name, vals in cases.items():
                out["%s/%s/%s" % (scene, kind, name)] = np.array(vals, dtype=np.int32 if name in INT_NAMES else bool if name == "flip" else np.float64)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez(PATH, **data)
    print(PATH, len(data), "arrays,", os.path.getsize(PATH), "bytes")

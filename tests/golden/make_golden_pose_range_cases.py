"""Generates tests/golden/pose_range_cases.npz: the case table of tests/test_gpu_pose_range_factor_regimes.py -- the inputs of range
factors between two poses (cuba_hip_set_pose_range_factors) on the 60-pose synthetic graph in every regime of
r = |a_j - t_j - R_j R_i^T (a_i - t_i)| - rbar, what tests/se3_mp_reference.py (mpmath, 60 digits) makes of them, and the error of the numpy
model (tests/pose_range_factor_reference.py) against that per regime, which the GPU bounds are derived from.  Data only; needs mpmath and
no GPU.  Run from the repo root: `python tests/golden/make_golden_pose_range_cases.py`.

One case per pair of free poses (case k sits on the poses 2 k and 2 k + 1; the odd cases name them as (i, j) = (2 k + 1, 2 k), so that
half of the off-diagonal blocks are stored transposed).  Pose i has a rotation of one radian about a random axis, pose j that rotation
turned by the case's RELATIVE rotation; both translations are set so that the turned cameras look at the centroid of their landmarks from
3 radii + 10 behind (every depth stays positive and the plain system small).  With a_i given, a_j = t_j + R_j w_i + rho n for a unit
vector n at 60 digits, rounded to fp64.  The plan:
  distance x rotation   rho = 1e-9 L0 ("near": the two points all but coincide, the cancellation in u), L0 ("unit") and 1e6 L0 ("far": a_j is
                        a thousand kilometres long), L0 = max(1, |a_i|, |t_i|, |t_j|) (infinity norms), each under relative rotations of
                        1e-8 (nearly identical orientations), 1, pi - 1e-6, and 1 with pose j given as -q; |r| / rho = 1e-3
  the residual          |r| / rho = 0 (rbar = rho rounded), 1e-9 (a residual far below rho) and 1 (rbar = 0 exactly) at the unit distance,
                        and 0 at the near distance
  long arms             |a_i| = 1000 L0 at rho = L0 (arms much longer than rho), relative rotations 1 and pi - 1e-6
  kernels               e / delta^2 at 0.25, 1 -+ 1e-9 and 4 under Huber and Tukey, at 1 -+ 1e-9 and 4 under Cauchy (one branch), at the
                        unit distance (delta follows from e)
The arm a_i is 0.5 times a unit vector, or (cases 1 mod 4) zero, or long.  rbar = rho (1 - ratio) at 60 digits from the ROUNDED inputs,
rounded to fp64; the expected outputs are computed from the ROUNDED numbers.

Keys: "q", "t" (the pose estimates), "pose_i", "pose_j", "range", "info", "arm_i", "arm_j", "kind", "delta" (the inputs as
HipSolver.set_pose_range_factors takes them), "theta", "sign", "distance" (-9, 0, 6: the decade of rho / L0), "rratio" (|r| / rho), "long"
(1: a long arm), "ratio" (e / delta^2; NaN without a kernel) (the prescription), the outputs "rho", "r", "e", "rhok" = rho_k(e), "w" = rho_k',
"Hii", "Hjj", "Hij" (Omega J_a^T J_b, 6 x 6) and "gi", "gj" (Omega r J^T), UNWEIGHTED, with J from central differences at 60 digits under
T <- exp(delta) T of either end, and "model_error/<regime>": the numpy model's largest error in that regime (measure:
tests/test_gpu_pose_range_factor_regimes.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import se3_mp_reference as ref  # noqa: E402
from make_golden_direction_cases import floats, looking_at_its_landmarks, unit  # noqa: E402

from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "pose_range_cases.npz")
ROTATIONS = ((1e-8, 1.0), (1.0, 1.0), (float(np.pi) - 1e-6, 1.0), (1.0, -1.0))          # (relative theta, sign of q_j)
DISTANCES = (-9, 0, 6)
RATIOS = (0.25, 1 - 1e-9, 1 + 1e-9, 4.0)
KERNELS = (ref.HUBER, ref.TUKEY, ref.CAUCHY)
NAN = float("nan")
INT_NAMES = ("pose_i", "pose_j", "kind", "distance", "long")


def graph():
    return flatten(synth_ba(60, 900, 3600, seed=2))


def distance(Ti, Tj, ai, aj):
    """rho = |a_j - t_j - R_j R_i^T (a_i - t_i)| at 60 digits"""
    u = aj - Tj[1] - Tj[0] * (Ti[0].T * (ai - Ti[1]))
    return ref.mp.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)


def pose_range_terms(qi, ti, qj, tj, arm_i, arm_j, rbar, info):
    """(rho, r, e, [H_ii, H_jj], [g_i, g_j], H_ij) of a factor at 60 digits: r = rho - rbar, J by central differences through either end's
    pose update"""
    Ti, Tj = ref.pose(qi, ti), ref.pose(qj, tj)
    ai, aj, Om = ref.column(arm_i), ref.column(arm_j), ref.matrix([[info]])
    residual = lambda A, B: ref.mp.matrix([distance(A, B, ai, aj) - ref.mpf(rbar)])  # noqa: E731
    r = residual(Ti, Tj)
    Js = ref.jacobians(residual, [Ti, Tj], [True, True])
    e, H, g, X = ref.terms(r, Js, Om)
    return distance(Ti, Tj, ai, aj), r[0], e, H, g, X


def plan():
    """per case (relative theta, sign of q_j, distance, |r| / rho, long arm, kernel kind, e / delta^2)"""
    out = [[th, sign, dist, 1e-3, 0, ref.NONE, NAN] for dist in DISTANCES for th, sign in ROTATIONS]
    out += [[1.0, 1.0, 0, rr, 0, ref.NONE, NAN] for rr in (0.0, 1e-9, 1.0)]
    out += [[1.0, 1.0, -9, 0.0, 0, ref.NONE, NAN]]
    out += [[th, 1.0, 0, 1e-3, 1, ref.NONE, NAN] for th in (1.0, float(np.pi) - 1e-6)]
    out += [[1.0, 1.0, 0, 1e-3, 0, kind, ratio] for kind in KERNELS for ratio in RATIOS if (kind, ratio) != (ref.CAUCHY, 0.25)]
    return [tuple(c) for c in out]


def cases(fp, rng):
    q = np.array(fp.q, dtype=np.float64).reshape(-1, 4)
    t = np.array(fp.t, dtype=np.float64).reshape(-1, 3)
    names = ("pose_i", "pose_j", "range", "info", "arm_i", "arm_j", "kind", "delta", "theta", "sign", "distance", "rratio", "long", "ratio", "rho", "r",
             "e", "rhok", "w", "Hii", "Hjj", "Hij", "gi", "gj")
    out = {k: [] for k in names}
    P = plan()
    assert 2 * len(P) <= fp.Pf
    for k, (theta, sign, dist, rratio, long_arm, kind, ratio) in enumerate(P):
        i, j = (2 * k, 2 * k + 1) if k % 2 == 0 else (2 * k + 1, 2 * k)
        qi = ref.quat_exp([ref.mpf(x) for x in unit(rng)])
        qj = ref.quat_mul(ref.quat_exp([ref.mpf(theta) * ref.mpf(x) for x in unit(rng)]), qi)
        q[i], q[j] = floats(qi), sign * floats(qj)
        t[i], t[j] = looking_at_its_landmarks(fp, i, q[i]), looking_at_its_landmarks(fp, j, q[j])
        L0 = max(1.0, float(np.abs(t[i]).max()), float(np.abs(t[j]).max()))
        arm_i = 1000.0 * L0 * unit(rng) if long_arm else np.zeros(3) if k % 4 == 1 else 0.5 * unit(rng)
        Ti, Tj = ref.pose(q[i], t[i]), ref.pose(q[j], t[j])
        n = ref.column(unit(rng))
        w = Ti[0].T * (ref.column(arm_i) - Ti[1])
        arm_j = floats(Tj[1] + Tj[0] * w + ref.mpf(10.0 ** dist * L0) * n)
        rho = distance(Ti, Tj, ref.column(arm_i), ref.column(arm_j))          # (of the ROUNDED arm)
        rbar = 0.0 if rratio == 1.0 else float(rho * (1 - ref.mpf(rratio)))
        info = 1000.0 * (1.0 + float(rng.uniform()))
        rho, r, e, H, g, X = pose_range_terms(q[i], t[i], q[j], t[j], arm_i, arm_j, rbar, info)
        delta = 0.0 if kind == ref.NONE else float(ref.mp.sqrt(e / ref.mpf(ratio)))
        vals = (i, j, rbar, info, arm_i, arm_j, kind, delta, theta, sign, dist, rratio, long_arm, ratio, float(rho), float(r), float(e),
                float(ref.rho(kind, delta, e)), float(ref.weight(kind, delta, e)), ref.to_array(H[0]), ref.to_array(H[1]), ref.to_array(X),
                floats(g[0]), floats(g[1]))
        for name, x in zip(out, vals):
            out[name].append(x)
    return q, t, out


def generate():
    fp = graph()
    q, t, sets = cases(fp, np.random.default_rng(23))
    out = {"q": q, "t": t}
    for name, vals in sets.items():
        out[name] = np.array(vals, dtype=np.int32 if name in INT_NAMES else np.float64)
    import test_gpu_pose_range_factor_regimes as tg
    for reg, err in tg.model_errors(out).items():
        out["model_error/" + reg] = np.float64(err)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez(PATH, **data)
    print(PATH, len(data), "arrays,", os.path.getsize(PATH), "bytes")
    for k in sorted(data):
        if k.startswith("model_error/"):
            print("%-28s %.3g" % (k, float(data[k])))

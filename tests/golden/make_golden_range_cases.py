"""Generates tests/golden/range_cases.npz: the case table of tests/test_gpu_range_factor_regimes.py -- the inputs of range factors
(cuba_hip_set_range_factors) on the 60-pose synthetic graph in every regime of r = |a - t - R b| - rbar, what tests/se3_mp_reference.py
(mpmath, 60 digits) makes of them, and the error of the numpy model (tests/range_factor_reference.py) against that per regime, which the
GPU bounds are derived from.  Data only; needs mpmath and no GPU.  Run from the repo root:
`python tests/golden/make_golden_range_cases.py`.

One case per free pose (case k sits on pose k): the product of
  the pose's rotation   R = exp(theta n) with theta = 1e-8, 1 and pi - 1e-6, and theta = 1 with the estimate given as -q (the quaternion at
                        60 digits, rounded to fp64; the translation is set so that the turned camera looks at the centroid of its landmarks
                        from 3 radii + 10 behind: every depth stays positive and the plain system small);
  the distance          "near": rho = 1e-6 L0, the cancellation in a - t - R b (L0 = max(1, |a|, |t|), infinity norms); "unit": rho = L0;
                        "far": rho = 1e6 L0, an anchor a thousand kilometres off.  The anchor is b = R^T (a - t - rho n) for a unit vector n,
                        at 60 digits, rounded to fp64;
  the residual          |r| / rho = 0 (rbar = rho rounded), 1e-9, 1e-3 and 1 (rbar = 0 exactly): rbar = rho (1 - ratio) at 60 digits from the
                        ROUNDED inputs, rounded to fp64.
The lever arm is 0.5 times a unit vector, or (cases 1 mod 4) zero.  Eighteen of the cases carry a robust kernel: e / delta^2 at 0.25,
1 -+ 1e-9, 4 and 1e6 under Huber, Tukey and Cauchy on the well-conditioned cases (unit and far, |r| / rho of 1e-3 and 1: delta follows
from the case's e), and e / delta^2 = 0 on three zero-residual cases of the unit distance (delta = 1).  Without kernels (the kernels'
ROBUST = false instantiations) every case is a regime case.  The expected outputs are computed from the ROUNDED numbers.

Keys: "q", "t" (the pose estimates), "pose", "anchor", "range", "info", "arm", "kind", "delta" (the inputs as HipSolver.set_range_factors
takes them), "theta", "sign", "distance" (-6, 0, 6: the decade of rho / L0), "rratio" (|r| / rho), "ratio" (e / delta^2; NaN without a kernel)
(the prescription), the outputs "rho", "r", "e", "rhok" = rho_k(e), "w" = rho_k', "H" (Omega J^T J, 6 x 6) and "g" (Omega r J^T), UNWEIGHTED,
with J from central differences at 60 digits under T <- exp(delta) T, and "model_error/<regime>": the numpy model's largest error in that
regime (measure: tests/test_gpu_range_factor_regimes.py)."""
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

PATH = os.path.join(HERE, "range_cases.npz")
ROTATIONS = ((1e-8, 1.0), (1.0, 1.0), (float(np.pi) - 1e-6, 1.0), (1.0, -1.0))          # (theta, sign of q)
DISTANCES = (-6, 0, 6)
RRATIOS = (0.0, 1e-9, 1e-3, 1.0)
RATIOS = (0.25, 1 - 1e-9, 1 + 1e-9, 4.0, 1e6)
KERNELS = (ref.HUBER, ref.TUKEY, ref.CAUCHY)
NAN = float("nan")
INT_NAMES = ("pose", "kind", "distance")


def graph():
    return flatten(synth_ba(60, 900, 3600, seed=2))


def distance(T, a, b):
    """rho = |a - t - R b| at 60 digits"""
    u = a - T[1] - T[0] * b
    return ref.mp.sqrt(u[0] ** 2 + u[1] ** 2 + u[2] ** 2)


def range_terms(q, t, arm, anchor, rbar, info):
    """(rho, r, e, H, g) of a factor at the pose (q, t), at 60 digits: r = rho - rbar, J by central differences through the pose update"""
    T = ref.pose(q, t)
    a, b, Om = ref.column(arm), ref.column(anchor), ref.matrix([[info]])
    residual = lambda P: ref.mp.matrix([distance(P, a, b) - ref.mpf(rbar)])  # noqa: E731
    r = residual(T)
    J, = ref.jacobians(residual, [T], [True])
    e, H, g, _ = ref.terms(r, [J], Om)
    return distance(T, a, b), r[0], e, H[0], g[0]


def plan():
    """per case (theta, sign of q, distance, |r| / rho, kernel kind, e / delta^2)"""
    out = [[th, sign, dist, rr, ref.NONE, NAN] for th, sign in ROTATIONS for dist in DISTANCES for rr in RRATIOS]
    well = [k for k, c in enumerate(out) if c[2] in (0, 6) and c[3] in (1e-3, 1.0)]
    zero = [k for k, c in enumerate(out) if c[2] == 0 and c[3] == 0.0]
    pairs = [(kind, ratio) for kind in KERNELS for ratio in RATIOS]
    assert len(well) >= len(pairs) and len(zero) >= len(KERNELS)
    for k, (kind, ratio) in zip(well, pairs):
        out[k][4:] = [kind, ratio]
    for k, kind in zip(zero, KERNELS):
        out[k][4:] = [kind, 0.0]
    return [tuple(c) for c in out]


def cases(fp, rng):
    q = np.array(fp.q, dtype=np.float64).reshape(-1, 4)
    t = np.array(fp.t, dtype=np.float64).reshape(-1, 3)
    names = ("pose", "anchor", "range", "info", "arm", "kind", "delta", "theta", "sign", "distance", "rratio", "ratio", "rho", "r", "e", "rhok", "w", "H", "g")
    out = {k: [] for k in names}
    P = plan()
    assert len(P) <= fp.Pf
    for p, (theta, sign, dist, rratio, kind, ratio) in enumerate(P):
        q[p] = sign * floats(ref.quat_exp([ref.mpf(theta) * ref.mpf(x) for x in unit(rng)]))
        t[p] = looking_at_its_landmarks(fp, p, q[p])
        arm = np.zeros(3) if p % 4 == 1 else 0.5 * unit(rng)
        L0 = max(1.0, float(np.abs(arm).max()), float(np.abs(t[p]).max()))
        T = ref.pose(q[p], t[p])
        n = ref.column(unit(rng))
        anchor = floats(T[0].T * (ref.column(arm) - T[1] - ref.mpf(10.0 ** dist * L0) * n))
        rho = distance(T, ref.column(arm), ref.column(anchor))          # (of the ROUNDED anchor)
        rbar = 0.0 if rratio == 1.0 else float(rho * (1 - ref.mpf(rratio)))
        info = 1000.0 * (1.0 + float(rng.uniform()))
        rho, r, e, H, g = range_terms(q[p], t[p], arm, anchor, rbar, info)
        delta = 0.0 if kind == ref.NONE else 1.0 if ratio == 0.0 else float(ref.mp.sqrt(e / ref.mpf(ratio)))
        vals = (p, anchor, rbar, info, arm, kind, delta, theta, sign, dist, rratio, ratio, float(rho), float(r), float(e),
                float(ref.rho(kind, delta, e)), float(ref.weight(kind, delta, e)), ref.to_array(H), floats(g))
        for k, x in zip(out, vals):
            out[k].append(x)
    return q, t, out


def generate():
    fp = graph()
    q, t, sets = cases(fp, np.random.default_rng(22))
    out = {"q": q, "t": t}
    for name, vals in sets.items():
        out[name] = np.array(vals, dtype=np.int32 if name in INT_NAMES else np.float64)
    import test_gpu_range_factor_regimes as tg
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

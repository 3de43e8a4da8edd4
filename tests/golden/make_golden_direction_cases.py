"""Generates tests/golden/direction_cases.npz: the case table of tests/test_gpu_direction_factor_regimes.py -- the inputs of direction
factors (cuba_hip_set_direction_factors) on the 60-pose synthetic graph in every regime of r = R d - m, what tests/se3_mp_reference.py
(mpmath, 60 digits) makes of them, and the error of the numpy model (tests/direction_factor_reference.py) against that per regime, which
the GPU bounds are derived from.  Data only; needs mpmath and no GPU.  Run from the repo root:
`python tests/golden/make_golden_direction_cases.py`.

One case per free pose (case k sits on pose k).  The REGIME cases prescribe the pose's rotation, R = exp(theta a) with theta = 1e-8, 1 and
pi - 1e-6 (the quaternion at 60 digits, rounded to fp64; the translation, which no direction factor reads, is set so that the turned
camera looks at the centroid of its landmarks from 3 radii + 10 behind: every depth stays positive and the plain system small), the size of the residual, |r| = 1e-8, 0.1 and 2
(m = R d - r at 60 digits, rounded; |r| = 2: r = 2 R d, so m = -R d), and the information, full rank or the rank-2 P Omega P with
P = I - m m^T / |m|^2; two more give the estimate as -q.  The KERNEL cases keep the synthesised rotation, |r| = 0.1, and put
e / delta^2 at 0 (a zero residual: m = R d rounded), 0.25, 1 -+ 1e-9, 4 and 1e6 under Huber, Tukey and Cauchy.  d is a unit vector
rounded to fp64, or (cases 1 mod 4) 9.81 times one; the expected outputs are computed from the ROUNDED numbers.

Keys: "q", "t" (the pose estimates), "pose", "d", "m", "info", "kind", "delta" (the inputs as HipSolver.set_direction_factors takes
them), "theta", "rnorm", "rank2", "ratio" (the prescription; NaN where it does not apply), the outputs "r", "e", "rho", "w" = rho', "H"
(J^T Omega J, 6 x 6) and "g" (J^T Omega r), UNWEIGHTED, with J from central differences at 60 digits under T <- exp(delta) T, and
"model_error/<regime>": the numpy model's largest error in that regime (measure: tests/test_gpu_direction_factor_regimes.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import se3_mp_reference as ref  # noqa: E402

from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PATH = os.path.join(HERE, "direction_cases.npz")
THETAS = (1e-8, 1.0, float(np.pi) - 1e-6)
RNORMS = (1e-8, 0.1, 2.0)
RATIOS = (0.0, 0.25, 1 - 1e-9, 1 + 1e-9, 4.0, 1e6)
KERNELS = (ref.HUBER, ref.TUKEY, ref.CAUCHY)
NAN = float("nan")
INT_NAMES = ("pose", "kind")


def graph():
    return flatten(synth_ba(60, 900, 3600, seed=2))


def norm(v):
    s = 0.0
    for x in v:
        s += float(x) * float(x)
    return s ** 0.5


def unit(rng):
    v = rng.normal(size=3)
    return v / norm(v)


def floats(v):
    return np.array([float(x) for x in v])


def information(rng, scale=1000.0):
    """scale (I + A A^T / 12) as explicit sums in index order (the table must not depend on a BLAS), symmetric by construction"""
    A = rng.normal(size=(3, 3))
    M = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            s = 0.0
            for k in range(3):
                s += float(A[i, k]) * float(A[j, k])
            M[i, j] = M[j, i] = s
    return scale * (np.eye(3) + 0.25 / 3 * M)


def projected(Om, m):
    """P Omega P, P = I - m m^T / |m|^2, in fp64 by explicit sums, symmetrised: the rank-2 information as a caller would compute it"""
    n2 = 0.0
    for x in m:
        n2 += float(x) * float(x)
    P = [[(1.0 if i == j else 0.0) - float(m[i]) * float(m[j]) / n2 for j in range(3)] for i in range(3)]
    out = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            s = 0.0
            for a in range(3):
                for b in range(3):
                    s += P[i][a] * float(Om[a, b]) * P[b][j]
            out[i, j] = s
    return 0.5 * (out + out.T)


def direction_terms(q, d, m, info):
    """(r, e, H, g) of a factor at the rotation of q, at 60 digits: r = R d - m, J by central differences through the pose update"""
    T = ref.pose(q, [0.0, 0.0, 0.0])
    dd, mm, Om = ref.column(d), ref.column(m), ref.matrix(info)
    residual = lambda P: P[0] * dd - mm  # noqa: E731
    r = residual(T)
    J, = ref.jacobians(residual, [T], [True])
    e, H, g, _ = ref.terms(r, [J], Om)
    return r, e, H[0], g[0]


def plan():
    """per case (theta or NaN, sign of q, |r|, rank2, kernel kind, ratio)"""
    out = [(th, 1.0, rn, rank2, ref.NONE, NAN) for th in THETAS for rn in RNORMS for rank2 in (False, True)]
    out += [(1.0, -1.0, 0.1, False, ref.NONE, NAN), (1.0, -1.0, 0.1, True, ref.NONE, NAN)]
    for x, (kind, ratio) in enumerate((k, r) for k in KERNELS for r in RATIOS):
        out.append((NAN, 1.0, 0.0 if ratio == 0.0 else 0.1, x % 2 == 1, kind, ratio))
    return out


def quat_to_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def looking_at_its_landmarks(fp, p, q):
    """t of pose p with the rotation of q such that the camera centre lies 3 radii + 10 behind the centroid of the landmarks the pose
    observes, on the optical axis"""
    X = np.asarray(fp.Xw, dtype=np.float64).reshape(-1, 3)[np.unique(np.asarray(fp.eL)[np.asarray(fp.eP) == p])]
    c = X.mean(axis=0)
    radius = float(np.sqrt(((X - c) ** 2).sum(axis=1)).max())
    R = quat_to_rot(q)
    centre = c - (3.0 * radius + 10.0) * R[2]          # (R[2] = R^T e_z: the optical axis in the world)
    return -np.array([R[i][0] * centre[0] + R[i][1] * centre[1] + R[i][2] * centre[2] for i in range(3)])      # (explicit sums: no BLAS)


def cases(fp, rng):
    q = np.array(fp.q, dtype=np.float64).reshape(-1, 4)
    t = np.array(fp.t, dtype=np.float64).reshape(-1, 3)
    names = ("pose", "d", "m", "info", "kind", "delta", "theta", "rnorm", "rank2", "ratio", "r", "e", "rho", "w", "H", "g")
    out = {k: [] for k in names}
    P = plan()
    assert len(P) <= fp.Pf
    for p, (theta, sign, rnorm, rank2, kind, ratio) in enumerate(P):
        if theta == theta:          # a prescribed rotation
            q[p] = sign * floats(ref.quat_exp([ref.mpf(theta) * ref.mpf(x) for x in unit(rng)]))
            t[p] = looking_at_its_landmarks(fp, p, q[p])
        d = unit(rng) * (9.81 if p % 4 == 1 else 1.0)
        R = ref.quat_rot(ref.quat_unit([ref.mpf(x) for x in q[p]]))
        v = R * ref.column(d)
        if rnorm == 2.0:
            r = 2 * v
        else:
            r = ref.column(rnorm * unit(rng))
        m = floats(v - r)
        info = information(rng)
        if rank2:
            info = projected(info, m)
        rr, e, H, g = direction_terms(q[p], d, m, info)
        delta = 0.0 if kind == ref.NONE else 1.0 if ratio == 0.0 else float(ref.mp.sqrt(e / ref.mpf(ratio)))
        vals = (p, d, m, info, kind, delta, theta, rnorm, rank2, ratio, floats(rr), float(e), float(ref.rho(kind, delta, e)),
                float(ref.weight(kind, delta, e)), ref.to_array(H), floats(g))
        for k, x in zip(out, vals):
            out[k].append(x)
    return q, t, out


def generate():
    fp = graph()
    q, t, sets = cases(fp, np.random.default_rng(21))
    out = {"q": q, "t": t}
    for name, vals in sets.items():
        out[name] = np.array(vals, dtype=np.int32 if name in INT_NAMES else bool if name == "rank2" else np.float64)
    import test_gpu_direction_factor_regimes as tg
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

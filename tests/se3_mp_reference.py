"""60-digit mpmath reference of the factors on poses and landmarks (pose priors, relative-pose edges, position factors, landmark priors and
their robust kernels) -- TEST INFRASTRUCTURE, used on the CPU only: tests/golden/make_golden_se3_cases.py evaluates it into
tests/golden/se3_cases.npz, and the GPU tests read that file, never this module.

It is a function of the fp64 numbers exactly as they are handed to the library: every input is converted to a 60-digit mpf (exactly)
before any arithmetic, a measured quaternion is first normalised in fp64 the way the library's take_factor_values does, and every output is
rounded to fp64 once, at the end.  It shares no formula with the kernels or with the numpy models (prior_reference.py and its siblings)
beyond the definitions:

    exp([w, u]) = [exp(w) | V(w) u]                     Rodrigues' formula and V = I + (1 - cos th) / th^2 W + (th - sin th) / th^3 W^2
                                                        (the coefficients in forms free of cancellation: the steps have th = 1e-25)
    log([R | t]) = [w, V(w)^-1 t]                       th = atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), w = th * axis; V u = t by LU
    prior:     r = log(T Tbar^-1)                       relative edge:  r = log(T_j T_i^-1 Zbar^-1)
    position:  r = R^T (a - t) - z                      landmark prior: r = X - Xbar

The Jacobians with respect to every free end are central differences with h = 1e-25 under the solver's update T <- exp(d) T, d in
[omega, upsilon] order (truncation h^2 = 1e-50 times a third derivative, rounding 1e-60 / h = 1e-35): no J_l^-1, no Q(w, u), no Ad appears.
(mp.logm on the 4 x 4 matrix is avoided on purpose: differenced near th = pi it is wrong by O(1).)  From r and the Jacobians:
e = r^T Omega r, H_ab = J_a^T Omega J_b, g_a = J_a^T Omega r, and rho(e), rho'(e) of the kernels none / Huber / Tukey / Cauchy."""
import mpmath

mp = mpmath.ctx_mp.MPContext()          # a context of its own: mpmath's global precision is left alone
mp.dps = 60

NONE, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3
STEP = mp.mpf(10) ** -25
TINY = mp.mpf(10) ** -40


def mpf(x):
    """an fp64 number -> the same number at 60 digits"""
    return mp.mpf(float(x))


def column(v):
    return mp.matrix([mpf(x) for x in v])


def matrix(M):
    return mp.matrix([[mpf(x) for x in row] for row in M])


def hat(w):
    return mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


# ---- quaternions (x, y, z, w) ------------------------------------------------------------------------------------------------------------
def library_unit(q):
    """q / |q| in fp64 as the library normalises a measured quaternion (sum of squares in index order, sqrt, four divisions)"""
    q = [float(x) for x in q]
    s = 0.0
    for x in q:
        s += x * x
    n = s ** 0.5
    return [x / n for x in q]


def quat_unit(q):
    q = [mp.mpf(x) for x in q]
    n = mp.sqrt(sum(x * x for x in q))
    return [x / n for x in q]


def quat_mul(a, b):
    return [a[3] * b[0] + b[3] * a[0] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + b[3] * a[1] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + b[3] * a[2] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def quat_conj(q):
    return [-q[0], -q[1], -q[2], q[3]]


def quat_exp(w):
    """the unit quaternion of the rotation vector w"""
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    if th == 0:
        return [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)]
    s = mp.sin(th / 2) / th
    return [s * w[0], s * w[1], s * w[2], mp.cos(th / 2)]


def quat_rot(q):
    """rotation matrix of a unit quaternion"""
    x, y, z, w = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- SE(3) as (R, t) ---------------------------------------------------------------------------------------------------------------------
def pose(q, t):
    """the pose of fp64 numbers (q, t): the rotation of q / |q| (the kernels normalise what they compose) and t"""
    return quat_rot(quat_unit([mpf(x) for x in q])), column(t)


def measured_pose(q, t):
    """a measurement as the library keeps it: the quaternion normalised in fp64 first"""
    return pose(library_unit(q), t)


def compose(a, b):
    return a[0] * b[0], a[0] * b[1] + a[1]


def inverse(a):
    Rt = a[0].T
    return Rt, -(Rt * a[1])


def rodrigues_coefficients(th):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3) without cancellation: the half-angle form of 1 - cos, and the Taylor series
    of th - sin th below 1e-3 (13 terms: truncation < 1e-75)"""
    if th == 0:
        return mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6
    a = mp.sin(th) / th
    b = 2 * (mp.sin(th / 2) / th) ** 2
    if th < mp.mpf(10) ** -3:
        c, term = mp.mpf(0), mp.mpf(1) / 6
        for k in range(13):
            c += term
            term *= -th * th / ((2 * k + 4) * (2 * k + 5))
    else:
        c = (th - mp.sin(th)) / th ** 3
    return a, b, c


def V_of(w):
    W = hat(w)
    _, b, c = rodrigues_coefficients(mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2))
    return mp.eye(3) + b * W + c * W * W


def exp6(d):
    w = [mp.mpf(x) for x in d[:3]]
    u = mp.matrix([mp.mpf(x) for x in d[3:]])
    W = hat(w)
    a, b, c = rodrigues_coefficients(mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2))
    return mp.eye(3) + a * W + b * W * W, (mp.eye(3) + b * W + c * W * W) * u


def log6(T):
    R, t = T
    v = [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2]
    s = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    f = mp.mpf(1) if s < TINY else mp.atan2(s, c) / s
    w = [f * x for x in v]
    u = mp.lu_solve(V_of(w), t)
    return mp.matrix([w[0], w[1], w[2], u[0], u[1], u[2]])


# ---- residuals ---------------------------------------------------------------------------------------------------------------------------
def prior_residual(T, Tbar):
    return log6(compose(T, inverse(Tbar)))


def relative_residual(Ti, Tj, Z):
    return log6(compose(compose(Tj, inverse(Ti)), inverse(Z)))


def position_residual(T, a, z):
    return T[0].T * (a - T[1]) - z


_steps = {}


def _step(k, sign):
    if (k, sign) not in _steps:
        d = [mp.mpf(0)] * 6
        d[k] = sign * STEP
        _steps[(k, sign)] = exp6(d)
    return _steps[(k, sign)]


def jacobians(residual, poses, free):
    """d residual(poses) / d d_e for every end e with free[e], under T_e <- exp(d_e) T_e: central differences, one m x 6 matrix per end (None
    for an end that is not free)"""
    out = []
    for e, T in enumerate(poses):
        if not free[e]:
            out.append(None)
            continue
        cols = []
        for k in range(6):
            hi = residual(*[compose(_step(k, 1), P) if x == e else P for x, P in enumerate(poses)])
            lo = residual(*[compose(_step(k, -1), P) if x == e else P for x, P in enumerate(poses)])
            cols.append((hi - lo) / (2 * STEP))
        J = mp.matrix(len(cols[0]), 6)
        for k in range(6):
            for i in range(len(cols[0])):
                J[i, k] = cols[k][i]
        out.append(J)
    return out


# ---- robust kernels ----------------------------------------------------------------------------------------------------------------------
def rho(kind, delta, e):
    d2 = mpf(delta) ** 2
    if kind == HUBER:
        return e if e <= d2 else 2 * mp.sqrt(e) * mpf(delta) - d2
    if kind == TUKEY:
        return d2 / 3 * (1 - (1 - e / d2) ** 3) if e <= d2 else d2 / 3
    if kind == CAUCHY:
        return d2 * mp.log1p(e / d2)
    return e


def weight(kind, delta, e):
    d2 = mpf(delta) ** 2
    if kind == HUBER:
        return mp.mpf(1) if e <= d2 else mpf(delta) / mp.sqrt(e)
    if kind == TUKEY:
        return (1 - e / d2) ** 2 if e <= d2 else mp.mpf(0)
    if kind == CAUCHY:
        return 1 / (1 + e / d2)
    return mp.mpf(1)


# ---- a factor's terms --------------------------------------------------------------------------------------------------------------------
def to_array(M):
    import numpy as np
    return np.array([[float(M[i, j]) for j in range(M.cols)] for i in range(M.rows)])


def terms(r, Js, Om):
    """(e, [H_aa], [g_a], H_01 or None) at 60 digits: e = r^T Omega r, H_ab = J_a^T Omega J_b, g_a = J_a^T Omega r"""
    Or = Om * r
    e = (r.T * Or)[0]
    H = [None if J is None else J.T * Om * J for J in Js]
    g = [None if J is None else J.T * Or for J in Js]
    X = Js[0].T * Om * Js[1] if len(Js) == 2 and Js[0] is not None and Js[1] is not None else None
    return e, H, g, X


def prior_terms(q, t, qb, tb, info):
    """a pose prior at the state (q, t): (r, e, H, g) with r, H, g still at 60 digits"""
    T, Tb, Om = pose(q, t), measured_pose(qb, tb), matrix(info)
    r = prior_residual(T, Tb)
    J, = jacobians(lambda P: prior_residual(P, Tb), [T], [True])
    e, H, g, _ = terms(r, [J], Om)
    return r, e, H[0], g[0]


def relative_terms(qi, ti, qj, tj, qz, tz, info, free_i=True, free_j=True):
    """a relative-pose edge: (r, e, [H_ii, H_jj], [g_i, g_j], H_ij = J_i^T Omega J_j); the entries of a fixed end are None"""
    Ti, Tj, Z, Om = pose(qi, ti), pose(qj, tj), measured_pose(qz, tz), matrix(info)
    r = relative_residual(Ti, Tj, Z)
    Js = jacobians(lambda A, B: relative_residual(A, B, Z), [Ti, Tj], [free_i, free_j])
    e, H, g, X = terms(r, Js, Om)
    return r, e, H, g, X


def position_terms(q, t, arm, z, info):
    T, a, zz, Om = pose(q, t), column(arm), column(z), matrix(info)
    r = position_residual(T, a, zz)
    J, = jacobians(lambda P: position_residual(P, a, zz), [T], [True])
    e, H, g, _ = terms(r, [J], Om)
    return r, e, H[0], g[0]


def landmark_terms(X, xbar, info):
    """a landmark prior: r = X - Xbar, J = I under X <- X + d"""
    Om = matrix(info)
    r = column(X) - column(xbar)
    e, H, g, _ = terms(r, [mp.eye(3)], Om)
    return r, e, H[0], g[0]


def relative_flip(qi, qj, qz):
    """the sign of the scalar part of q_j (x) conj(q_z (x) q_i), the relative quaternion the kernel takes the logarithm of"""
    qb = quat_mul([mpf(x) for x in library_unit(qz)], [mpf(x) for x in qi])
    return sum(mpf(a) * b for a, b in zip(qj, qb)) < 0


def prior_flip(q, qb):
    return sum(mpf(a) * mpf(b) for a, b in zip(q, library_unit(qb))) < 0

"""Reference for pose refinement with the landmarks held (cuba_hip_refine_poses), fp64 on a FlatProblem and a state, and a 60-digit mpmath
twin of its numeric steps that takes its own accept / reject decisions.

The definition (include/cuba_hip.h), per free selected pose p, over its reprojection edges of live information omega > 0:
  classification at the start of round k = 0 ... rounds - 1 and once more behind the last round, at the pose's then-current value: an edge
      is in iff omega > 0 and depth > 0 and (k > 0 or final) omega |r|^2 <= chi2_max[stereo]; an edge that was out can come back.
      FEW_OBSERVATIONS: fewer than 3 in at round 0.  FEW_INLIERS: fewer than max(3, min_inliers) in later or at the end.
  one round: lambda = 1e-5 max_k H_kk at the first linearisation, nu = 2, then `iterations` trials (a fixed count):
      H = sum w' J^T J, b = sum w' J^T r, F = sum rho(omega |r|^2), r = proj - meas, J = -d r / d [omega; upsilon] for T <- exp([omega; upsilon]) T,
      w' = omega rho'(omega |r|^2), rho = the robust kernels in the rounds below robust_rounds, the identity later;
      (H + lambda I) d = b by LDL^T (a non-positive pivot or a non-finite number: SINGULAR); T' = exp(d) T; rejected if an edge of the round
      has depth <= 0 at T' or F' is not finite; else gain = (F - F') / (d^T (lambda d + b)); gain > 0: accept,
      lambda *= max(1/3, 1 - (2 gain - 1)^3), nu = 2; else lambda *= nu, nu *= 2.
Every sum runs over the pose's edges sorted by landmark, front to back."""
import numpy as np

OK, NOT_SELECTED, FIXED, FEW_OBSERVATIONS, SINGULAR, FEW_INLIERS = range(6)
STATUS_NAMES = ("ok", "not_selected", "fixed", "few_observations", "singular", "few_inliers")
CHI2_MONO, CHI2_STEREO = 5.991, 7.815


class Arith:
    """the arithmetic the numeric steps run in: python floats (fp64) ..."""
    num = staticmethod(float)
    sqrt = staticmethod(lambda x: float(np.sqrt(x)))
    sin = staticmethod(lambda x: float(np.sin(x)))
    cos = staticmethod(lambda x: float(np.cos(x)))
    finite = staticmethod(lambda x: bool(np.isfinite(x)))


class ArithMp:
    """... or mpmath numbers (the caller sets the working precision: mpmath.workdps(60))"""
    @staticmethod
    def num(x):
        import mpmath
        return mpmath.mpf(x) if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x))

    @staticmethod
    def sqrt(x):
        import mpmath
        return mpmath.sqrt(x)

    @staticmethod
    def sin(x):
        import mpmath
        return mpmath.sin(x)

    @staticmethod
    def cos(x):
        import mpmath
        return mpmath.cos(x)

    @staticmethod
    def finite(x):
        import mpmath
        return bool(mpmath.isfinite(x))


def float_rounded(fp, state=None):
    """(FlatProblem, state) with everything the fp32 library holds as float rounded to float"""
    import copy
    r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # noqa: E731
    out = copy.copy(fp)
    out.q, out.t, out.Xw, out.cam, out.meas, out.omega = r(fp.q), r(fp.t), r(fp.Xw), r(fp.cam), r(fp.meas), r(fp.omega)
    return out, (None if state is None else tuple(r(a) for a in state))


def float_rounded_kernels(rk):
    return tuple((int(k), float(np.float32(d))) for k, d in rk)


def pose_edges(fp):
    """per pose its edge ids, sorted by landmark (stable)"""
    order = np.lexsort((fp.eL, fp.eP))
    ptr = np.zeros(fp.Pt + 1, dtype=np.int64)
    np.cumsum(np.bincount(fp.eP, minlength=fp.Pt), out=ptr[1:])
    return [[int(e) for e in order[ptr[p]:ptr[p + 1]]] for p in range(fp.Pt)]


def rotation(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def quat_rotate(q, v):
    a = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    a = [2 * x for x in a]
    return [v[0] + q[3] * a[0] + (q[1] * a[2] - q[2] * a[1]), v[1] + q[3] * a[1] + (q[2] * a[0] - q[0] * a[2]),
            v[2] + q[3] * a[2] + (q[0] * a[1] - q[1] * a[0])]


def exp_update(upd, q, t, ar):
    """T <- exp([omega; upsilon]) T: (q', t'), the steps of pose_exp_update (csrc/ba_math.hpp)"""
    one, zero = ar.num(1.0), ar.num(0.0)
    wx, wy, wz = upd[0], upd[1], upd[2]
    theta = ar.sqrt(wx * wx + wy * wy + wz * wz)
    if theta < 0.00001:
        a1, a2, a3 = one, one / 2, one / 6
    else:
        sn, cs = ar.sin(theta), ar.cos(theta)
        a1, a2, a3 = sn / theta, (1 - cs) / (theta * theta), (theta - sn) / (theta * theta * theta)
    xx, yy, zz, xy, yz, zx = wx * wx, wy * wy, wz * wz, wx * wy, wy * wz, wz * wx
    K = [[zero, -wz, wy], [wz, zero, -wx], [-wy, wx, zero]]
    K2 = [[-yy - zz, xy, zx], [xy, -zz - xx, yz], [zx, yz, -xx - yy]]
    R = [[(one if i == j else zero) + a1 * K[i][j] + a2 * K2[i][j] for j in range(3)] for i in range(3)]
    te = [sum(((one if i == j else zero) + a2 * K[i][j] + a3 * K2[i][j]) * upd[3 + j] for j in range(3)) for i in range(3)]
    qe = [zero] * 4
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        tr = ar.sqrt(tr + 1)
        qe[3] = tr / 2
        tr = one / 2 / tr
        qe[0], qe[1], qe[2] = (R[2][1] - R[1][2]) * tr, (R[0][2] - R[2][0]) * tr, (R[1][0] - R[0][1]) * tr
    else:
        c1 = R[1][1] > R[0][0]
        c2 = R[2][2] > (R[1][1] if c1 else R[0][0])
        i = 2 if c2 else 1 if c1 else 0
        j, k = (i + 1) % 3, (i + 2) % 3
        tr = ar.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
        qe[i] = tr / 2
        tr = one / 2 / tr
        qe[3], qe[j], qe[k] = (R[k][j] - R[j][k]) * tr, (R[j][i] + R[i][j]) * tr, (R[k][i] + R[i][k]) * tr
    u = quat_rotate(qe, t)
    t2 = [te[i] + u[i] for i in range(3)]
    c = [qe[3] * q[0] + qe[0] * q[3] + qe[1] * q[2] - qe[2] * q[1],
         qe[3] * q[1] + qe[1] * q[3] + qe[2] * q[0] - qe[0] * q[2],
         qe[3] * q[2] + qe[2] * q[3] + qe[0] * q[1] - qe[1] * q[0],
         qe[3] * q[3] - qe[0] * q[0] - qe[1] * q[1] - qe[2] * q[2]]
    invn = 1 / ar.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3])
    if c[3] < 0:
        invn = -invn
    return [invn * v for v in c], t2


def robust(kind, delta, e, ar):
    """(rho(e), rho'(e)) (robust_rho / robust_weight of csrc/ba_math.hpp)"""
    d2 = delta * delta
    if kind == 1 and not e <= d2:
        s = ar.sqrt(e)
        return 2 * s * delta - d2, delta / s
    if kind == 2:
        u, top = 1 - e / d2, d2 / 3
        return (top * (1 - u * u * u), u * u) if e <= d2 else (top, ar.num(0.0))
    return e, ar.num(1.0)


def edge_residual(ed, R, t, ar):
    """(Xc, r = proj - meas, omega |r|^2) of an edge (X, cam, meas, omega, stereo) at the pose (R, t); None for a depth of exactly 0"""
    X, cam, m, w, stereo = ed
    Xc = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]
    if Xc[2] == 0:
        return Xc, None, None
    invZ = 1 / Xc[2]
    u = cam[0] * invZ * Xc[0] + cam[2]
    v = cam[1] * invZ * Xc[1] + cam[3]
    r = [u - m[0], v - m[1], (u - cam[4] * invZ) - m[2] if stereo else ar.num(0.0)]
    return Xc, r, w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2])


def pose_jacobian(ed, Xc, ar):
    """J = -d r / d [omega; upsilon], 3 x 6 (row 2 zero for a monocular edge): the pose half of edge_jacobians (csrc/ba_math.hpp)"""
    _, cam, _, _, stereo = ed
    X, Y = Xc[0], Xc[1]
    invZ = 1 / Xc[2]
    invZZ = invZ * invZ
    fu, fv = cam[0], cam[1]
    zero = ar.num(0.0)
    bf, s = (cam[4], ar.num(1.0)) if stereo else (zero, zero)
    J0 = [X * Y * invZZ * fu, -(1 + (X * X * invZZ)) * fu, Y * invZ * fu, -invZ * fu, zero, X * invZZ * fu]
    J1 = [(1 + Y * Y * invZZ) * fv, -X * Y * invZZ * fv, -X * invZ * fv, zero, -invZ * fv, Y * invZZ * fv]
    J2 = [s * (J0[0] - bf * Y * invZZ), s * (J0[1] + bf * X * invZZ), s * J0[2], s * J0[3], zero, s * (J0[5] - bf * invZZ)]
    return [J0, J1, J2]


def load_edges(fp, state, omega, edges, ar):
    n = ar.num
    out = []
    for e in edges:
        stereo = int(fp.eDim[e]) == 3
        out.append(([n(v) for v in state[2][fp.eL[e]]], [n(v) for v in fp.cam[fp.eP[e]]],
                    [n(fp.meas[e][0]), n(fp.meas[e][1]), n(fp.meas[e][2]) if stereo else n(0.0)], n(omega[e]), stereo))
    return out


def cost(eds, inl, q, t, rk, use_robust, ar):
    """F = sum rho(omega |r|^2) over the edges eds[i], i in inl, at (q, t); None where a depth is <= 0"""
    R = rotation(q)
    F = ar.num(0.0)
    for i in inl:
        Xc, r, chi = edge_residual(eds[i], R, t, ar)
        if r is None or not Xc[2] > 0:
            return None
        kind, delta = (rk[1] if eds[i][4] else rk[0]) if use_robust else (0, 0.0)
        F = F + robust(kind, ar.num(delta), chi, ar)[0]
    return F


def linearise(eds, inl, q, t, rk, use_robust, ar):
    """(H 6 x 6, b, F, depths of the edges) over eds[i], i in inl, at (q, t); (None, None, None, depths) where a depth is <= 0"""
    R = rotation(q)
    zero = ar.num(0.0)
    H = [[zero] * 6 for _ in range(6)]
    b, F, depths = [zero] * 6, zero, []
    bad = False
    terms = []
    for i in inl:
        Xc, r, chi = edge_residual(eds[i], R, t, ar)
        depths.append(Xc[2])
        if r is None or not Xc[2] > 0:
            bad = True
            continue
        terms.append((i, Xc, r, chi))
    if bad:
        return None, None, None, depths
    for i, Xc, r, chi in terms:
        kind, delta = (rk[1] if eds[i][4] else rk[0]) if use_robust else (0, 0.0)
        rho, wr = robust(kind, ar.num(delta), chi, ar)
        wr = wr * eds[i][3]
        F = F + rho
        J = pose_jacobian(eds[i], Xc, ar)
        for c in range(6):
            for rr in range(c + 1):
                H[rr][c] = H[rr][c] + wr * (J[0][rr] * J[0][c] + J[1][rr] * J[1][c] + J[2][rr] * J[2][c])
            b[c] = b[c] + wr * (J[0][c] * r[0] + J[1][c] * r[1] + J[2][c] * r[2])
    for c in range(6):
        for rr in range(c):
            H[c][rr] = H[rr][c]
    return H, b, F, depths


def ldlt_solve(H, b, lam, ar):
    """(d or None, the pivots as fractions of their diagonal entries H_jj + lambda)"""
    L = [[ar.num(0.0)] * 6 for _ in range(6)]
    D, frac, ok = [], [], True
    for j in range(6):
        p = H[j][j] + lam
        diag = p
        for k in range(j):
            p = p - L[j][k] * L[j][k] * D[k]
        frac.append(float(p / diag) if ar.finite(p) and ar.finite(diag) and diag != 0 else float("nan"))
        if not p > 0:
            return None, frac
        D.append(p)
        for i in range(j + 1, 6):
            v = H[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k] * D[k]
            L[i][j] = v / p
    y = []
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y.append(v)
    d = [None] * 6
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * d[k]
        d[i] = v
        if not ar.finite(v):
            ok = False
    return (d if ok else None), frac


def _errstate(fn):
    def wrapped(*a, **kw):
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
    return wrapped


@_errstate
def refine_one(fp, state, omega, p, edges, rounds, iterations, robust_rounds, chi2_max, min_inliers, rk, ar=Arith):
    """The definition on one free pose p with the edges `edges` (all of the pose's, sorted).  Returns dict: status, q, t (the final pose
    in the arithmetic's numbers, also of a rejected pose), inliers (the count at the last classification), chi2 (sum omega |r|^2 over the
    final inliers, 0.0 without a final classification), cls (edge id -> bool: the final classification, or None), final_inliers (positions
    in `edges`), history (the edge ids in at every classification, in turn), accepted (trials accepted), and the margins of every decision that rounding could turn: m_chi, m_depth, m_gain, m_pivot
    (lists of relative distances from the decision point)"""
    eds = load_edges(fp, state, omega, edges, ar)
    q, t = [ar.num(v) for v in state[0][p]], [ar.num(v) for v in state[1][p]]
    out = dict(status=OK, q=q, t=t, inliers=0, chi2=0.0, cls=None, final_inliers=[], accepted=0, history=[], m_chi=[], m_depth=[], m_gain=[], m_pivot=[])
    need = max(3, int(min_inliers))

    def classify(chi_test):
        R = rotation(q)
        inl, chis = [], []
        for i, ed in enumerate(eds):
            if not ed[3] > 0:
                continue
            Xc, r, chi = edge_residual(ed, R, t, ar)
            z = Xc[2]
            out["m_depth"].append(float(abs(z) / max(abs(z), 1)) if ar.finite(z) else float("inf"))
            if r is None or not z > 0:
                continue
            if chi_test:
                thr = chi2_max[1] if ed[4] else chi2_max[0]
                if np.isfinite(thr) and ar.finite(chi):
                    out["m_chi"].append(float(abs(chi - thr) / thr))
                if not chi <= thr:
                    continue
            inl.append(i); chis.append(chi)
        out["history"].append([edges[i] for i in inl])
        return inl, chis

    for k in range(rounds):
        use_robust = k < robust_rounds
        inl, _ = classify(k > 0)
        out["inliers"] = len(inl)
        if len(inl) < (3 if k == 0 else need):
            out["status"] = FEW_OBSERVATIONS if k == 0 else FEW_INLIERS
            return out
        H, b, F, _ = linearise(eds, inl, q, t, rk, use_robust, ar)
        lam, nu = ar.num(1e-5) * max(H[j][j] for j in range(6)), ar.num(2.0)
        for _ in range(iterations):
            d, frac = ldlt_solve(H, b, lam, ar)
            out["m_pivot"] += [abs(f) for f in frac]
            if d is None:
                out["status"] = SINGULAR
                return out
            q2, t2 = exp_update(d, q, t, ar)
            H2, b2, F2, depths = linearise(eds, inl, q2, t2, rk, use_robust, ar)
            out["m_depth"] += [float(abs(z) / max(abs(z), 1)) if ar.finite(z) else float("inf") for z in depths]
            accept = False
            if H2 is not None and ar.finite(F2):
                den = sum(d[j] * (lam * d[j] + b[j]) for j in range(6))
                gain = (F - F2) / den if den != 0 else ar.num(float("nan"))
                out["m_gain"].append(float(abs(F - F2) / F) if F > 0 else float("inf"))
                accept = bool(gain > 0)
            if accept:
                q, t, H, b, F = q2, t2, H2, b2, F2
                c = 2 * gain - 1
                lam, nu = lam * max(ar.num(1.0) / 3, 1 - c * c * c), ar.num(2.0)
                out["accepted"] += 1
            else:
                lam, nu = lam * nu, nu * 2
        out["q"], out["t"] = q, t
    inl, chis = classify(True)
    out["inliers"] = len(inl)
    out["final_inliers"] = inl
    out["chi2"] = float(sum(chis, ar.num(0.0)))
    out["cls"] = {edges[i]: (i in set(inl)) for i in range(len(edges))}
    if len(inl) < need:
        out["status"] = FEW_INLIERS
    return out


def refine(fp, state=None, select=None, rounds=4, iterations=10, robust_rounds=2, chi2_max=(CHI2_MONO, CHI2_STEREO), min_inliers=10,
           rk=((0, 0.0), (0, 0.0)), omega=None, poses=None, ar=Arith):
    """The definition on every pose (or on `poses` only: the others keep status -1).  state = (q, t, Xw), default the FlatProblem's;
    omega: the live information per edge in the caller's order, default fp.omega.  Returns dict: status int32[Pt], q [Pt, 4], t [Pt, 3]
    (the refined pose of an OK pose, the state's of every other), inliers int32[Pt], chi2 [Pt], edge_inlier bool[E], counts {name: n},
    steps (per pose the dict of refine_one, or None)"""
    state = (fp.q, fp.t, fp.Xw) if state is None else state
    state = tuple(np.asarray(a, dtype=np.float64) for a in state)
    omega = np.asarray(fp.omega if omega is None else omega, dtype=np.float64)
    lists = pose_edges(fp)
    Pt = fp.Pt
    status = np.full(Pt, -1, dtype=np.int32)
    q, t = state[0].copy(), state[1].copy()
    inliers, chi2 = np.zeros(Pt, dtype=np.int32), np.zeros(Pt)
    edge_inlier = omega > 0
    steps = [None] * Pt
    for p in (range(Pt) if poses is None else poses):
        if select is not None and not select[p]:
            status[p] = NOT_SELECTED; continue
        if p >= fp.Pf:
            status[p] = FIXED; continue
        st = refine_one(fp, state, omega, p, lists[p], rounds, iterations, robust_rounds, chi2_max, min_inliers, rk, ar)
        steps[p] = st
        status[p], inliers[p], chi2[p] = st["status"], st["inliers"], st["chi2"]
        if st["cls"] is not None:
            for e, v in st["cls"].items():
                edge_inlier[e] = v
        if st["status"] == OK:
            q[p], t[p] = [float(v) for v in st["q"]], [float(v) for v in st["t"]]
    counts = {name: int((status == k).sum()) for k, name in enumerate(STATUS_NAMES)}
    return dict(status=status, q=q, t=t, inliers=inliers, chi2=chi2, edge_inlier=edge_inlier, counts=counts, steps=steps, fp=fp,
                args=dict(rounds=rounds, iterations=iterations, robust_rounds=robust_rounds, chi2_max=tuple(chi2_max), min_inliers=min_inliers, rk=rk),
                state=state, omega=omega)


def decision_margin(ref):
    """the smallest relative distance of any decision of the reference from its decision point: (classification, depth, gain, pivot)"""
    m = [np.inf] * 4
    for st in ref["steps"]:
        if st is None:
            continue
        for i, key in enumerate(("m_chi", "m_depth", "m_gain", "m_pivot")):
            if st[key]:
                m[i] = min(m[i], min(st[key]))
    return tuple(float(v) for v in m)


def pose_distance(qa, ta, qb, tb):
    """max(|ta - tb|_inf / max(1, |tb|_inf), the rotation angle of R_a^T R_b), evaluated with 40 digits (the angle of two nearly equal
    rotations is a difference of nearly equal numbers)"""
    import mpmath
    with mpmath.workdps(40):
        qa, qb = [mpmath.mpf(v) for v in qa], [mpmath.mpf(v) for v in qb]
        ta, tb = [mpmath.mpf(v) for v in ta], [mpmath.mpf(v) for v in tb]
        na, nb = mpmath.sqrt(sum(v * v for v in qa)), mpmath.sqrt(sum(v * v for v in qb))
        qa, qb = [v / na for v in qa], [v / nb for v in qb]
        # vector part of conj(qa) qb
        v = [qa[3] * qb[0] - qb[3] * qa[0] - (qa[1] * qb[2] - qa[2] * qb[1]),
             qa[3] * qb[1] - qb[3] * qa[1] - (qa[2] * qb[0] - qa[0] * qb[2]),
             qa[3] * qb[2] - qb[3] * qa[2] - (qa[0] * qb[1] - qa[1] * qb[0])]
        s = mpmath.sqrt(sum(x * x for x in v))
        angle = 2 * mpmath.asin(min(s, mpmath.mpf(1)))
        dt = max(abs(a - b) for a, b in zip(ta, tb)) / max(1, max(abs(b) for b in tb))
        return float(max(dt, angle))


def model_distance(ref, poses):
    """D: the largest pose_distance between the reference's final poses and those of the 60-digit twin run with the same arguments, over
    `poses` (those with a final pose in both); the twin's statuses {pose: status}; the twin's steps {pose: dict}"""
    import mpmath
    fp, a = ref["fp"], ref["args"]
    lists = pose_edges(fp)
    worst, statuses, steps = 0.0, {}, {}
    with mpmath.workdps(60):
        for p in poses:
            st = ref["steps"][p]
            if st is None:
                continue
            mp = refine_one(fp, ref["state"], ref["omega"], p, lists[p], a["rounds"], a["iterations"], a["robust_rounds"], a["chi2_max"], a["min_inliers"],
                            a["rk"], ar=ArithMp)
            statuses[p], steps[p] = mp["status"], mp
            worst = max(worst, pose_distance([float(v) for v in st["q"]], [float(v) for v in st["t"]], mp["q"], mp["t"]))
    return worst, statuses, steps


def gradient_check(fp, state, omega, p, edge_ids, q, t, rk, use_robust, h=1e-15):
    """(central-difference gradient of the 60-digit cost F(exp(d) T) at d = 0 over the edges edge_ids, b of the fp64 linearisation there,
    the size of the gradient's terms: sum_e |w' J_e^T r_e|_inf).  dF/dd = -2 b in this library's sign convention (J = -d r / d d)."""
    import mpmath
    lists_ar = load_edges(fp, state, omega, edge_ids, Arith)
    idx = list(range(len(edge_ids)))
    _, b, _, _ = linearise(lists_ar, idx, [float(v) for v in q], [float(v) for v in t], rk, use_robust, Arith)
    size = 0.0
    for i in idx:
        _, bi, _, _ = linearise(lists_ar, [i], [float(v) for v in q], [float(v) for v in t], rk, use_robust, Arith)
        size += max(abs(v) for v in bi)
    with mpmath.workdps(60):
        eds = load_edges(fp, state, omega, edge_ids, ArithMp)
        qm, tm = [ArithMp.num(v) for v in q], [ArithMp.num(v) for v in t]
        grad = []
        for k in range(6):
            f = []
            for sgn in (1, -1):
                d = [mpmath.mpf(0)] * 6
                d[k] = mpmath.mpf(sgn) * mpmath.mpf(h)
                q2, t2 = exp_update(d, qm, tm, ArithMp)
                f.append(cost(eds, idx, q2, t2, rk, use_robust, ArithMp))
            grad.append(float((f[0] - f[1]) / (2 * mpmath.mpf(h))))
    return np.array(grad), np.array([float(v) for v in b]), size


# ---- graphs -------------------------------------------------------------------------------------------------------------------------
def perturbed_poses(fp, seed, rot_deg=0.3, trans=0.02):
    """(q, t): the FlatProblem's poses moved by exp(d), d random of about rot_deg degrees and trans metres"""
    rng = np.random.default_rng(seed)
    q, t = fp.q.copy(), fp.t.copy()
    for p in range(fp.Pt):
        d = np.concatenate([np.deg2rad(rot_deg) * rng.uniform(-1, 1, 3), trans * rng.uniform(-1, 1, 3)])
        q2, t2 = exp_update([float(v) for v in d], [float(v) for v in q[p]], [float(v) for v in t[p]], Arith)
        q[p], t[p] = q2, t2
    return q, t


ZOO_CAM = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])
ZOO_ROLES = ("two_edges", "three_edges", "n64", "n65", "n150", "mono_only", "stereo_only", "fixed_landmarks", "fixed_pose", "gated",
             "outliers", "behind", "min_inliers", "fill0", "fill1", "fill2")


def wide_problem(seed=7, P=5, L=400, counts=(129, 150, 200, 257, 300)):
    """FlatProblem at the true poses: P free poses of counts[p] observations each (more than 128: the lane-strided loop of a wave runs more
    than twice; 129 and 257 end a trip with one lane), mono and stereo mixed, 0.5 px of noise, one observation in 20 a 5 - 15 px outlier"""
    from scipy.spatial.transform import Rotation
    from cuba_amd.graph import Graph, flatten
    rng = np.random.default_rng(seed)
    centre = np.zeros((P, 3)); centre[:, 0] = 0.4 * np.arange(P)
    rot = Rotation.from_rotvec(np.deg2rad(3.0) * rng.uniform(-1, 1, (P, 3)))
    Rm, q = rot.as_matrix(), rot.as_quat()
    t = -np.einsum("nij,nj->ni", Rm, centre)
    fx, fy, cx, cy, bf = ZOO_CAM
    X = np.column_stack([rng.uniform(-6, 8, L), rng.uniform(-3, 3, L), rng.uniform(8, 25, L)])
    mono, stereo = [], []
    for p in range(P):
        for l in rng.choice(L, counts[p], replace=False):
            Xc = Rm[p] @ X[l] + t[p]
            u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            m = np.array([u, v, u - bf / Xc[2]]) + 0.5 * rng.standard_normal(3)
            if rng.random() < 0.05:
                m = m + rng.uniform(5, 15) * np.array([1.0, -1.0, 1.0])
            (stereo if rng.random() < 0.5 else mono).append((p, int(l), tuple(m)))
    g = Graph(pose_ids=np.arange(P, dtype=np.int64), pose_fixed=np.zeros(P, bool), pose_q=q, pose_t=t, pose_cam=np.tile(ZOO_CAM, (P, 1)),
              lm_ids=np.arange(L, dtype=np.int64), lm_fixed=np.zeros(L, bool), lm_X=X,
              mono_vp=np.array([m[0] for m in mono], dtype=np.int64), mono_vl=np.array([m[1] for m in mono], dtype=np.int64),
              mono_meas=np.array([m[2][:2] for m in mono], dtype=np.float64).reshape(-1, 2), mono_info=np.ones(len(mono)),
              stereo_vp=np.array([m[0] for m in stereo], dtype=np.int64), stereo_vl=np.array([m[1] for m in stereo], dtype=np.int64),
              stereo_meas=np.array([m[2] for m in stereo], dtype=np.float64).reshape(-1, 3), stereo_info=np.ones(len(stereo)), truth=dict(q=q, t=t))
    return flatten(g)


ZOO_START = (2.0, 0.2)      # degrees, metres: how far the zoo's poses start from the true ones
ZOO_NEAR = 1.8               # px: the planted outlier that comes back


def zoo_graph(seed=5):
    """(Graph, roles, extras): one pose per role (roles: name -> row of Graph.pose_*), 300 free landmarks and 40 fixed ones in front of
    the poses; measurements = projections of the points from the TRUE poses + 0.3 px of noise, the poses of zoo_problem = the true ones moved
    by about ZOO_START.
      two_edges, three_edges, n64, n65, n150   poses of 2, 3, 64, 65, 150 observations (mono and stereo mixed)
      mono_only, stereo_only   30 observations of one kind
      fixed_landmarks          30 observations of fixed landmarks only
      fixed_pose               a fixed pose with 30 observations
      gated                    40 observations, 10 of them 40 px off: for the test to gate off (extras["gated_edges"]: rows of the edge lists)
      outliers                 40 mono observations, 6 of them 8 - 12 px off and one ZOO_NEAR px off in u: with one trial per round
                               the pose is still a few px off at round 1, where all seven are out; at round 2 the near one is back
      behind                   10 observations of points behind the camera: FEW_OBSERVATIONS
      min_inliers              8 good observations: FEW_INLIERS with min_inliers = 10, OK with min_inliers = 0
      fill*                    20 - 40 observations"""
    from scipy.spatial.transform import Rotation
    from cuba_amd.graph import Graph
    rng = np.random.default_rng(seed)
    P = len(ZOO_ROLES)
    roles = {name: i for i, name in enumerate(ZOO_ROLES)}
    centre = np.zeros((P, 3)); centre[:, 0] = 0.3 * np.arange(P)
    rot = Rotation.from_rotvec(np.deg2rad(3.0) * rng.uniform(-1, 1, (P, 3)))
    Rm, q_true = rot.as_matrix(), rot.as_quat()
    t_true = -np.einsum("nij,nj->ni", Rm, centre)
    fx, fy, cx, cy, bf = ZOO_CAM
    nfree, nfixed = 300, 40
    X = np.column_stack([rng.uniform(-6, 12, nfree + nfixed), rng.uniform(-3, 3, nfree + nfixed), rng.uniform(8, 25, nfree + nfixed)])
    X_behind = np.column_stack([rng.uniform(0, 5, 10), rng.uniform(-2, 2, 10), rng.uniform(-20, -8, 10)])
    X = np.vstack([X, X_behind])
    lm_fixed = np.zeros(len(X), bool); lm_fixed[nfree:nfree + nfixed] = True
    mono, stereo = [], []
    extras = dict(gated_edges=[], far_outliers=[], near_outlier=None)

    def project(p, Xw):
        Xc = Rm[p] @ Xw + t_true[p]
        u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
        return np.array([u, v, u - bf / Xc[2]])

    def observe(name, lms, stereo_frac=0.5, offsets=None):
        p = roles[name]
        keys = []
        for k, l in enumerate(lms):
            m = project(p, X[l]) + 0.3 * rng.standard_normal(3)
            if offsets is not None and k in offsets:
                m = m + np.array([offsets[k][0], offsets[k][1], offsets[k][0]])
            if rng.random() < stereo_frac:
                stereo.append((p, int(l), tuple(m))); keys.append(("s", len(stereo) - 1))
            else:
                mono.append((p, int(l), tuple(m[:2]))); keys.append(("m", len(mono) - 1))
        return keys

    free = np.arange(nfree)
    for name, n in (("two_edges", 2), ("three_edges", 3), ("n64", 64), ("n65", 65), ("n150", 150)):
        observe(name, rng.choice(free, n, replace=False))
    observe("mono_only", rng.choice(free, 30, replace=False), stereo_frac=0.0)
    observe("stereo_only", rng.choice(free, 30, replace=False), stereo_frac=1.0)
    observe("fixed_landmarks", nfree + rng.choice(nfixed, 30, replace=False))
    observe("fixed_pose", rng.choice(free, 30, replace=False))
    keys = observe("gated", rng.choice(free, 40, replace=False), offsets={k: (40.0, -40.0) for k in range(10)})
    extras["gated_edges"] = keys[:10]
    off = {k: (float(rng.uniform(8, 12)) * (1 if k % 2 else -1), float(rng.uniform(8, 12))) for k in range(6)}
    off[6] = (ZOO_NEAR, 0.0)
    keys = observe("outliers", rng.choice(free, 40, replace=False), stereo_frac=0.0, offsets=off)
    extras["far_outliers"], extras["near_outlier"] = keys[:6], keys[6]
    observe("behind", np.arange(nfree + nfixed, nfree + nfixed + 10))
    observe("min_inliers", rng.choice(free, 8, replace=False))
    for k in range(3):
        observe(f"fill{k}", rng.choice(free, int(rng.integers(20, 41)), replace=False))
    pose_fixed = np.zeros(P, bool); pose_fixed[roles["fixed_pose"]] = True
    g = Graph(pose_ids=np.arange(P, dtype=np.int64), pose_fixed=pose_fixed, pose_q=q_true.copy(), pose_t=t_true.copy(), pose_cam=np.tile(ZOO_CAM, (P, 1)),
              lm_ids=np.arange(len(X), dtype=np.int64), lm_fixed=lm_fixed, lm_X=X.copy(),
              mono_vp=np.array([m[0] for m in mono], dtype=np.int64), mono_vl=np.array([m[1] for m in mono], dtype=np.int64),
              mono_meas=np.array([m[2] for m in mono], dtype=np.float64).reshape(-1, 2), mono_info=np.ones(len(mono)),
              stereo_vp=np.array([m[0] for m in stereo], dtype=np.int64), stereo_vl=np.array([m[1] for m in stereo], dtype=np.int64),
              stereo_meas=np.array([m[2] for m in stereo], dtype=np.float64).reshape(-1, 3), stereo_info=np.ones(len(stereo)),
              truth=dict(q=q_true, t=t_true))
    extras["n_mono"] = len(mono)
    return g, roles, extras


def zoo_problem(seed=5, rot_deg=ZOO_START[0], trans=ZOO_START[1]):
    """(FlatProblem with the perturbed poses and the pose "no_edges" added, {role: solver pose index}, select mask that leaves out fill0, edge mask that gates the
    planted edges of `gated`, {far: [solver edge ids], near: solver edge id} of `outliers`)"""
    from cuba_amd.graph import flatten
    g, roles, extras = zoo_graph(seed)
    fp = flatten(g)
    solver = np.empty(fp.Pt, dtype=np.int64); solver[fp.pose_src] = np.arange(fp.Pt)
    idx = {name: int(solver[row]) for name, row in roles.items()}
    esolver = np.empty(fp.E, dtype=np.int64); esolver[fp.edge_src] = np.arange(fp.E)
    eid = lambda key: int(esolver[key[1] + (extras["n_mono"] if key[0] == "s" else 0)])      # noqa: E731
    fp.q, fp.t = perturbed_poses(fp, seed + 1, rot_deg, trans)
    # "no_edges": a free pose without any edge, behind the last free pose (flatten leaves such a vertex out, the C ABI takes it)
    from cuba_amd.graph import FlatProblem
    P = fp.Pf
    ins = lambda a: np.insert(a, P, a[0], axis=0)      # noqa: E731
    idx = {name: (i + 1 if i >= P else i) for name, i in idx.items()}
    idx["no_edges"] = P
    fp = FlatProblem(fp.Pt + 1, fp.Pf + 1, fp.Lt, fp.Lf, ins(fp.q), ins(fp.t), ins(fp.cam), fp.Xw, np.where(fp.eP >= P, fp.eP + 1, fp.eP).astype(np.int32),
                     fp.eL, fp.eDim, fp.meas, fp.omega, ins(fp.pose_src), fp.lm_src, fp.edge_src)
    select = np.ones(fp.Pt, bool); select[idx["fill0"]] = False
    edge_mask = np.ones(fp.E, bool); edge_mask[[eid(k) for k in extras["gated_edges"]]] = False
    planted = dict(far=[eid(k) for k in extras["far_outliers"]], near=eid(extras["near_outlier"]))
    return fp, idx, select, edge_mask, planted

"""Reference for landmark triangulation (cuba_hip_triangulate_landmarks), numpy + fp64 on a FlatProblem and a state, and a 60-digit mpmath
twin of its numeric steps.

The definition (include/cuba_hip.h), per landmark l, the first status that applies:
  1. active edges S_l: the landmark's edges of information omega > 0.  NOT_SELECTED (a mask was given and select[l] == 0), FIXED,
     FEW_OBSERVATIONS (|S_l| < 2 and no active stereo edge has u - u_r > 0).
  2. parallax, only without such a stereo edge and with min_parallax_deg > 0: unit rays d_i = R_i^T normalize((u - cx) / fx, (v - cy) / fy, 1),
     c = |sum d_i| / |S_l|, LOW_PARALLAX if c > cos(min_parallax_deg / 2).
  3. linear start (the current Xw[l] is never read): rows a = fx R[0] + (cx - u) R[2], b = -(fx t[0] + (cx - u) t[2]); the same in v; stereo:
     a = fx R[0] + (cx - u_r) R[2], b = bf - (fx t[0] + (cx - u_r) t[2]).  A = sum omega a a^T, g = sum omega a b, X = A^-1 g through the
     symmetric 3 x 3 adjugate inverse.  SINGULAR if det A <= 0 or anything is non-finite.
  4. refine_iterations Gauss-Newton steps: H = sum w' JL^T JL, h = sum w' JL^T r, r = proj - meas, JL = -d proj / d X,
     w' = omega rho'(omega |r|^2) with the robust kernels, X <- X + H^-1 h.  SINGULAR as above.
  5. acceptance at the final X: BEHIND_CAMERA if an active edge has Xc.z <= 0, CHI2 if one has omega |r|^2 > chi2_max[stereo], else OK.

Every sum runs over the landmark's edges sorted by (landmark, pose) -- the order of the library's sorted edges when the poses keep the
caller's numbering -- front to back."""
import numpy as np

OK, NOT_SELECTED, FIXED, FEW_OBSERVATIONS, LOW_PARALLAX, SINGULAR, BEHIND_CAMERA, CHI2 = range(8)
STATUS_NAMES = ("ok", "not_selected", "fixed", "few_observations", "low_parallax", "singular", "behind_camera", "chi2")
CHI2_MONO, CHI2_STEREO = 5.991, 7.815
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))        # the packing of sym3_inverse


def quat_to_rot(q):
    x, y, z, w = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def sorted_edges(fp):
    """edge ids sorted by (landmark, pose), stable; ptr[Lt + 1] = every landmark's range"""
    order = np.lexsort((fp.eP, fp.eL))
    ptr = np.zeros(fp.Lt + 1, dtype=np.int64)
    np.cumsum(np.bincount(fp.eL, minlength=fp.Lt), out=ptr[1:])
    return order, ptr


def float_rounded(fp, state=None):
    """(FlatProblem, state) with everything the fp32 library holds as float rounded to float"""
    import copy
    r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # noqa: E731
    out = copy.copy(fp)
    with np.errstate(over="ignore"):         # (the zoo's pose of translation 1e308: inf as a float)
        out.q, out.t, out.Xw, out.cam, out.meas, out.omega = r(fp.q), r(fp.t), r(fp.Xw), r(fp.cam), r(fp.meas), r(fp.omega)
        return out, (None if state is None else tuple(r(a) for a in state))


def float_rounded_kernels(rk):
    return tuple((int(k), float(np.float32(d))) for k, d in rk)


def robust_weight(kind, delta, e):
    d2 = delta * delta
    if kind == 1:
        return 1.0 if e <= d2 else delta / np.sqrt(e)
    if kind == 2:
        u = 1 - e / d2
        return u * u if e <= d2 else 0.0
    return 1.0


def sym3_solve(A, b):
    """(det, A^-1 b) with the adjugate formula of sym3_inverse; A as its 6 unique entries"""
    A00, A01, A02, A11, A12, A22 = A
    det = A00 * A11 * A22 + A01 * A12 * A02 + A02 * A01 * A12 - A00 * A12 * A12 - A02 * A11 * A02 - A01 * A01 * A22
    i = 1 / det
    B = (i * (A11 * A22 - A12 * A12), i * (A02 * A12 - A01 * A22), i * (A01 * A12 - A02 * A11),
         i * (A00 * A22 - A02 * A02), i * (A02 * A01 - A00 * A12), i * (A00 * A11 - A01 * A01))
    x = (B[0] * b[0] + B[1] * b[1] + B[2] * b[2], B[1] * b[0] + B[3] * b[1] + B[4] * b[2], B[2] * b[0] + B[4] * b[1] + B[5] * b[2])
    return det, x


class Arith:
    """the arithmetic the numeric steps run in: python floats (fp64) ..."""
    num = staticmethod(float)
    sqrt = staticmethod(lambda x: float(np.sqrt(x)))
    finite = staticmethod(lambda x: bool(np.isfinite(x)))


class ArithMp:
    """... or mpmath numbers of 60 digits"""
    @staticmethod
    def num(x):
        import mpmath
        return mpmath.mpf(float(x))

    @staticmethod
    def sqrt(x):
        import mpmath
        return mpmath.sqrt(x)

    @staticmethod
    def finite(x):
        import mpmath
        return bool(mpmath.isfinite(x))


def _edge(fp, state, omega, e, ar):
    """one edge in the arithmetic ar: (R rows, t, cam, meas, omega, stereo)"""
    q, t = state[0][fp.eP[e]], state[1][fp.eP[e]]
    n = ar.num
    if ar is Arith:
        R = [[float(v) for v in row] for row in quat_to_rot(q)]
    else:
        x, y, z, w = (n(v) for v in q)
        tx, ty, tz = 2 * x, 2 * y, 2 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        R = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
    stereo = int(fp.eDim[e]) == 3
    m = [n(fp.meas[e][0]), n(fp.meas[e][1]), n(fp.meas[e][2]) if stereo else n(0.0)]
    return R, [n(v) for v in t], [n(v) for v in fp.cam[fp.eP[e]]], m, n(omega[e]), stereo


def _start_terms(ed, ar):
    """A[6], g[3] of one edge"""
    R, t, cam, m, w, stereo = ed
    fx, fy, cx, cy, bf = cam
    du, dv, dr = cx - m[0], cy - m[1], cx - m[2]
    s = ar.num(1.0 if stereo else 0.0)
    a = [[fx * R[0][j] + du * R[2][j] for j in range(3)], [fy * R[1][j] + dv * R[2][j] for j in range(3)],
         [s * (fx * R[0][j] + dr * R[2][j]) for j in range(3)]]
    b = [-(fx * t[0] + du * t[2]), -(fy * t[1] + dv * t[2]), s * (bf - (fx * t[0] + dr * t[2]))]
    A = [w * (a[0][i] * a[0][j] + a[1][i] * a[1][j] + a[2][i] * a[2][j]) for i, j in SYM]
    g = [w * (a[0][i] * b[0] + a[1][i] * b[1] + a[2][i] * b[2]) for i in range(3)]
    return A, g


def _ray(ed, ar):
    R, _, cam, m, _, _ = ed
    nx, ny = -(cam[2] - m[0]) / cam[0], -(cam[3] - m[1]) / cam[1]
    inv = 1 / ar.sqrt(nx * nx + ny * ny + 1)
    d = (nx * inv, ny * inv, inv)
    return [R[0][j] * d[0] + R[1][j] * d[1] + R[2][j] * d[2] for j in range(3)]


def _residual(ed, X, ar):
    """(Xc, r = proj - meas, omega |r|^2)"""
    R, t, cam, m, w, stereo = ed
    Xc = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]
    invZ = 1 / Xc[2]
    u = cam[0] * invZ * Xc[0] + cam[2]
    v = cam[1] * invZ * Xc[1] + cam[3]
    r = [u - m[0], v - m[1], (u - cam[4] * invZ) - m[2] if stereo else ar.num(0.0)]
    return Xc, r, w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2])


def _gn_terms(ed, X, rk, ar):
    """H[6], h[3] of one edge at X"""
    R, _, cam, _, w, stereo = ed
    Xc, r, chi = _residual(ed, X, ar)
    kind, delta = rk[1] if stereo else rk[0]
    if ar is Arith:
        wr = w * robust_weight(kind, float(delta), chi)
    else:
        d = ar.num(delta); d2 = d * d
        wr = w * (1 if kind == 0 else (1 if chi <= d2 else d / ar.sqrt(chi)) if kind == 1 else ((1 - chi / d2) ** 2 if chi <= d2 else 0))
    invZ = 1 / Xc[2]
    invZZ = invZ * invZ
    fu, fv = cam[0], cam[1]
    bf, s = (cam[4], ar.num(1.0)) if stereo else (ar.num(0.0), ar.num(0.0))
    J0 = [-fu * R[0][j] * invZ + fu * Xc[0] * R[2][j] * invZZ for j in range(3)]
    J1 = [-fv * R[1][j] * invZ + fv * Xc[1] * R[2][j] * invZZ for j in range(3)]
    J2 = [s * (J0[j] - bf * R[2][j] * invZZ) for j in range(3)]
    H = [wr * (J0[i] * J0[j] + J1[i] * J1[j] + J2[i] * J2[j]) for i, j in SYM]
    h = [wr * (J0[i] * r[0] + J1[i] * r[1] + J2[i] * r[2]) for i in range(3)]
    return H, h


def _sum(terms, width, ar):
    """front to back"""
    s = [ar.num(0.0)] * width
    for t in terms:
        s = [a + b for a, b in zip(s, t)]
    return s


def _errstate(fn):
    def wrapped(*a, **kw):
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
    return wrapped


@_errstate
def numeric_steps(fp, state, omega, edges, refine_iterations, chi2_max, rk, ar=Arith):
    """steps 3 - 5 on the active edges `edges` (sorted) of one landmark.  Returns dict: status, X (the final position, also of a landmark
    rejected in step 5; None where a step was singular), iterates (X behind the start and every step), h (the last gradient formed at the
    final X, or None), chi ([omega |r|^2] at the final X), depth ([Xc.z]), det (every determinant that was tested, as a fraction of the
    product of its matrix's diagonal -- inf where that product is 0 or the determinant not finite: no rounding decides those)"""
    eds = [_edge(fp, state, omega, e, ar) for e in edges]
    out = dict(status=SINGULAR, X=None, iterates=[], h=None, chi=[], depth=[], det=[])

    def solve(terms):
        s = _sum([a + b for a, b in terms], 9, ar)
        try:
            det, x = sym3_solve(s[:6], s[6:])
        except ZeroDivisionError:              # (det == 0: python raises where IEEE gives inf)
            out["det"].append(0.0 if s[0] * s[3] * s[5] > 0 else float("inf"))
            return None
        hadamard = s[0] * s[3] * s[5]              # (det <= it for a positive semi-definite matrix)
        out["det"].append(float(det / hadamard) if hadamard > 0 and ar.finite(det) else float("inf"))
        return list(x) if det > 0 and all(ar.finite(v) for v in x) else None
    X = solve([_start_terms(ed, ar) for ed in eds])
    if X is None:
        return out
    out["iterates"].append(X)
    for _ in range(refine_iterations):
        try:
            d = solve([_gn_terms(ed, X, rk, ar) for ed in eds])
        except ZeroDivisionError:
            d = None
        if d is None:
            return out
        X = [a + b for a, b in zip(X, d)]
        if not all(ar.finite(v) for v in X):
            return out
        out["iterates"].append(X)
    out["X"] = X
    try:
        res = [_residual(ed, X, ar) for ed in eds]
        out["h"] = _sum([_gn_terms(ed, X, rk, ar)[1] for ed in eds], 3, ar)
    except ZeroDivisionError:
        out["status"] = BEHIND_CAMERA          # (a depth of exactly 0)
        return out
    out["depth"] = [r[0][2] for r in res]
    out["chi"] = [r[2] for r in res]
    thr = [chi2_max[1] if ed[5] else chi2_max[0] for ed in eds]
    if any(z <= 0 for z in out["depth"]):
        out["status"] = BEHIND_CAMERA
    elif any(c > t for c, t in zip(out["chi"], thr)):
        out["status"] = CHI2
    else:
        out["status"] = OK
    return out


@_errstate
def triangulate(fp, state=None, select=None, refine_iterations=5, min_parallax_deg=1.0, chi2_max=(CHI2_MONO, CHI2_STEREO),
                rk=((0, 0.0), (0, 0.0)), omega=None, landmarks=None):
    """The definition on every landmark (or on `landmarks` only: the others keep status -1).  state = (q, t, Xw), default the
    FlatProblem's; omega: the live information per edge in the caller's order, default fp.omega.  Returns dict: status int32[Lt],
    xyz [Lt, 3] (the accepted position of an OK landmark, the state's of every other), counts {name: n}, final [Lt, 3] (the final position
    of every landmark that reached step 5, NaN elsewhere), c [Lt] (the parallax number where it was tested, NaN elsewhere), steps (per
    landmark the dict of numeric_steps, or None), active (per landmark its active edges, sorted)"""
    state = (fp.q, fp.t, fp.Xw) if state is None else state
    state = tuple(np.asarray(a, dtype=np.float64) for a in state)
    omega = np.asarray(fp.omega if omega is None else omega, dtype=np.float64)
    order, ptr = sorted_edges(fp)
    Lt = fp.Lt
    status = np.full(Lt, -1, dtype=np.int32)
    xyz, final, cs = state[2].copy(), np.full((Lt, 3), np.nan), np.full(Lt, np.nan)
    steps, active = [None] * Lt, [None] * Lt
    cos_half = float(np.cos(np.deg2rad(min_parallax_deg) / 2))
    for l in (range(Lt) if landmarks is None else landmarks):
        edges = [int(e) for e in order[ptr[l]:ptr[l + 1]] if omega[e] > 0]
        active[l] = edges
        if select is not None and not select[l]:
            status[l] = NOT_SELECTED; continue
        if l >= fp.Lf:
            status[l] = FIXED; continue
        depth = any(fp.eDim[e] == 3 and fp.meas[e][0] - fp.meas[e][2] > 0 for e in edges)
        if len(edges) < 2 and not depth:
            status[l] = FEW_OBSERVATIONS; continue
        if not depth and min_parallax_deg > 0:
            d = _sum([_ray(_edge(fp, state, omega, e, Arith), Arith) for e in edges], 3, Arith)
            cs[l] = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])) / len(edges)
            if cs[l] > cos_half:
                status[l] = LOW_PARALLAX; continue
        st = numeric_steps(fp, state, omega, edges, refine_iterations, chi2_max, rk)
        steps[l] = st
        status[l] = st["status"]
        if st["X"] is not None:
            final[l] = st["X"]
        if st["status"] == OK:
            xyz[l] = st["X"]
    counts = {name: int((status == k).sum()) for k, name in enumerate(STATUS_NAMES)}
    return dict(status=status, xyz=xyz, counts=counts, final=final, c=cs, steps=steps, active=active, cos_half=cos_half, chi2_max=tuple(chi2_max), fp=fp)


def threshold_margin(ref):
    """per landmark the smallest relative distance of any tested quantity from its threshold -- c from cos(min_parallax / 2), every
    omega |r|^2 at the final position from its chi2 threshold (where that is finite), every depth Xc.z from 0 (|z| / max(|z|, 1): relative
    above a metre, absolute below) --; inf where no such test was made.  (The determinants: determinant_margin.)"""
    fp, Lt = ref["fp"], len(ref["status"])
    m = np.full(Lt, np.inf)
    for l in range(Lt):
        if np.isfinite(ref["c"][l]):
            m[l] = min(m[l], abs(ref["c"][l] - ref["cos_half"]) / ref["cos_half"])
        st = ref["steps"][l]
        if st is None or st["X"] is None:
            continue
        for e, chi, z in zip(ref["active"][l], st["chi"], st["depth"]):
            thr = ref["chi2_max"][1 if fp.eDim[e] == 3 else 0]
            if np.isfinite(thr) and np.isfinite(chi):
                m[l] = min(m[l], abs(chi - thr) / thr)
            m[l] = min(m[l], abs(z) / max(abs(z), 1.0))
    return m


def determinant_margin(ref):
    """per landmark the smallest |det| that was tested against 0, as a fraction of the product of its matrix's diagonal; inf where no
    rounding decides the test.  With every edge of a landmark at full weight the matrices are far from singular (1e-4 and more on the
    suite's graphs).  A Tukey kernel that zeroes all but one mono edge of a landmark leaves H of rank 2: its determinant is then 1e-16 of
    that product, its sign rounding noise, and no two summation orders agree on SINGULAR there."""
    m = np.full(len(ref["status"]), np.inf)
    for l, st in enumerate(ref["steps"]):
        if st is not None and st["det"]:
            m[l] = min(abs(d) for d in st["det"])
    return m


def position_distance(a, b):
    """|a - b|_inf / max(1, |b|_inf) per row"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    return np.abs(a - b).max(1) / np.maximum(1.0, np.abs(b).max(1))


def model_distance(fp, ref, landmarks, refine_iterations, rk, state=None, omega=None):
    """D: the largest position_distance between the reference's final positions and the 60-digit twin's, over `landmarks` (those that
    reached step 5 in both), and the twin's statuses"""
    state = (fp.q, fp.t, fp.Xw) if state is None else state
    omega = np.asarray(fp.omega if omega is None else omega, dtype=np.float64)
    import mpmath
    worst, statuses = 0.0, {}
    with mpmath.workdps(60):
        for l in landmarks:
            if ref["steps"][l] is None:
                continue
            mp = numeric_steps(fp, state, omega, ref["active"][l], refine_iterations, ref["chi2_max"], rk, ar=ArithMp)
            statuses[l] = mp["status"]
            if mp["X"] is not None and ref["steps"][l]["X"] is not None:
                worst = max(worst, float(position_distance(ref["steps"][l]["X"], [float(v) for v in mp["X"]])[0]))
    return worst, statuses


# ---- the zoo: every segment length around the wave / workgroup boundary and one landmark for every status --------------------------
ZOO_COUNTS = (2, 63, 64, 65, 130, 257)
ZOO_CAM = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])


def zoo_graph(seed=3):
    """(Graph, roles): 300 poses on a line looking along +z (a few degrees of rotation each), pose 300 apart; measurements = projections
    of the true points + 0.5 px of noise.  roles: name -> row of Graph.lm_*:
      n2 ... n257       landmarks of 2, 63, 64, 65, 130, 257 observations (mono and stereo mixed)
      one_stereo        one stereo observation: OK through its depth
      no_disparity      one stereo observation with u_r > u: FEW_OBSERVATIONS
      parallel          two mono observations of the principal point from two poses of identity rotation: LOW_PARALLAX -- and, without the
                        parallax test, SINGULAR: A = diag(2 fx^2, 2 fy^2, 0) has the determinant 0 exactly, in any summation order
      behind            two mono rays that meet behind both cameras: BEHIND_CAMERA
      overflow          two mono observations, one from pose 300 whose translation is 1e308: its row's right-hand side overflows, SINGULAR
      outlier           seven mono observations, one of them 30 px off: CHI2
      fixed             a fixed landmark
      gated             four observations, for the test to gate off
      fill*             25 landmarks of 3 - 8 observations
    Landmark `true` positions: Graph.truth["X"]."""
    from scipy.spatial.transform import Rotation
    from cuba_amd.graph import Graph
    rng = np.random.default_rng(seed)
    P = 301
    centre = np.zeros((P, 3)); centre[:, 0] = 0.1 * np.arange(P)
    rot = Rotation.from_rotvec(np.deg2rad(3.0) * rng.uniform(-1, 1, (P, 3)))
    ident = (10, 20, 40, 50, 300)                    # poses of identity rotation (the exact cases)
    rv = rot.as_rotvec(); rv[list(ident)] = 0.0
    rot = Rotation.from_rotvec(rv)
    Rm = rot.as_matrix()
    q = rot.as_quat(); q[list(ident)] = (0.0, 0.0, 0.0, 1.0)
    t = -np.einsum("nij,nj->ni", Rm, centre)
    t[[10, 20, 40, 50]] = -centre[[10, 20, 40, 50]]
    t[300] = (1e308, 0.0, 0.0)
    fx, fy, cx, cy, bf = ZOO_CAM
    X, fixed, roles = [], [], {}
    mono, stereo = [], []        # (pose, landmark row, measurement)

    def project(p, Xw):
        Xc = Rm[p] @ Xw + t[p]
        u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
        return u, v, u - bf / Xc[2]

    def add(name, Xw, poses, stereo_frac=0.5, is_fixed=False):
        row = len(X); roles[name] = row
        X.append(np.asarray(Xw, dtype=np.float64)); fixed.append(is_fixed)
        for p in poses:
            u, v, ur = np.array(project(int(p), X[row])) + 0.5 * rng.standard_normal(3)
            if rng.random() < stereo_frac:
                stereo.append((int(p), row, (u, v, ur)))
            else:
                mono.append((int(p), row, (u, v)))
        return row

    point = lambda: np.array([rng.uniform(5, 25), rng.uniform(-2, 2), rng.uniform(8, 20)])      # noqa: E731
    usable = np.array([p for p in range(300) if p not in ident])
    for n in ZOO_COUNTS:
        poses = np.arange(257) if n == 257 else np.arange(170, 300) if n == 130 else rng.choice(usable, n, replace=False)
        add(f"n{n}", point(), [p for p in poses])
    for k in range(25):
        add(f"fill{k}", point(), rng.choice(usable, int(rng.integers(3, 9)), replace=False))
    add("one_stereo", point(), [7], stereo_frac=1.0)
    row = add("no_disparity", point(), [], stereo_frac=1.0)
    u, v, ur = project(8, X[row]); stereo.append((8, row, (u, v, u + 1.0)))
    row = add("parallel", (1.5, 0.0, 10.0), [])
    mono.append((10, row, (cx, cy))); mono.append((20, row, (cx, cy)))
    row = add("behind", (4.5, 0.0, -5.0), [])
    mono.append((40, row, (cx - 50.0, cy))); mono.append((50, row, (cx + 50.0, cy)))
    row = add("overflow", point(), [60], stereo_frac=0.0)
    mono.append((300, row, (cx + 10.0, cy - 5.0)))
    row = add("outlier", point(), rng.choice(usable, 6, replace=False), stereo_frac=0.0)
    u, v, _ = project(70, X[row]); mono.append((70, row, (u + 30.0, v)))
    add("gated", point(), rng.choice(usable, 4, replace=False))
    add("fixed", point(), rng.choice(usable, 5, replace=False), is_fixed=True)
    X = np.array(X)
    g = Graph(pose_ids=np.arange(P, dtype=np.int64), pose_fixed=np.zeros(P, bool), pose_q=q, pose_t=t, pose_cam=np.tile(ZOO_CAM, (P, 1)),
              lm_ids=np.arange(len(X), dtype=np.int64), lm_fixed=np.array(fixed), lm_X=X.copy(),
              mono_vp=np.array([m[0] for m in mono], dtype=np.int64), mono_vl=np.array([m[1] for m in mono], dtype=np.int64),
              mono_meas=np.array([m[2] for m in mono], dtype=np.float64).reshape(-1, 2), mono_info=np.ones(len(mono)),
              stereo_vp=np.array([m[0] for m in stereo], dtype=np.int64), stereo_vl=np.array([m[1] for m in stereo], dtype=np.int64),
              stereo_meas=np.array([m[2] for m in stereo], dtype=np.float64).reshape(-1, 3), stereo_info=np.ones(len(stereo)),
              truth=dict(X=X))
    return g, roles


def zoo_problem(seed=3):
    """(FlatProblem, {role: solver landmark index}, select mask that leaves out fill0, edge mask that gates the edges of `gated`)"""
    from cuba_amd.graph import flatten
    g, roles = zoo_graph(seed)
    fp = flatten(g)
    solver = np.empty(fp.Lt, dtype=np.int64); solver[fp.lm_src] = np.arange(fp.Lt)
    idx = {name: int(solver[row]) for name, row in roles.items()}
    select = np.ones(fp.Lt, bool); select[idx["fill0"]] = False
    edge_mask = fp.eL != idx["gated"]
    return fp, idx, select, edge_mask

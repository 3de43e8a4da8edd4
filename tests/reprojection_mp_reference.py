"""60-digit mpmath reference of the reprojection edges (mono and stereo), of the normal equations and the Schur complement they assemble
into, of the back-substitution and of the pose / landmark update -- TEST INFRASTRUCTURE, used on the CPU only:
tests/golden/make_golden_reprojection_cases.py evaluates it into tests/golden/reprojection_cases.npz, and the GPU tests read that file, never
this module.  Quaternions, exp6, rho / weight and the mpf conversion are those of tests/se3_mp_reference.py.

It is a function of the fp64 numbers exactly as they are handed to the library (every input becomes a 60-digit mpf before any arithmetic,
every output is rounded to fp64 once, at the end), written from the mathematics and not from the kernels' camera-frame shortcuts:

    Xc = R(q / |q|) X + t          u = fx Xc_x / Xc_z + cx     v = fy Xc_y / Xc_z + cy     (stereo) u_r = u - bf / Xc_z
    r = projection - measurement   e = omega |r|^2             w' = omega rho'(e)           F = sum rho(e)
    D = d projection / d Xc        J_L = D R                   J_P = D [-[Xc]x | I]         (T <- exp([omega; upsilon]) T, X <- X + d)

J_P and J_L are the derivatives of r (the library's arrays hold their negatives; every product below is even in that sign or carries it
explicitly) and are checked against central differences taken at 60 digits (check_jacobians).  With them

    Hll = sum w' J_L^T J_L     bl = -sum w' J_L^T r     Hpp = sum w' J_P^T J_P     bp = -sum w' J_P^T r     Hpl_e = w' J_P^T J_L
    inv_l = (Hll + lambda I)^-1                          Hsc[a][b] = [a == b] Hpp - sum_l sum_{e of a, e' of b} Hpl_e inv_l Hpl_e'^T
    bsc[a] = bp - sum_l sum_{e of a} Hpl_e inv_l bl      xl = inv_l (bl - sum_e Hpl_e^T xp)     scale = sum x (lambda x + b)

over free poses and free landmarks only (Hsc carries no lambda: the library adds it to the pose diagonal when it sets up the reduced solve).
Beside every sum goes the sum of the absolute values of its terms (fp64 is plenty for those), per output entry: the error measure of
tests/test_reprojection_mp_reference.py divides by it."""
import numpy as np

import se3_mp_reference as ref

mp = ref.mp
mpf = ref.mpf
NONE, HUBER, TUKEY = ref.NONE, ref.HUBER, ref.TUKEY
UP = np.triu_indices(6)


def fl(v):
    return np.array([float(x) for x in v])


def fl2(M):
    return np.array([[float(x) for x in row] for row in M])


def rotation(q):
    """rows of R(q / |q|) of fp64 numbers q, at 60 digits"""
    R = ref.quat_rot(ref.quat_unit([mpf(x) for x in q]))
    return [[R[i, j] for j in range(3)] for i in range(3)]


def camera_point(R, t, X):
    return [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]


def project(Xc, cam, stereo):
    fx, fy, cx, cy, bf = cam
    u, v = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
    return [u, v, u - bf / Xc[2]] if stereo else [u, v]


def edge_terms(R, t, cam, X, meas, stereo):
    """(r, J_P, J_L, Xc) of one edge, everything mpf: r has 2 or 3 rows"""
    fx, fy, cx, cy, bf = cam
    Xc = camera_point(R, t, X)
    p = project(Xc, cam, stereo)
    r = [p[i] - meas[i] for i in range(len(p))]
    x, y, z = Xc
    D = [[fx / z, 0, -fx * x / (z * z)], [0, fy / z, -fy * y / (z * z)]]
    if stereo:
        D.append([fx / z, 0, (bf - fx * x) / (z * z)])
    G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0], [y, -x, 0, 0, 0, 1]]          # d Xc / d [omega; upsilon] = [-[Xc]x | I]
    JP = [[sum(Dm[k] * G[k][c] for k in range(3)) for c in range(6)] for Dm in D]
    JL = [[sum(Dm[k] * R[k][c] for k in range(3)) for c in range(3)] for Dm in D]
    return r, JP, JL, Xc


def check_jacobians(q, t, cam, X, meas, stereo):
    """the largest difference between (J_P, J_L) and central differences of r at 60 digits, relative to the largest entry of each"""
    cam, Xm, mm = [mpf(x) for x in cam], [mpf(x) for x in X], [mpf(x) for x in meas]
    T = ref.pose(q, t)
    R0 = [[T[0][i, j] for j in range(3)] for i in range(3)]
    _, JP, JL, _ = edge_terms(R0, [T[1][i] for i in range(3)], cam, Xm, mm, stereo)

    def residual(P, Xv):
        return edge_terms([[P[0][i, j] for j in range(3)] for i in range(3)], [P[1][i] for i in range(3)], cam, Xv, mm, stereo)[0]

    worst = mp.mpf(0)
    for c in range(9):
        if c < 6:
            hi, lo = residual(ref.compose(ref._step(c, 1), T), Xm), residual(ref.compose(ref._step(c, -1), T), Xm)
        else:
            hi = residual(T, [x + (ref.STEP if k == c - 6 else 0) for k, x in enumerate(Xm)])
            lo = residual(T, [x - (ref.STEP if k == c - 6 else 0) for k, x in enumerate(Xm)])
        J = JP if c < 6 else JL
        top = max(abs(x) for row in J for x in row)
        for m in range(len(hi)):
            worst = max(worst, abs((hi[m] - lo[m]) / (2 * ref.STEP) - J[m][c % 6 if c < 6 else c - 6]) / top)
    return float(worst)


class Scene:
    """a graph in the solver numbering (free vertices first) as fp64 arrays: Pf, Lf, q, t, cam, X, eP, eL, stereo[E], meas[E, 3], omega[E]"""

    def __init__(self, Pf, Lf, q, t, cam, X, eP, eL, stereo, meas, omega):
        self.Pf, self.Lf, self.q, self.t, self.cam, self.X = int(Pf), int(Lf), np.asarray(q), np.asarray(t), np.asarray(cam), np.asarray(X)
        self.eP, self.eL, self.stereo, self.meas, self.omega = np.asarray(eP), np.asarray(eL), np.asarray(stereo, dtype=bool), np.asarray(meas), np.asarray(omega)
        self.E = len(self.eP)


def geometry(S, poses=None, X=None):
    """per edge (r, J_P, J_L, Xc) at the scene's estimate, or at given mpf poses [(R rows, t)] / landmarks"""
    if poses is None:
        poses = []
        for p in range(len(S.q)):
            poses.append((rotation(S.q[p]), [mpf(x) for x in S.t[p]]))
    if X is None:
        X = [[mpf(x) for x in row] for row in S.X]
    cams = [[mpf(x) for x in row] for row in S.cam]
    out = []
    for k in range(S.E):
        p, l = int(S.eP[k]), int(S.eL[k])
        out.append(edge_terms(poses[p][0], poses[p][1], cams[p], X[l], [mpf(x) for x in S.meas[k]], bool(S.stereo[k])))
    return out


def chi(S, geo):
    """e = omega |r|^2 per edge"""
    return [mpf(S.omega[k]) * sum(x * x for x in g[0]) for k, g in enumerate(geo)]


def kernel_of(S, k, setting):
    """setting = ((kind, delta) of the mono edges, (kind, delta) of the stereo edges)"""
    return setting[1] if S.stereo[k] else setting[0]


def weights(S, e, setting):
    """(w' = omega rho'(e), rho(e)) per edge"""
    w, rho = [], []
    for k in range(S.E):
        kind, delta = kernel_of(S, k, setting)
        w.append(mpf(S.omega[k]) * ref.weight(kind, delta, e[k]))
        rho.append(ref.rho(kind, delta, e[k]))
    return w, rho


def _inv3(A):
    M = mp.matrix(A) ** -1
    return [[M[i, j] for j in range(3)] for i in range(3)]


def max_diagonal(S, geo, w):
    """the largest diagonal entry of Hll and Hpp over the free vertices"""
    dl, dp = {}, {}
    for k, (r, JP, JL, _) in enumerate(geo):
        p, l = int(S.eP[k]), int(S.eL[k])
        for i in range(3):
            if l < S.Lf:
                dl[(l, i)] = dl.get((l, i), 0) + w[k] * sum(row[i] * row[i] for row in JL)
        for i in range(6):
            if p < S.Pf:
                dp[(p, i)] = dp.get((p, i), 0) + w[k] * sum(row[i] * row[i] for row in JP)
    return max(list(dl.values()) + list(dp.values()))


def system(S, geo, w, lam, pairs, xp=None):
    """the assembled quantities of a scene as fp64 arrays, each with the term sums `<name>_abs` beside it:
    Hll [Lf, 3, 3], bl [Lf, 3], Hpp [Pf, 6, 6], bp [Pf, 6], inv [Lf, 3, 3] = (Hll + lam I)^-1, hdiag [Pf, 6, 6], bsc [Pf, 6],
    hoff [len(pairs), 6, 6] (the blocks (a, b) of the listed pose pairs, a < b), maxdiag, and with xp [Pf, 6]: xl [Lf, 3], scale"""
    Pf, Lf, lam = S.Pf, S.Lf, mpf(lam)
    zero = mp.mpf(0)
    Hll = [[[zero] * 3 for _ in range(3)] for _ in range(Lf)]
    bl = [[zero] * 3 for _ in range(Lf)]
    Hpp = [[[zero] * 6 for _ in range(6)] for _ in range(Pf)]
    bp = [[zero] * 6 for _ in range(Pf)]
    A = {n: np.zeros(s) for n, s in (("Hll", (Lf, 3, 3)), ("bl", (Lf, 3)), ("Hpp", (Pf, 6, 6)), ("bp", (Pf, 6)), ("hdiag", (Pf, 6, 6)), ("bsc", (Pf, 6)),
                                     ("hoff", (len(pairs), 6, 6)), ("xl", (Lf, 3)))}
    Hpl, of_lm = {}, [[] for _ in range(Lf)]
    for k, (r, JP, JL, _) in enumerate(geo):
        p, l, m = int(S.eP[k]), int(S.eL[k]), len(r)
        jp, jl, rr, wk = fl2(JP), fl2(JL), fl(r), float(w[k])
        if l < Lf:
            for i in range(3):
                for j in range(3):
                    Hll[l][i][j] += w[k] * sum(JL[a][i] * JL[a][j] for a in range(m))
                bl[l][i] -= w[k] * sum(JL[a][i] * r[a] for a in range(m))
            A["Hll"][l] += wk * np.abs(jl).T @ np.abs(jl)
            A["bl"][l] += wk * np.abs(jl).T @ np.abs(rr)
        if p < Pf:
            for i in range(6):
                for j in range(i, 6):
                    Hpp[p][i][j] += w[k] * sum(JP[a][i] * JP[a][j] for a in range(m))
                bp[p][i] -= w[k] * sum(JP[a][i] * r[a] for a in range(m))
            A["Hpp"][p] += wk * np.abs(jp).T @ np.abs(jp)
            A["bp"][p] += wk * np.abs(jp).T @ np.abs(rr)
        if p < Pf and l < Lf:
            Hpl[k] = [[w[k] * sum(JP[a][i] * JL[a][j] for a in range(m)) for j in range(3)] for i in range(6)]
            of_lm[l].append(k)
    for p in range(Pf):
        for i in range(6):
            for j in range(i):
                Hpp[p][i][j] = Hpp[p][j][i]
    inv = [_inv3([[Hll[l][i][j] + (lam if i == j else 0) for j in range(3)] for i in range(3)]) for l in range(Lf)]
    hdiag = [[row[:] for row in Hpp[p]] for p in range(Pf)]
    A["hdiag"] += A["Hpp"]
    bsc = [row[:] for row in bp]
    A["bsc"] += A["bp"]
    HI = {}          # Hpl_e inv_l, per edge
    for l in range(Lf):
        ai, abl = np.abs(fl2(inv[l])), A["bl"][l]
        for k in of_lm[l]:
            HI[k] = [[sum(Hpl[k][i][c] * inv[l][c][j] for c in range(3)) for j in range(3)] for i in range(6)]
        by_pose = {}
        for k in of_lm[l]:
            by_pose.setdefault(int(S.eP[k]), []).append(k)
        for p, ks in by_pose.items():
            for a in ks:
                aa = np.abs(fl2(Hpl[a]))
                for i in range(6):
                    bsc[p][i] -= sum(HI[a][i][c] * bl[l][c] for c in range(3))
                A["bsc"][p] += aa @ ai @ abl
                for b in ks:
                    for i in range(6):
                        for j in range(6):
                            hdiag[p][i][j] -= sum(HI[a][i][c] * Hpl[b][j][c] for c in range(3))
                    A["hdiag"][p] += aa @ ai @ np.abs(fl2(Hpl[b])).T
    edges_of = {}
    for l in range(Lf):
        for k in of_lm[l]:
            edges_of.setdefault((int(S.eP[k]), l), []).append(k)
    lms_of = {}
    for (p, l) in edges_of:
        lms_of.setdefault(p, set()).add(l)
    hoff = []
    for n, (a, b) in enumerate(pairs):
        T = [[zero] * 6 for _ in range(6)]
        for l in sorted(lms_of.get(a, set()) & lms_of.get(b, set())):
            ai = np.abs(fl2(inv[l]))
            for ea in edges_of[(a, l)]:
                for eb in edges_of[(b, l)]:
                    for i in range(6):
                        for j in range(6):
                            T[i][j] -= sum(HI[ea][i][c] * Hpl[eb][j][c] for c in range(3))
                    A["hoff"][n] += np.abs(fl2(Hpl[ea])) @ ai @ np.abs(fl2(Hpl[eb])).T
        hoff.append(T)
    out = {"Hll": np.array([fl2(x) for x in Hll]).reshape(Lf, 3, 3), "bl": np.array([fl(x) for x in bl]).reshape(Lf, 3),
           "Hpp": np.array([fl2(x) for x in Hpp]).reshape(Pf, 6, 6), "bp": np.array([fl(x) for x in bp]).reshape(Pf, 6),
           "inv": np.array([fl2(x) for x in inv]).reshape(Lf, 3, 3), "hdiag": np.array([fl2(x) for x in hdiag]).reshape(Pf, 6, 6),
           "bsc": np.array([fl(x) for x in bsc]).reshape(Pf, 6), "hoff": np.array([fl2(x) for x in hoff]).reshape(len(pairs), 6, 6)}
    diag = [Hll[l][i][i] for l in range(Lf) for i in range(3)] + [Hpp[p][i][i] for p in range(Pf) for i in range(6)]
    out["maxdiag"] = float(max(diag))
    if xp is not None:
        xpm = [[mpf(x) for x in row] for row in xp]
        xl, scale, scale_abs = [], zero, 0.0
        for l in range(Lf):
            c, ca = bl[l][:], A["bl"][l].copy()
            for k in of_lm[l]:
                p = int(S.eP[k])
                for j in range(3):
                    c[j] -= sum(Hpl[k][i][j] * xpm[p][i] for i in range(6))
                ca += np.abs(fl2(Hpl[k])).T @ np.abs(np.asarray(xp[p], dtype=np.float64))
            x = [sum(inv[l][i][j] * c[j] for j in range(3)) for i in range(3)]
            A["xl"][l] = np.abs(fl2(inv[l])) @ ca
            xl.append(x)
            for i in range(3):
                scale += x[i] * (lam * x[i] + bl[l][i])
                scale_abs += abs(float(x[i])) * (float(lam) * abs(float(x[i])) + A["bl"][l][i])
        for p in range(Pf):
            for i in range(6):
                scale += xpm[p][i] * (lam * xpm[p][i] + bp[p][i])
                scale_abs += abs(float(xp[p][i])) * (float(lam) * abs(float(xp[p][i])) + A["bp"][p][i])
        out["xl"], out["scale"], A["scale"] = np.array([fl(x) for x in xl]).reshape(Lf, 3), float(scale), scale_abs
    else:
        del A["xl"]
    for n, a in A.items():
        out[n + "_abs"] = a
    return out


def updated_pose(q, t, d):
    """T <- exp([omega; upsilon]) T of fp64 (q, t, d): (quaternion normalised with w >= 0, translation, the composed quaternion's w
    before the sign was settled), mpf"""
    dm = [mpf(x) for x in d]
    qe = ref.quat_exp(dm[:3])
    qn = ref.quat_unit(ref.quat_mul(qe, ref.quat_unit([mpf(x) for x in q])))
    Re, te = ref.exp6(dm)
    tn = Re * ref.column(t) + te
    w = qn[3]
    if w < 0:
        qn = [-x for x in qn]
    return qn, [tn[i] for i in range(3)], w

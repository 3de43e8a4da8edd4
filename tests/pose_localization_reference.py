"""Reference for pose localisation from scratch (cuba_hip_localize_poses): a numpy model of the definition in include/cuba_hip.h -- hash,
sample, P3P, discard rules, MSAC score, arg-min, classification -- in fp64, and a 60-digit mpmath twin of its numeric steps.

Per free selected pose p: the usable edges are its reprojection edges of live information omega > 0 (fewer than 4: FEW_OBSERVATIONS).
Hypothesis h takes the three usable edges of smallest key K(seed, p, h, e) (p, e: the caller's indices), ordered by key.  P3P: Grunert's
law-of-cosines system reduced to a quartic in v = s_3 / s_1 (N^2 - 2 cg N D + D^2 W, multiplied out), Ferrari's split through the largest
real root of the resolvent cubic (closed form, two Newton steps), each root polished by two Newton steps on the quartic and the three
distances by two Newton steps on the law-of-cosines system itself, [R | t] from two orthonormal triads.  A candidate is discarded if it is not finite, a distance is <= 0, its three points are collinear to rounding in
either frame (sin^2 <= 1e-24) or one of its own three edges has depth <= 0 or omega |r|^2 > chi2_max[dim].  Score C = sum over the usable edges of min(omega |r|^2, chi2_max[dim]) (depth <= 0 or a chi2 that is not
finite: chi2_max[dim]); the winner is the candidate of smallest C, a tie to the smaller 4 h + root; none: NO_SOLUTION; fewer than
max(4, min_inliers) edges in at the winner: FEW_INLIERS.

The sample is integer arithmetic, so the twin takes the reference's samples.  The twin does not score every candidate again (a pose of 300
edges and 1024 hypotheses has some 10^6 edge evaluations): it recomputes the reference's winner and runner-up with 60 digits, scores both
and asserts that they keep their order; margin (a) says how far apart the reference's two best scores are."""
import numpy as np

import pose_refinement_reference as PR

OK, NOT_SELECTED, FIXED, FEW_OBSERVATIONS, NO_SOLUTION, FEW_INLIERS = range(6)
STATUS_NAMES = ("ok", "not_selected", "fixed", "few_observations", "no_solution", "few_inliers")
CHI2_MONO, CHI2_STEREO = 5.991, 7.815
MASK = (1 << 64) - 1
GOLDEN = 0x9e3779b97f4a7c15


class Arith(PR.Arith):
    acos = staticmethod(lambda x: float(np.arccos(x)))
    cbrt = staticmethod(lambda x: float(np.cbrt(x)))


class ArithMp(PR.ArithMp):
    @staticmethod
    def acos(x):
        import mpmath
        return mpmath.acos(x)

    @staticmethod
    def cbrt(x):
        import mpmath
        return mpmath.cbrt(x)


# ---- the hash ---------------------------------------------------------------------------------------------------------------------------
def mix(x):
    """the finaliser of splitmix64 on a python int"""
    x &= MASK
    x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & MASK
    x ^= x >> 27; x = (x * 0x94d049bb133111eb) & MASK
    x ^= x >> 31
    return x


def key(seed, p, h, e):
    """K(seed, p, h, e)"""
    return mix(mix(mix(mix(seed + GOLDEN) + p) + h) + e)


def mix_array(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(30); x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
    return x


def samples(seed, p, hypotheses, usable, edge_ids=None):
    """[hypotheses, 3] edge ids: per hypothesis the three edges of `usable` with the smallest keys, ordered by key (a tie: the smaller
    caller's index).  edge_ids: the caller's index of every edge where it is not the edge's own position (a permuted copy of a graph)"""
    usable = np.asarray(usable, dtype=np.int64)
    ids = usable if edge_ids is None else np.asarray(edge_ids, dtype=np.int64)[usable]
    first = np.argsort(ids, kind="stable")
    usable, ids = usable[first], ids[first].astype(np.uint64)
    kh = np.array([mix(mix(mix(seed + GOLDEN) + p) + h) for h in range(hypotheses)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        keys = mix_array(kh[:, None] + ids[None, :])
    order = np.argsort(keys, axis=1, kind="stable")[:, :3]
    return usable[order]


# ---- P3P ----------------------------------------------------------------------------------------------------------------------------------
def unit(v, ar):
    inv = 1 / ar.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [inv * v[0], inv * v[1], inv * v[2]]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def triad(A, B, C, ar):
    """rows e1 = unit(B - A), e2 = e3 x e1, e3 = unit(e1 x (C - A)); None: the points are collinear (or coincide) to rounding,
    |e1 x (C - A)|^2 <= 1e-24 |C - A|^2"""
    d1, d2 = [B[i] - A[i] for i in range(3)], [C[i] - A[i] for i in range(3)]
    if d1[0] == 0 and d1[1] == 0 and d1[2] == 0:
        return None
    e1 = unit(d1, ar)
    n = cross(e1, d2)
    if not n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > ar.num(1e-24) * (d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2]):
        return None
    e3 = unit(n, ar)
    return [e1, cross(e3, e1), e3]


def bearing(cam, m, ar):
    return unit([(m[0] - cam[2]) / cam[0], (m[1] - cam[3]) / cam[1], ar.num(1.0)], ar)


def quartic(f, X, ar):
    """the normalised quartic v^4 + B v^3 + C v^2 + D v + E of the sample and Ferrari's split (s, the two discriminants)"""
    a2 = sum((X[1][i] - X[2][i]) * (X[1][i] - X[2][i]) for i in range(3))
    b2 = sum((X[0][i] - X[2][i]) * (X[0][i] - X[2][i]) for i in range(3))
    c2 = sum((X[0][i] - X[1][i]) * (X[0][i] - X[1][i]) for i in range(3))
    ca = sum(f[1][i] * f[2][i] for i in range(3))
    cb = sum(f[0][i] * f[2][i] for i in range(3))
    cg = sum(f[0][i] * f[1][i] for i in range(3))
    K, Cc = (a2 - c2) / b2, c2 / b2
    n2, n1, n0 = K - 1, -2 * K * cb, 1 + K
    d1, d0 = -2 * ca, 2 * cg
    w2, w1, w0 = -Cc, 2 * Cc * cb, 1 - Cc
    g2 = 2 * cg
    A4 = n2 * n2 + d1 * d1 * w2
    A3 = 2 * n2 * n1 - g2 * (n2 * d1) + d1 * d1 * w1 + 2 * d1 * d0 * w2
    A2 = n1 * n1 + 2 * n2 * n0 - g2 * (n2 * d0 + n1 * d1) + d1 * d1 * w0 + 2 * d1 * d0 * w1 + d0 * d0 * w2
    A1 = 2 * n1 * n0 - g2 * (n1 * d0 + n0 * d1) + 2 * d1 * d0 * w0 + d0 * d0 * w1
    A0 = n0 * n0 - g2 * (n0 * d0) + d0 * d0 * w0
    B, C, D, E = A3 / A4, A2 / A4, A1 / A4, A0 / A4
    BB = B * B
    p = C - 3 * BB / 8
    q = D - B * C / 2 + BB * B / 8
    r = E - B * D / 4 + BB * C / 16 - 3 * BB * BB / 256
    c1, c0 = p * p / 4 - r, -q * q / 8
    P = -p * p / 12 - r
    Q = -p * p * p / 108 + p * r / 3 - q * q / 8
    disc = Q * Q / 4 + P * P * P / 27
    z = ar.num(0.0)
    if disc > 0:
        A = ar.cbrt(abs(Q) / 2 + ar.sqrt(disc))
        if Q > 0:
            A = -A
        z = A - P / (3 * A)
    elif P < 0:
        sp = ar.sqrt(-P / 3)
        arg = (3 * Q / (2 * P)) / sp
        arg = 1 if arg > 1 else -1 if arg < -1 else arg
        z = 2 * sp * ar.cos(ar.acos(arg) / 3)
    m = z - p / 3
    for _ in range(2):
        gm = ((m + p) * m + c1) * m + c0
        gp = (3 * m + 2 * p) * m + c1
        if gp != 0:
            m = m - gm / gp
    s = ar.sqrt(2 * m) if m >= 0 else ar.num(float("nan"))
    hq = q / (2 * s) if s != 0 else ar.num(float("nan"))
    return dict(B=B, C=C, D=D, E=E, s=s, disc=(s * s - 4 * (p / 2 + m + hq), s * s - 4 * (p / 2 + m - hq)), n=(n2, n1, n0), ca=ca, cb=cb, cg=cg, a2=a2, b2=b2, c2=c2)


def candidate(k, slot, f, X, ar):
    """root `slot` of the quartic -> (R, t), or None: no such root, a distance <= 0, a number that is not finite"""
    disc = k["disc"][0 if slot < 2 else 1]
    if not disc >= 0:
        return None
    sq = ar.sqrt(disc)
    v = ((k["s"] if slot < 2 else -k["s"]) + (-sq if slot & 1 else sq)) / 2 - k["B"] / 4
    for _ in range(2):
        fv = (((v + k["B"]) * v + k["C"]) * v + k["D"]) * v + k["E"]
        fp = ((4 * v + 3 * k["B"]) * v + 2 * k["C"]) * v + k["D"]
        if fp != 0:
            v = v - fv / fp
    n2, n1, n0 = k["n"]
    den = 2 * (k["cg"] - k["ca"] * v)
    w = 1 + v * v - 2 * v * k["cb"]
    if den == 0 or not ar.finite(v) or not w > 0:
        return None
    u = ((n2 * v + n1) * v + n0) / den
    s1 = ar.sqrt(k["b2"] / w)
    s2, s3 = u * s1, v * s1
    ca, cb, cg = k["ca"], k["cb"], k["cg"]
    for _ in range(2):                         # two Newton steps on the law-of-cosines system in the three distances (Cramer's rule)
        F1 = s2 * s2 + s3 * s3 - 2 * s2 * s3 * ca - k["a2"]
        F2 = s1 * s1 + s3 * s3 - 2 * s1 * s3 * cb - k["b2"]
        F3 = s1 * s1 + s2 * s2 - 2 * s1 * s2 * cg - k["c2"]
        ja, jb = 2 * (s2 - s3 * ca), 2 * (s3 - s2 * ca)
        jc, jd = 2 * (s1 - s3 * cb), 2 * (s3 - s1 * cb)
        je, jg = 2 * (s1 - s2 * cg), 2 * (s2 - s1 * cg)
        det = ja * jd * je + jb * jc * jg
        if det != 0:
            s1, s2, s3 = (s1 - (-F1 * jd * jg + ja * jd * F3 + jb * jg * F2) / det, s2 - (F1 * jd * je + jb * jc * F3 - jb * je * F2) / det,
                          s3 - (-ja * jc * F3 + ja * je * F2 + F1 * jc * jg) / det)
    if not (s1 > 0 and s2 > 0 and s3 > 0):
        return None
    Y = [[s * f[j][i] for i in range(3)] for j, s in enumerate((s1, s2, s3))]
    ec, ew = triad(Y[0], Y[1], Y[2], ar), triad(X[0], X[1], X[2], ar)
    if ec is None or ew is None:
        return None
    R = [[ec[0][i] * ew[0][j] + ec[1][i] * ew[1][j] + ec[2][i] * ew[2][j] for j in range(3)] for i in range(3)]
    t = [Y[0][i] - (R[i][0] * X[0][0] + R[i][1] * X[0][1] + R[i][2] * X[0][2]) for i in range(3)]
    if not all(ar.finite(x) for row in R for x in row) or not all(ar.finite(x) for x in t):
        return None
    return R, t


def p3p(f, X, ar=Arith):
    """[(root index, R, t)] of the bearings f[3] and the points X[3]: the candidates before the test on their own edges"""
    with np.errstate(all="ignore"):
        try:
            k = quartic(f, X, ar)
        except ZeroDivisionError:
            return []
        out = []
        for slot in range(4):
            try:
                c = candidate(k, slot, f, X, ar)
            except ZeroDivisionError:
                c = None
            if c is not None:
                out.append((slot, c[0], c[1]))
        return out


def quaternion(R, ar):
    """(x, y, z, w), w >= 0, of a rotation matrix: Shepperd, the branches of pose_exp_update"""
    c = [ar.num(0.0)] * 4
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        tr = ar.sqrt(tr + 1)
        c[3] = tr / 2
        tr = ar.num(1.0) / 2 / tr
        c[0], c[1], c[2] = (R[2][1] - R[1][2]) * tr, (R[0][2] - R[2][0]) * tr, (R[1][0] - R[0][1]) * tr
    else:
        c1 = R[1][1] > R[0][0]
        c2 = R[2][2] > (R[1][1] if c1 else R[0][0])
        i = 2 if c2 else 1 if c1 else 0
        j, k = (i + 1) % 3, (i + 2) % 3
        tr = ar.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
        c[i] = tr / 2
        tr = ar.num(1.0) / 2 / tr
        c[3], c[j], c[k] = (R[k][j] - R[j][k]) * tr, (R[j][i] + R[i][j]) * tr, (R[k][i] + R[i][k]) * tr
    invn = 1 / ar.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3])
    if c[3] < 0:
        invn = -invn
    return [invn * v for v in c]


# ---- residuals: one formula for a python float, an mpmath number and a numpy array of edges ---------------------------------------------
def edge_chi(R, t, cam, X, m, stereo, w):
    """(depth, omega |r|^2) at [R | t]; X[3], m[3], stereo (1 / 0) and w scalars or arrays over edges"""
    Xc = [R[i][0] * X[0] + R[i][1] * X[1] + R[i][2] * X[2] + t[i] for i in range(3)]
    invZ = 1 / Xc[2]
    u = cam[0] * invZ * Xc[0] + cam[2]
    v = cam[1] * invZ * Xc[1] + cam[3]
    r0, r1 = u - m[0], v - m[1]
    r2 = stereo * ((u - cam[4] * invZ) - m[2])
    return Xc[2], w * (r0 * r0 + r1 * r1 + r2 * r2)


class PoseEdges:
    """the usable edges of a pose as arrays (fp64) and as lists in an arithmetic"""
    def __init__(self, fp, state, omega, p, edges):
        self.ids = np.array([e for e in edges if omega[e] > 0], dtype=np.int64)
        ids = self.ids
        self.stereo = (np.asarray(fp.eDim)[ids] == 3).astype(np.float64)
        self.X = np.asarray(state[2], dtype=np.float64)[np.asarray(fp.eL)[ids]].T.copy()
        self.m = np.asarray(fp.meas, dtype=np.float64)[ids].T.copy()
        self.m[2] = np.where(self.stereo > 0, self.m[2], 0.0)
        self.w = np.asarray(omega, dtype=np.float64)[ids]
        self.cam = [float(v) for v in fp.cam[p]]
        self.row = {int(e): i for i, e in enumerate(ids)}

    def one(self, e, ar):
        i = self.row[int(e)]
        n = ar.num
        return [n(self.X[k, i]) for k in range(3)], [n(self.m[k, i]) for k in range(3)], n(self.stereo[i]), n(self.w[i])


def score(pe, R, t, chi2_max):
    """(C, depth[n], chi[n]) in fp64 over the usable edges"""
    with np.errstate(all="ignore"):
        R = [[float(x) for x in row] for row in R]
        t = [float(x) for x in t]
        depth, chi = edge_chi(R, t, pe.cam, pe.X, pe.m, pe.stereo, pe.w)
        cap = np.where(pe.stereo > 0, chi2_max[1], chi2_max[0])
        inl = (depth > 0) & (chi <= cap)
        # (a sum front to back, as the device's thread takes it)
        return float(np.add.reduce(np.where(inl, chi, cap))), depth, chi, inl


def score_mp(pe, R, t, chi2_max):
    """the same with the twin's numbers: (C, depth[n], chi[n], inl[n])"""
    import mpmath
    cam = [ArithMp.num(v) for v in pe.cam]
    C, depths, chis, inl = mpmath.mpf(0), [], [], []
    for e in pe.ids:
        X, m, st, w = pe.one(e, ArithMp)
        try:
            depth, chi = edge_chi(R, t, cam, X, m, st, w)
        except ZeroDivisionError:
            depth, chi = mpmath.mpf(0), mpmath.mpf("nan")
        cap = ArithMp.num(chi2_max[1] if st > 0 else chi2_max[0])
        ok = bool(depth > 0 and chi <= cap)
        C += chi if ok else cap
        depths.append(depth); chis.append(chi); inl.append(ok)
    return C, depths, chis, inl


def solve_sample(pe, sample, chi2_max, ar):
    """[(root index, R, t)]: the candidates of a sample that pass the test on their own three edges"""
    cam = [ar.num(v) for v in pe.cam]
    own = [pe.one(e, ar) for e in sample]
    f = [bearing(cam, o[1], ar) for o in own]
    X = [o[0] for o in own]
    out = []
    for slot, R, t in p3p(f, X, ar):
        good = True
        for Xo, mo, st, w in own:
            try:
                depth, chi = edge_chi(R, t, cam, Xo, mo, st, w)
            except ZeroDivisionError:
                good = False; break
            if not (depth > 0 and chi <= (chi2_max[1] if st > 0 else chi2_max[0])):
                good = False; break
        if good:
            out.append((slot, R, t))
    return out


def localize_one(fp, state, omega, p, edges, hypotheses, seed, chi2_max, min_inliers, edge_ids=None):
    """The definition on one free pose p with the edges `edges` (all of the pose's).  Returns dict: status, usable, and with a winner: winner
    (4 h + root), R, t, q (the quaternion), cost, inliers, cls (edge id -> bool), candidates ([(C, 4 h + root, sample tuple)], sorted)"""
    pe = PoseEdges(fp, state, omega, p, edges)
    out = dict(status=OK, usable=len(pe.ids), inliers=len(pe.ids), cost=0.0, winner=-1, cls=None, pe=pe, candidates=[])
    if len(pe.ids) < 4:
        out["status"] = FEW_OBSERVATIONS
        return out
    smp = samples(seed, p, hypotheses, pe.ids, edge_ids)
    best = None
    for h in range(hypotheses):
        for slot, R, t in solve_sample(pe, smp[h], chi2_max, Arith):
            C = score(pe, R, t, chi2_max)[0]
            idx = 4 * h + slot
            out["candidates"].append((C, idx, tuple(int(e) for e in smp[h])))
            if best is None or C < best[0]:
                best = (C, idx, R, t)
    out["candidates"].sort()
    if best is None:
        out["status"] = NO_SOLUTION
        return out
    C, idx, R, t = best
    _, _, _, inl = score(pe, R, t, chi2_max)
    out.update(cost=C, inliers=int(inl.sum()), cls={int(e): bool(v) for e, v in zip(pe.ids, inl)}, R=R, t=t, q=quaternion(R, Arith), best=idx)
    if out["inliers"] < max(4, int(min_inliers)):
        out["status"] = FEW_INLIERS
    else:
        out["winner"] = idx
    return out


def localize(fp, state=None, select=None, hypotheses=256, seed=0, chi2_max=(CHI2_MONO, CHI2_STEREO), min_inliers=10, omega=None, poses=None,
             scalar=np.float64, edge_ids=None):
    """The definition on every pose (or on `poses` only: the others keep status -1).  state = (q, t, Xw), default the FlatProblem's (q and t
    are only passed through); omega: the live information per edge in the caller's order, default fp.omega; scalar: the type the estimate is
    stored as.  Returns dict: status int32[Pt], q [Pt, 4], t [Pt, 3] (the winner's pose of an OK pose, the state's of every other), inliers,
    winner int32[Pt], cost [Pt], edge_inlier bool[E], counts {name: n}, steps (per pose the dict of localize_one, or None)"""
    state = (fp.q, fp.t, fp.Xw) if state is None else state
    state = tuple(np.asarray(a, dtype=np.float64) for a in state)
    omega = np.asarray(fp.omega if omega is None else omega, dtype=np.float64)
    lists = PR.pose_edges(fp)
    Pt = fp.Pt
    status = np.full(Pt, -1, dtype=np.int32)
    q, t = state[0].copy(), state[1].copy()
    inliers, winner, cost = np.zeros(Pt, dtype=np.int32), np.full(Pt, -1, dtype=np.int32), np.zeros(Pt)
    edge_inlier = omega > 0
    steps = [None] * Pt
    for p in (range(Pt) if poses is None else poses):
        if select is not None and not select[p]:
            status[p] = NOT_SELECTED; continue
        if p >= fp.Pf:
            status[p] = FIXED; continue
        st = localize_one(fp, state, omega, p, lists[p], hypotheses, seed, chi2_max, min_inliers, edge_ids)
        steps[p] = st
        status[p], inliers[p], cost[p], winner[p] = st["status"], st["inliers"], st["cost"], st["winner"]
        if st["cls"] is not None:
            for e, v in st["cls"].items():
                edge_inlier[e] = v
        if st["status"] == OK:
            q[p] = np.asarray(st["q"], dtype=scalar).astype(np.float64)
            t[p] = np.asarray(st["t"], dtype=scalar).astype(np.float64)
    counts = {name: int((status == k).sum()) for k, name in enumerate(STATUS_NAMES)}
    return dict(status=status, q=q, t=t, inliers=inliers, winner=winner, cost=cost, edge_inlier=edge_inlier, counts=counts, steps=steps, fp=fp,
                args=dict(hypotheses=hypotheses, seed=seed, chi2_max=tuple(chi2_max), min_inliers=min_inliers), state=state, omega=omega)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def twin_candidate(ref, p, idx):
    """(R, t, C, depths, chis, inl) of candidate idx = 4 h + root of pose p, recomputed with 60 digits from the reference's sample; None
    where the twin has no such candidate"""
    import mpmath
    st, a = ref["steps"][p], ref["args"]
    sample = next(s for _, i, s in st["candidates"] if i == idx)
    with mpmath.workdps(60):
        for slot, R, t in solve_sample(st["pe"], sample, a["chi2_max"], ArithMp):
            if slot == idx % 4:
                return (R, t) + score_mp(st["pe"], R, t, a["chi2_max"])
    return None


def decision_margin(ref, poses=None):
    """{pose: (a, b)} for the poses with a winner.
    (a) the relative gap (C_2 - C_1) / C_1 between the winner's score and the best score of any OTHER ordered sample or root (a later
        hypothesis that draws the winner's own three edges in the same order repeats its arithmetic bit for bit and loses the tie by its
        index: no decision of rounding); inf with a single candidate.  The twin's scores of the two must keep that order, or (a) is 0.
    (b) the smallest relative distance, at the winner as the twin sees it, of a usable edge's omega |r|^2 from its threshold and of a
        depth from 0 (|z| / max(|z|, 1))."""
    import mpmath
    out = {}
    for p, st in enumerate(ref["steps"]):
        if st is None or st["cls"] is None or (poses is not None and p not in poses):
            continue
        cands = st["candidates"]
        C1, i1, s1 = cands[0]
        assert i1 == st["best"]
        other = [c for c in cands[1:] if not (c[2] == s1 and c[1] % 4 == i1 % 4)]
        a = float("inf")
        with mpmath.workdps(60):
            tw = twin_candidate(ref, p, i1)
            if tw is None:
                out[p] = (0.0, 0.0); continue
            if other:
                a = (other[0][0] - C1) / C1 if C1 > 0 else float("inf")
                tw2 = twin_candidate(ref, p, other[0][1])
                if tw2 is not None and not tw[2] < tw2[2]:
                    a = 0.0
            _, _, _, depths, chis, _ = tw
            caps = np.where(st["pe"].stereo > 0, ref["args"]["chi2_max"][1], ref["args"]["chi2_max"][0])
            b = float("inf")
            for z, chi, cap in zip(depths, chis, caps):
                b = min(b, float(abs(z) / max(abs(z), 1)))
                if mpmath.isfinite(chi):
                    b = min(b, float(abs(chi - cap) / cap))
        out[p] = (float(a), b)
    return out


def model_distance(ref, poses):
    """{pose: D}: pose_distance between the reference's winner and the twin's recomputation of it (both before the rounding to the stored
    scalar type), over `poses` (those with status OK)"""
    import mpmath
    out = {}
    for p in poses:
        st = ref["steps"][p]
        if st is None or st["status"] != OK:
            continue
        with mpmath.workdps(60):
            tw = twin_candidate(ref, p, st["winner"])
            assert tw is not None
            qm = quaternion(tw[0], ArithMp)
            out[p] = PR.pose_distance([float(v) for v in st["q"]], [float(v) for v in st["t"]], qm, tw[1])
    return out


# ---- graphs -------------------------------------------------------------------------------------------------------------------------------
def with_outliers(fp, seed, noise=0.5, outlier_frac=0.2, lo=50.0, hi=200.0):
    """a copy of the FlatProblem whose measurements carry `noise` px of Gaussian noise and of which one edge in five is a gross outlier (moved
    by 50 - 200 px in a random direction); returns (fp, outlier mask)"""
    import copy
    rng = np.random.default_rng(seed)
    out = copy.copy(fp)
    meas = np.array(fp.meas, dtype=np.float64, copy=True)
    meas[:, :3] += noise * rng.standard_normal((fp.E, 3))
    bad = rng.random(fp.E) < outlier_frac
    ang = rng.uniform(0, 2 * np.pi, fp.E)
    mag = rng.uniform(lo, hi, fp.E)
    meas[bad, 0] += (mag * np.cos(ang))[bad]
    meas[bad, 1] += (mag * np.sin(ang))[bad]
    meas[bad, 2] += (mag * np.cos(ang))[bad]
    meas[np.asarray(fp.eDim) != 3, 2] = np.asarray(fp.meas)[np.asarray(fp.eDim) != 3, 2]
    out.meas = meas
    return out, bad


def nan_poses(fp, select=None):
    """(q, t) with the selected free poses' values thrown away"""
    q, t = np.array(fp.q, dtype=np.float64, copy=True), np.array(fp.t, dtype=np.float64, copy=True)
    sel = (np.ones(fp.Pt, bool) if select is None else np.asarray(select, bool)) & (np.arange(fp.Pt) < fp.Pf)
    q[sel] = np.nan; t[sel] = np.nan
    return q, t


def tiny_problem():
    """FlatProblem at the true poses: five free poses of 3, 4, 5, 6 and 6 mono observations of 12 landmarks (`three`, `four`, `five`,
    `collinear`: its six landmarks lie on one line, `gated`: the test switches its edges off) and one fixed pose of 6; exact measurements.
    Returns (fp, {name: solver pose index}, {name: solver edge ids})"""
    from scipy.spatial.transform import Rotation
    from cuba_amd.graph import Graph, flatten
    rng = np.random.default_rng(3)
    names = ("three", "four", "five", "collinear", "gated", "fixed")
    n_obs = (3, 4, 5, 6, 6, 6)
    P = len(names)
    centre = np.zeros((P, 3)); centre[:, 0] = 0.3 * np.arange(P)
    rot = Rotation.from_rotvec(np.deg2rad(4.0) * rng.uniform(-1, 1, (P, 3)))
    Rm, q = rot.as_matrix(), rot.as_quat()
    t = -np.einsum("nij,nj->ni", Rm, centre)
    X = np.column_stack([rng.uniform(-4, 5, 12), rng.uniform(-2, 2, 12), rng.uniform(8, 20, 12)])
    line = np.array([-2.0, 0.5, 10.0])[None, :] + np.arange(6)[:, None] * np.array([0.9, 0.2, 1.1])[None, :]
    X = np.vstack([X, line])
    fx, fy, cx, cy, _ = PR.ZOO_CAM
    mono = []
    for p, name in enumerate(names):
        lms = 12 + np.arange(6) if name == "collinear" else rng.choice(12, n_obs[p], replace=False)
        for l in lms:
            Xc = Rm[p] @ X[l] + t[p]
            mono.append((p, int(l), (fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy)))
    fixed = np.zeros(P, bool); fixed[names.index("fixed")] = True
    g = Graph(pose_ids=np.arange(P, dtype=np.int64), pose_fixed=fixed, pose_q=q, pose_t=t, pose_cam=np.tile(PR.ZOO_CAM, (P, 1)),
              lm_ids=np.arange(len(X), dtype=np.int64), lm_fixed=np.zeros(len(X), bool), lm_X=X,
              mono_vp=np.array([m[0] for m in mono], dtype=np.int64), mono_vl=np.array([m[1] for m in mono], dtype=np.int64),
              mono_meas=np.array([m[2] for m in mono], dtype=np.float64).reshape(-1, 2), mono_info=np.ones(len(mono)),
              stereo_vp=np.zeros(0, dtype=np.int64), stereo_vl=np.zeros(0, dtype=np.int64), stereo_meas=np.zeros((0, 3)), stereo_info=np.zeros(0),
              truth=dict(q=q, t=t))
    fp = flatten(g)
    solver = np.empty(fp.Pt, dtype=np.int64); solver[fp.pose_src] = np.arange(fp.Pt)
    idx = {name: int(solver[i]) for i, name in enumerate(names)}
    edges = {name: np.flatnonzero(np.asarray(fp.eP) == idx[name]) for name in names}
    return fp, idx, edges


# ---- the inputs of tests/test_gpu_pose_localization.py; tests/test_pose_localization_reference.py checks the margin condition on them ----
HYPOTHESES = (1, 64, 256, 257, 1024)
MARGIN = 1e-6
SEED = {"small": 9, "wide": 2}          # the seeds of localize_poses (the header of tests/test_gpu_pose_localization.py says which were tried)
NOISE_SEED = {"small": 21, "wide": 22}
_inputs, _cases = {}, {}


def gpu_input(name):
    """"small": the suite's small graph (39 free poses of 14 ... 115 edges, mono and stereo mixed, one fixed pose) at the true poses and
    points; "wide": wide_problem (5 poses of 129 ... 300 edges; it carries 0.5 px of noise already) with the poses 0 and 1 made mono-only.
    Measurements: 0.5 px of noise, one edge in five a gross outlier of 50 - 200 px."""
    if name not in _inputs:
        from cuba_amd.graph import flatten
        from cuba_amd.synth import synth_ba
        if name == "small":
            fp, _ = with_outliers(flatten(synth_ba(40, 600, 2400, seed=1, perturb=False)), NOISE_SEED[name])
        else:
            fp = PR.wide_problem()
            fp.eDim = np.where(np.asarray(fp.eP) < 2, 2, np.asarray(fp.eDim)).astype(np.asarray(fp.eDim).dtype)
            fp.meas = np.array(fp.meas, dtype=np.float64, copy=True)
            fp.meas[np.asarray(fp.eDim) == 2, 2] = 0.0
            fp, _ = with_outliers(fp, NOISE_SEED[name], noise=0.0)
        _inputs[name] = fp
    return _inputs[name]


def gpu_case(name, hypotheses, f32=False, **args):
    """(FlatProblem, the reference's result, {pose: (a, b)} margins, {pose: D}) of an input of the GPU tests, computed once; f32: the
    reference on the float-rounded inputs, its poses rounded to float"""
    key = (name, hypotheses, f32, tuple(sorted(args.items())))
    if key not in _cases:
        fp = gpu_input(name)
        src = PR.float_rounded(fp)[0] if f32 else fp
        ref = localize(src, hypotheses=hypotheses, seed=args.pop("seed", SEED[name]), scalar=np.float32 if f32 else np.float64, **args)
        _cases[key] = (fp, ref, decision_margin(ref), model_distance(ref, range(fp.Pt)))
    return _cases[key]

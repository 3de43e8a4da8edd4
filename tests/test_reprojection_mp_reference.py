"""The numpy transcription of the reprojection kernels (csrc/ba_math.hpp: edge_residual, edge_jacobians, robust_weight / robust_rho,
sym3_inverse, pose_exp_update; the camera-frame pose and block passes of csrc/ba_linearize.hip; edge_hplT_x / finish_landmark of
csrc/ba_edge.hip) against the 60-digit reference of tests/reprojection_mp_reference.py, over the three scenes recorded in
tests/golden/reprojection_cases.npz (tests/golden/make_golden_reprojection_cases.py).  This module also holds what
tests/test_gpu_reprojection_regimes.py shares with it: the fixture's reader, the builder of the counts scene, the model, the error measure,
the regimes and their bounds.

ERROR MEASURE.  Every output entry is a sum; the fixture holds, per block (a landmark's Hll, bl, inverse, xl; a pose's Hpp, bp, diagonal
block of Hsc, bsc; a pair's block of Hsc), the largest sum of the ABSOLUTE values of the terms of its entries, and the error of a block is
max |got - want| over the block divided by that -- never by the maximum of a whole array.  ((Hll + lambda I)^-1 is measured against its
own largest entry, e per edge against e.)  A block whose terms all vanish (a landmark all of whose edges have weight 0) must be 0 exactly.

REGIMES AND BOUNDS.  Regimes scene: {residual: e per edge; direct: Hll, bl, Hpp, bp -- plain sums over edges; schur: the inverse, diagonal
and off-diagonal blocks of Hsc, bsc, xl -- everything behind (Hll + lambda I)^-1} x depth tier (Z ~ 0.5, 8, 400, 2e4) x {near, moved}; the counts scene is one regime of
each group.  MODEL_ERROR holds the largest error of the fp64 model per regime (test_models_against_the_reference keeps it honest within a
factor 3); a kernel output is held to max(16 x MODEL_ERROR, 32 eps), x 2^29 on the fp32 library (tm.bound's rule, unchanged).  Measured:

    regime        residual: near    moved      direct: near    moved      schur: near    moved
    Z ~ 0.5           2.5e-12     4.2e-10        3.1e-12     2.1e-10       2.5e-13     4.3e-11
    Z ~ 8             2.8e-13     2.4e-11        1.1e-12     1.4e-11       5.5e-14     3.2e-12
    Z ~ 400           1.3e-12     1.2e-12        7.8e-13     8.5e-13       6.6e-13     6.4e-13
    Z ~ 2e4           5.8e-13     5.8e-13        4.7e-13     1.1e-12       4.5e-13     6.0e-13
    counts            8.2e-12                    9.2e-13                   3.4e-13

(relative to the sums of absolute terms the schur rows are no worse than the direct ones, even at Z ~ 2e4, where the stereo disparity is
0.0025 pixel and Hll is regular only through lambda: the adjugate inverse is measured against its own largest entry.  Every row is led by
the cancellation in r = projection - measurement, |r| ~ 0.25 pixel of ~500, which "moved" makes worse at Z ~ 0.5: R X + t at |t| ~ 1e3.)

ROBUST KERNELS.  A weight is a function of e, which carries the regime's error B: besides B relative, a block may be off by what the
variation dw of rho' over e (1 +- 2 B) (tm.kernel_window) makes of its edges' terms, sum_e omega dw_e s_e relative to sum_e omega w_e s_e
(s_e the size of the edge's unweighted J^T J), x 4 because a weight enters a Schur product twice and its inverse once.

POSE UPDATE.  pose_exp_update transcribed and run at the library's own precision, float64 and float32 separately, per band of theta
(split at 1e-5, 3.4e-4, 1e-2, 2 pi / 3, pi): quaternion entries relative to 1, the translation relative to |V upsilon| + |t|.  The bound
of the update is 16 x the model's error at that precision, at least 32 eps of that precision (no 2^29 rule: float32 loses far less than
that would allow, except where the formula itself loses a2 and a3).  Measured:

    band of theta            float64 model   float32 model
    [0, 1e-5)                1.5e-16         1.1e-07
    [1e-5, 3.4e-4)           6.2e-13         1.5e-05
    [3.4e-4, 1e-2)           2.9e-15         8.6e-06
    [1e-2, 2 pi / 3)         1.1e-15         5.4e-07
    [2 pi / 3, pi)           5.4e-16         4.0e-07
    [pi, ...)                4.6e-16         2.2e-07

In float32 the translation of a step with 1e-5 <= theta < 3.4e-4 is wrong by up to 1.5e-05 of |V upsilon| + |t| (theta |upsilon| / 2 in
absolute terms: the whole 1/2 omega x upsilon term), 140 x the 1.1e-07 of the series branch below 1e-5, and the band above it still loses
8.6e-06; float64 loses 6.2e-13 there to the same cancellation, 4000 x its neighbours.  This is the formula the library shares with the
project it was modelled on; it is recorded here, not fixed, and the kernel is pinned to it and to nothing worse.  ("landmark": X + xl, one
addition; "objective": sum rho at the updated estimate, relative to itself.)"""
import os
import sys

import numpy as np
import pytest

import robust_pose_factor_reference as rf
import test_se3_mp_reference as tm

GOLDEN = tm.GOLDEN
PATH = os.path.join(GOLDEN, "reprojection_cases.npz")
EPS = tm.EPS
EPS32 = float(np.finfo(np.float32).eps)
TIERS = ("Z ~ 0.5", "Z ~ 8", "Z ~ 400", "Z ~ 2e4")
SCENES = ("near", "moved")
DIRECT = ("Hll", "bl", "Hpp", "bp")
SCHUR = ("inv", "hdiag", "bsc", "hoff", "xl")
LANDMARK_FAMILIES = ("Hll", "bl", "inv", "xl")
UP, UP3 = np.triu_indices(6), np.triu_indices(3)
BAND_EDGES = (1e-5, 3.4e-4, 1e-2, 2 * float(np.pi) / 3, float(np.pi))
BANDS = ("[0, 1e-5)", "[1e-5, 3.4e-4)", "[3.4e-4, 1e-2)", "[1e-2, 2 pi / 3)", "[2 pi / 3, pi)", "[pi, ...)")

MODEL_ERROR = {
    ('residual', 0, 'near'): 2.5e-12, ('residual', 1, 'near'): 2.8e-13, ('residual', 2, 'near'): 1.3e-12, ('residual', 3, 'near'): 5.8e-13,
    ('residual', 0, 'moved'): 4.2e-10, ('residual', 1, 'moved'): 2.4e-11, ('residual', 2, 'moved'): 1.2e-12, ('residual', 3, 'moved'): 5.8e-13,
    ('direct', 0, 'near'): 3.1e-12, ('direct', 1, 'near'): 1.1e-12, ('direct', 2, 'near'): 7.8e-13, ('direct', 3, 'near'): 4.7e-13,
    ('direct', 0, 'moved'): 2.1e-10, ('direct', 1, 'moved'): 1.4e-11, ('direct', 2, 'moved'): 8.5e-13, ('direct', 3, 'moved'): 1.1e-12,
    ('schur', 0, 'near'): 2.5e-13, ('schur', 1, 'near'): 5.5e-14, ('schur', 2, 'near'): 6.6e-13, ('schur', 3, 'near'): 4.5e-13,
    ('schur', 0, 'moved'): 4.3e-11, ('schur', 1, 'moved'): 3.2e-12, ('schur', 2, 'moved'): 6.4e-13, ('schur', 3, 'moved'): 6.0e-13,
    ('residual', 'counts'): 8.2e-12, ('direct', 'counts'): 9.2e-13, ('schur', 'counts'): 3.4e-13,
}
UPDATE_MODEL_ERROR = {
    (0, 'f64'): 1.5e-16, (1, 'f64'): 6.2e-13, (2, 'f64'): 2.9e-15, (3, 'f64'): 1.1e-15, (4, 'f64'): 5.4e-16, (5, 'f64'): 4.6e-16,
    ('landmark', 'f64'): 1.1e-16, ('objective', 'f64'): 5.8e-12, (0, 'f32'): 1.1e-07, (1, 'f32'): 1.5e-05, (2, 'f32'): 8.6e-06, (3, 'f32'): 5.4e-07,
    (4, 'f32'): 4.0e-07, (5, 'f32'): 2.2e-07, ('landmark', 'f32'): 8.9e-08, ('objective', 'f32'): 6.9e-04,
}


def bound(regime, precision="f64"):
    """tm.bound's rule on this module's table: 16 x the model's error, at least 32 eps; x 2^29 on the fp32 library"""
    return max(16.0 * MODEL_ERROR[regime], 32.0 * EPS) * (2.0 ** 29 if precision == "f32" else 1.0)


def update_bound(band, precision):
    """16 x the error of the model run at that precision, at least 32 eps of that precision"""
    return max(16.0 * UPDATE_MODEL_ERROR[(band, precision)], 32.0 * (EPS32 if precision == "f32" else EPS))


# ---- small helpers in plain IEEE arithmetic (no libm beyond sqrt: the counts scene must come out bit for bit everywhere) -------------------
def unit(q):
    """se3_mp_reference.library_unit, for any length"""
    s = 0.0
    for x in q:
        s += float(x) * float(x)
    n = float(np.sqrt(s))
    return np.array([float(x) / n for x in q])


def unit3(v):
    return unit(v)


def quat_to_rot(q, T=np.float64):
    x, y, z, w = (T(v) for v in q)
    two = T(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = T(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=T)


def band_of(theta):
    return np.searchsorted(np.array(BAND_EDGES), np.asarray(theta), side="right")


def shepperd_branch_of(w):
    """-1: positive trace (theta < 2 pi / 3); else the index of the largest diagonal entry of exp(w), which is the largest |axis| entry"""
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    th = np.linalg.norm(w, axis=1)
    return np.where(th < BAND_EDGES[3], -1, np.abs(w).argmax(axis=1))


def chosen_xp(Pf, size=1e-3):
    return np.array([[size * ((7 * p + 3 * i) % 11 - 5) / 5.0 for i in range(6)] for p in range(Pf)])


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
_fixture = {}


def fixture():
    """{key: array} of the npz, read once"""
    if not _fixture:
        with np.load(PATH) as z:
            for key in z.files:
                _fixture[key] = z[key]
    return _fixture


def sub(prefix):
    """the entries under a prefix, by their remaining name"""
    return {k[len(prefix) + 1:]: v for k, v in fixture().items() if k.startswith(prefix + "/")}


def scene_inputs(name):
    """the graph of a scene as a dict: the fixture's arrays, for "counts" what counts_graph() builds"""
    if name == "counts":
        G = counts_graph()
        assert np.array_equal(np.array([G["meas"].sum(), G["X"].sum(), G["q"].sum(), G["t"].sum()]), fixture()["counts/checksum"])
        return G
    S = sub(name)
    G = {k: S[k] for k in ("q", "t", "cam", "X", "eP", "eL", "stereo", "meas", "omega")}
    G["Pf"], G["Lf"] = int(S["sizes"][0]), int(S["sizes"][1])
    return G


def settings_of(name):
    return [s for s in range(3) if "%s/s%d/lam" % (name, s) in fixture()]


def kernels_of(name, s):
    k = fixture()["%s/s%d/kernels" % (name, s)] if name != "update" else fixture()["update/kernels"]
    return ((int(k[0][0]), float(k[0][1])), (int(k[1][0]), float(k[1][1])))


# ---- scene "counts": built from plain arithmetic ------------------------------------------------------------------------------------------
COUNT_LANDMARKS = (1, 2, 3, 63, 64, 65, 128, 256, 257, 271)
COUNT_POSES = (1, 63, 64, 65, 129)
LISTED_PAIRS = {(263, 264): 1, (268, 269): 15, (265, 266): 16, (261, 262): 17, (259, 260): 64, (257, 258): 65}
_counts = {}


def counts_graph():
    """272 poses (the last one fixed) and the landmarks' observation lists, chosen one by one: see assert_counts() for what they realise.
    Landmark order = the order the waves are packed in when the library's landmark reordering is off: 63 + 1 fill one wave exactly,
    2 + 3 + 59 the next, the landmark with 64 edges a third; then the landmarks with more than 64."""
    if _counts:
        return _counts
    P = 272
    q = np.array([unit([0.01 * (p % 7 - 3), 0.02 * (p % 5 - 2), 0.005 * (p % 11 - 5), 1.0]) for p in range(P)])
    t = np.array([[0.05 * p - 7.0, 0.3 * (p % 3), 0.1 * (p % 4)] for p in range(P)])
    centre = -t          # (approximately: the rotations are small)
    free, fixed = [], []          # (observing poses, depth, repeated observation of the first pose)

    def add(poses, depth, to=free, twice=False):
        to.append((list(poses), depth, twice))

    add(range(190, 253), 30.0), add([270], 6.0), add([268, 269], 6.0), add([265, 266, 267], 6.0), add(range(100, 159), 30.0), add(range(150, 214), 30.0)
    add(range(0, 65), 32.0), add(range(0, 128), 34.0), add(range(0, 256), 36.0), add(range(0, 257), 38.0), add(range(0, 271), 40.0)
    for n in range(64):
        add([257, 258, 0], 8.0)
    for n in range(63):
        add([259, 260] + ([0] if n < 60 else []), 8.0)
    for n in range(16):
        add([261, 262], 6.0)
    for n in range(14):
        add([265, 266, 261], 6.0)
    for n in range(13):
        add([268, 269, 261], 6.0)
    for n in range(19):
        add([261], 6.0)
    add([262, 267], 6.0, twice=True)
    add([271], 6.0), add([271], 7.0)
    add(range(100, 200), 33.0, fixed), add([5, 6], 8.0, fixed)
    lms = free + fixed
    X = np.zeros((len(lms), 3))
    edges = []          # (pose, landmark, stereo)
    for l, (poses, depth, twice) in enumerate(lms):
        c = np.array([centre[p] for p in poses])
        X[l] = [c[:, 0].sum() / len(poses) + 0.11 * (l % 9 - 4), 0.13 * (l % 7 - 3), depth + 0.05 * (l % 40)]
        single = len(poses) == 1
        for n, p in enumerate(poses):
            edges.append((p, l, single or (n + l) % 3 != 0))
        if twice:
            edges.append((poses[0], l, False))
    edges.sort(key=lambda e: e[2])          # mono first
    eP, eL = np.array([e[0] for e in edges], dtype=np.int32), np.array([e[1] for e in edges], dtype=np.int32)
    stereo = np.array([e[2] for e in edges], dtype=bool)
    cam = np.tile(np.array([500.0, 480.0, 320.0, 240.0, 50.0]), (P, 1))
    noise = np.random.default_rng(5).random((len(edges), 3))
    meas = np.zeros((len(edges), 3))
    for k in range(len(edges)):
        r, _, _ = model_residual(q[eP[k]], t[eP[k]], cam[eP[k]], X[eL[k]], np.zeros(3), bool(stereo[k]))
        meas[k, :3 if stereo[k] else 2] = (r + (noise[k] - 0.5) * 0.6)[:3 if stereo[k] else 2]
        if k % 97 == 5:
            meas[k, 0] += 3.0
    sampled, n = [], 0
    while len(sampled) < 64:          # a fixed sample among the pairs of the big landmarks
        a = (7 * n) % 230
        if (a, a + 1 + (13 * n) % 20) not in sampled:
            sampled.append((a, a + 1 + (13 * n) % 20))
        n += 1
    _counts.update(Pf=P - 1, Lf=len(free), q=q, t=t, cam=cam, X=X, eP=eP, eL=eL, stereo=stereo, meas=meas, omega=np.ones(len(edges)),
                   listed_pairs=sorted(LISTED_PAIRS) + [(0, 257), (262, 267)], sampled_pairs=sampled,
                   mode0_poses=np.array([0, 257, 258, 259, 260, 261, 262, 263, 264, 267, 270] + list(range(10, 250, 16))))
    return _counts


def assert_counts(G):
    """every count the scene is there for"""
    Pf, Lf = G["Pf"], G["Lf"]
    per_lm = np.bincount(G["eL"], minlength=len(G["X"]))
    assert set(COUNT_LANDMARKS) <= set(per_lm[:Lf]) and (per_lm[Lf:] > 64).any()
    assert list(per_lm[:6]) == [63, 1, 2, 3, 59, 64] and np.all(per_lm[6:11] > 64)          # the packing: 64 | 64 | 64 | the big ones
    per_pose = np.bincount(G["eP"], minlength=Pf + 1)
    assert set(COUNT_POSES) <= set(per_pose[:Pf])
    seen = [set(G["eL"][(G["eP"] == p) & (G["eL"] < Lf)]) for p in range(Pf)]
    for (a, b), n in LISTED_PAIRS.items():
        assert len(seen[a] & seen[b]) == n, (a, b, len(seen[a] & seen[b]))
    twice = [(p, l) for p in range(Pf) for l in seen[p] if ((G["eP"] == p) & (G["eL"] == l)).sum() == 2]
    assert twice == [(262, int(np.nonzero(per_lm == 3)[0][-1]))] or len(twice) == 1
    assert len(G["sampled_pairs"]) == 64 and all(len(seen[a] & seen[b]) >= 3 for a, b in G["sampled_pairs"])


# ---- the model: the kernels' formulas in numpy, at precision T ---------------------------------------------------------------------------
def model_quat_rotate(q, v):
    a0 = q[1] * v[2] - q[2] * v[1]
    a1 = q[2] * v[0] - q[0] * v[2]
    a2 = q[0] * v[1] - q[1] * v[0]
    a0, a1, a2 = a0 + a0, a1 + a1, a2 + a2
    return np.array([v[0] + q[3] * a0 + (q[1] * a2 - q[2] * a1), v[1] + q[3] * a1 + (q[2] * a0 - q[0] * a2), v[2] + q[3] * a2 + (q[0] * a1 - q[1] * a0)])


def model_residual(q, t, cam, X, meas, stereo, T=np.float64):
    """edge_residual: (r[3], Xc, |r|^2)"""
    q, t, cam, X, meas = (np.asarray(a, dtype=T) for a in (q, t, cam, X, meas))
    Xc = model_quat_rotate(q, X) + t
    invZ = T(1) / Xc[2]
    u = cam[0] * invZ * Xc[0] + cam[2]
    v = cam[1] * invZ * Xc[1] + cam[3]
    r = np.array([u - meas[0], v - meas[1], (u - cam[4] * invZ) - meas[2] if stereo else T(0)], dtype=T)
    return r, Xc, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]


def model_jacobians(Xc, R, cam, stereo, mutant=None):
    """edge_jacobians: (JP [3, 6], JL [3, 3]), the library's sign (minus the derivative of r)"""
    T = Xc.dtype.type
    X, Y = Xc[0], Xc[1]
    invZ = T(1) / Xc[2]
    invZZ = invZ * invZ
    fu, fv, bf, s = cam[0], cam[1], (cam[4] if stereo else T(0)), (T(1) if stereo else T(0))
    JL, JP = np.zeros((3, 3), dtype=T), np.zeros((3, 6), dtype=T)
    for j in range(3):
        r0, r1, r2 = (R[j][0], R[j][1], R[j][2]) if mutant == "JL from the columns of R" else (R[0][j], R[1][j], R[2][j])
        JL[0][j] = -fu * r0 * invZ + fu * X * r2 * invZZ
        JL[1][j] = -fv * r1 * invZ + fv * Y * r2 * invZZ
        JL[2][j] = s * (JL[0][j] - bf * r2 * invZZ)
    JP[0] = [X * Y * invZZ * fu, -(T(1) + (X * X * invZZ)) * fu, Y * invZ * fu, -invZ * fu, T(0), X * invZZ * fu]
    JP[1] = [(T(1) + Y * Y * invZZ) * fv, -X * Y * invZZ * fv, -X * invZ * fv, T(0), -invZ * fv, Y * invZZ * fv]
    JP[2] = [s * (JP[0][0] - (T(0) if mutant == "stereo JP[2][0] without bf Y / Z^2" else bf * Y * invZZ)), s * (JP[0][1] + bf * X * invZZ), s * JP[0][2], s * JP[0][3], T(0),
             s * (JP[0][5] - bf * invZZ)]
    return JP, JL


def model_weight(kind, delta, e, mutant=None):
    T = type(e)
    delta = T(delta)
    d2 = delta * delta
    if kind == rf.HUBER:
        return T(1) if e <= d2 else (delta / e if mutant == "Huber weight delta / e" else delta / np.sqrt(e))
    if kind == rf.TUKEY:
        u = T(1) - e / d2
        return (u if mutant == "Tukey weight u" else u * u) if e <= d2 else T(0)
    return T(1)


def model_rho(kind, delta, e):
    T = type(e)
    delta = T(delta)
    d2 = delta * delta
    if kind == rf.HUBER:
        return e if e <= d2 else (T(2) * np.sqrt(e) * delta - d2)
    if kind == rf.TUKEY:
        u = T(1) - e / d2
        top = (T(1) / T(3)) * d2
        return top * (T(1) - u * u * u) if e <= d2 else top
    return e


def sym3(a):
    return np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])


def sym3_batch(a):
    """[n, 6] packed symmetric 3 x 3 (00, 01, 02, 11, 12, 22) -> [n, 3, 3]"""
    return np.array([sym3(r) for r in a]).reshape(-1, 3, 3)


def model_sym3_inverse(A):
    A00, A01, A02, A11, A12, A22 = A
    det = A00 * A11 * A22 + A01 * A12 * A02 + A02 * A01 * A12 - A00 * A12 * A12 - A02 * A11 * A02 - A01 * A01 * A22
    i = type(det)(1) / det
    return np.array([i * (A11 * A22 - A12 * A12), i * (A02 * A12 - A01 * A22), i * (A01 * A12 - A02 * A11), i * (A00 * A22 - A02 * A02), i * (A02 * A01 - A00 * A12),
                     i * (A00 * A11 - A01 * A01)])


def model_camera_frame(Xc, w, stereo, cam, R, mutant=None):
    """camera_frame_edge + camera_frame_m: (K as 6 packed entries, d00, d02, d11, d12, d22, M [3, 3])"""
    T = Xc.dtype.type
    X, Y, Z = Xc
    invZ = T(1) / Z
    invZZ = invZ * invZ
    d00, d02, d11, d12 = -cam[0] * invZ, cam[0] * X * invZZ, -cam[1] * invZ, cam[1] * Y * invZZ
    d22 = d02 - cam[4] * invZZ if stereo else T(0)
    k00 = w * (T(2) * d00 * d00 if stereo else d00 * d00)
    k02 = w * (d00 * d02 + (d00 * d22 if stereo and mutant != "k02 without d00 d22" else T(0)))
    k11, k12 = w * d11 * d11, w * d11 * d12
    k22 = w * (d02 * d02 + d12 * d12 + d22 * d22)
    M = np.array([[k00 * R[0][j] + k02 * R[2][j] for j in range(3)], [k11 * R[1][j] + k12 * R[2][j] for j in range(3)],
                  [k02 * R[0][j] + k12 * R[1][j] + k22 * R[2][j] for j in range(3)]], dtype=T)
    return np.array([k00, T(0), k02, k11, k12, k22], dtype=T), (d00, d02, d11, d12, d22), M


def cross_matrix(X):
    return np.array([[0, -X[2], X[1]], [X[2], 0, -X[0]], [-X[1], X[0], 0]], dtype=X.dtype)


def sandwich(Xa, N, Xb):
    """G_a^T N G_b with G = [-[X]x | I]: the 6 x 6 block the pose and block passes build from a camera-frame 3 x 3 N"""
    Ga = np.hstack([-cross_matrix(Xa), np.eye(3, dtype=Xa.dtype)])
    Gb = np.hstack([-cross_matrix(Xb), np.eye(3, dtype=Xb.dtype)])
    return Ga.T @ N @ Gb


def model_system(G, setting, lam, pairs, xp=None, T=np.float64, mutant=None):
    """what the kernels make of a graph, in the layout of reprojection_mp_reference.system() plus e [E] and F"""
    Pf, Lf, E = G["Pf"], G["Lf"], len(G["eP"])
    q, t, cam, X = (np.asarray(G[k], dtype=T) for k in ("q", "t", "cam", "X"))
    lam = T(lam)
    R = [quat_to_rot(q[p], T) for p in range(len(q))]
    out = {"e": np.zeros(E), "Hll": np.zeros((Lf, 3, 3), dtype=T), "bl": np.zeros((Lf, 3), dtype=T), "Hpp": np.zeros((Pf, 6, 6), dtype=T), "bp": np.zeros((Pf, 6), dtype=T),
           "hdiag": np.zeros((Pf, 6, 6), dtype=T), "bsc": np.zeros((Pf, 6), dtype=T), "hoff": np.zeros((len(pairs), 6, 6), dtype=T)}
    edge, F = [], T(0)
    per_pose, per_lm = {}, {}
    for k in range(E):
        p, l, st = int(G["eP"][k]), int(G["eL"][k]), bool(G["stereo"][k])
        per_pose[p] = per_pose.get(p, 0) + 1
        per_lm[l] = per_lm.get(l, 0) + 1
        r, Xc, ss = model_residual(q[p], t[p], cam[p], X[l], G["meas"][k], st, T)
        kind, delta = setting[1] if st else setting[0]
        e = T(G["omega"][k]) * ss
        out["e"][k] = e
        F += model_rho(kind, delta, e)
        w = T(G["omega"][k]) * model_weight(kind, delta, e, mutant)
        JP, JL = model_jacobians(Xc, R[p], cam[p], st, mutant)
        dropped_l = mutant == "257th edge of a landmark dropped" and per_lm[l] == 257
        dropped_p = mutant == "65th edge of a pose dropped" and per_pose[p] == 65
        edge.append((p, l, st, r, Xc, w, JP, JL, dropped_p))
        if l < Lf and not dropped_l:
            out["Hll"][l] += w * (JL.T @ JL)
            out["bl"][l] += w * (JL.T @ r)
    out["F"] = float(F)
    inv = np.zeros((Lf, 6), dtype=T)
    for l in range(Lf):
        H = out["Hll"][l]
        inv[l] = model_sym3_inverse(np.array([H[0][0] + lam, H[0][1], H[0][2], H[1][1] + lam, H[1][2], H[2][2] + lam], dtype=T))
    out["inv"] = np.array([sym3(a) for a in inv]).reshape(Lf, 3, 3)
    frames, by = {}, {}
    for k, (p, l, st, r, Xc, w, JP, JL, dropped_p) in enumerate(edge):
        if p >= Pf or dropped_p:
            continue
        K, (d00, d02, d11, d12, d22), M = model_camera_frame(Xc, w, st, cam[p], R[p], mutant)
        r2 = r[2] if st else T(0)
        v = np.array([w * d00 * (r[0] + r2), w * d11 * r[1], w * (d02 * r[0] + d12 * r[1] + d22 * r2)], dtype=T)
        S, vs = sym3(K), v.copy()
        out["Hpp"][p] += sandwich(Xc, S, Xc)
        if l < Lf:
            Pm = M @ sym3(inv[l])
            S = S - Pm @ M.T
            vs = v - Pm @ out["bl"][l]
            frames[k] = (Xc, M)
            by.setdefault((p, l), []).append(k)
        out["hdiag"][p] += sandwich(Xc, S, Xc)
        g = np.concatenate([np.cross(Xc, v), v])
        out["bp"][p] += g
        out["bsc"][p] += np.concatenate([np.cross(Xc, vs), vs])
    lms_of = {}
    for (p, l) in by:
        lms_of.setdefault(p, set()).add(l)
    for (p, l), ks in by.items():          # a pose that sees a landmark twice: the block pass adds the cross products to the diagonal block
        for i, a in enumerate(ks):
            for b in ks[i + 1:]:
                N = frames[a][1] @ sym3(inv[l]) @ frames[b][1].T
                Tab = sandwich(frames[a][0], N, frames[b][0])
                out["hdiag"][p] -= Tab + Tab.T
    for n, (a, b) in enumerate(pairs):
        for l in sorted(lms_of.get(a, set()) & lms_of.get(b, set())):
            for ea in by[(a, l)]:
                for eb in by[(b, l)]:
                    N = frames[ea][1] @ sym3(inv[l]) @ frames[eb][1].T
                    out["hoff"][n] -= sandwich(frames[ea][0], N, frames[eb][0])
    diag = np.concatenate([np.einsum("lii->li", out["Hll"]).ravel(), np.einsum("pii->pi", out["Hpp"]).ravel()])
    out["maxdiag"] = float(diag.max())
    if xp is not None:
        xpT = np.asarray(xp, dtype=T)
        csum = np.zeros((Lf, 3), dtype=T)
        for p, l, st, r, Xc, w, JP, JL, _ in edge:          # edge_hplT_x: JL^T w (JP x)
            if l < Lf and p < Pf:
                csum[l] += JL.T @ (w * (JP @ xpT[p]))
        out["xl"] = np.array([sym3(inv[l]) @ (out["bl"][l] - csum[l]) for l in range(Lf)], dtype=T).reshape(Lf, 3)
        out["scale"] = float((out["xl"] * (lam * out["xl"] + out["bl"])).sum() + (xpT * (lam * xpT + out["bp"])).sum())
    return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def model_pose_update(upd, q, t, T=np.float64, mutant=None):
    """pose_exp_update at precision T: (q, t) after T <- exp([omega; upsilon]) T"""
    upd, q, t = (np.asarray(a, dtype=T) for a in (upd, q, t))
    wx, wy, wz = upd[0], upd[1], upd[2]
    theta = np.sqrt(wx * wx + wy * wy + wz * wz)
    if theta < T(0.00001):
        a1, a2, a3 = T(1), T(0.5), T(1) / T(6)
    else:
        sn, cs = np.sin(theta), np.cos(theta)
        a1, a2, a3 = sn / theta, (T(1) - cs) / (theta * theta), (theta - sn) / (theta * theta * theta)
    if mutant == "a3 = 1 / 6 for every theta":
        a3 = T(1) / T(6)
    xx, yy, zz, xy, yz, zx = wx * wx, wy * wy, wz * wz, wx * wy, wy * wz, wz * wx
    o = T(0)
    K = np.array([[o, -wz, wy], [wz, o, -wx], [-wy, wx, o]], dtype=T)
    K2 = np.array([[-yy - zz, xy, zx], [xy, -zz - xx, yz], [zx, yz, -xx - yy]], dtype=T)
    R, te = np.zeros((3, 3), dtype=T), np.zeros(3, dtype=T)
    for i in range(3):
        acc = T(0)
        for j in range(3):
            one = T(1) if i == j else T(0)
            R[i][j] = one + a1 * K[i][j] + a2 * K2[i][j]
            acc += (one + a2 * K[i][j] + a3 * K2[i][j]) * upd[3 + j]
        te[i] = acc
    qe = np.zeros(4, dtype=T)
    tr = R[0][0] + R[1][1] + R[2][2]
    if tr > 0:
        tr = np.sqrt(tr + T(1))
        qe[3] = T(0.5) * tr
        tr = T(0.5) / tr
        qe[0], qe[1], qe[2] = (R[2][1] - R[1][2]) * tr, (R[0][2] - R[2][0]) * tr, (R[1][0] - R[0][1]) * tr
    else:
        c1 = R[1][1] > R[0][0]
        c2 = R[2][2] > (R[1][1] if c1 else R[0][0])
        i = 2 if c2 else 1 if c1 else 0
        if mutant == "two Shepperd branches swapped" and i != 2:
            i = 1 - i
        j, k = (i + 1) % 3, (i + 2) % 3
        tr = np.sqrt(R[i][i] - R[j][j] - R[k][k] + T(1))
        qe[i] = T(0.5) * tr
        tr = T(0.5) / tr
        qe[3], qe[j], qe[k] = (R[k][j] - R[j][k]) * tr, (R[j][i] + R[i][j]) * tr, (R[k][i] + R[i][k]) * tr
    u = t if mutant == "translation te + t" else model_quat_rotate(qe, t)
    tn = te + u
    c = np.zeros(4, dtype=T)
    c[3] = qe[3] * q[3] - qe[0] * q[0] - qe[1] * q[1] - qe[2] * q[2]
    c[0] = qe[3] * q[0] + qe[0] * q[3] + qe[1] * q[2] - qe[2] * q[1]
    c[1] = qe[3] * q[1] + qe[1] * q[3] + qe[2] * q[0] - qe[0] * q[2]
    c[2] = qe[3] * q[2] + qe[2] * q[3] + qe[0] * q[1] - qe[1] * q[0]
    invn = T(1) / np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3])
    if c[3] < 0 and mutant != "no w >= 0 normalisation":
        invn = -invn
    return invn * c, tn


# ---- the error measure -------------------------------------------------------------------------------------------------------------------
def packed(name, a):
    """a family's array as the fixture stores it: symmetric blocks as their 6 or 21 upper entries"""
    a = np.asarray(a, dtype=np.float64)
    if name in ("Hll", "inv"):
        return a[:, UP3[0], UP3[1]]
    return a[:, UP[0], UP[1]] if name in ("Hpp", "hdiag") else a


def block_errors(name, got, want, scale):
    """per block max |got - want| / scale; a block without terms must be 0 exactly"""
    n = len(want)
    d = np.abs(packed(name, got).reshape(n, -1) - want.reshape(n, -1)).max(axis=1) if n else np.zeros(0)
    scale = np.asarray(scale, dtype=np.float64)
    return np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d == 0, 0.0, np.inf))


def edges_of_blocks(G, name, pairs):
    """per block of a family the edges whose weights enter it"""
    if name in LANDMARK_FAMILIES:
        return [np.nonzero(G["eL"] == l)[0] for l in range(G["Lf"])]
    if name == "hoff":
        return [np.nonzero((G["eP"] == a) | (G["eP"] == b))[0] for a, b in pairs]
    return [np.nonzero(G["eP"] == p)[0] for p in range(G["Pf"])]


def windows(G, e, w, setting, B):
    """per edge omega dw: what the kernel's conditioning lets the weight of an edge be off by, beyond B relative"""
    out = np.zeros(len(e))
    for k in range(len(e)):
        kind, delta = setting[1] if G["stereo"][k] else setting[0]
        if kind != rf.NONE:
            out[k] = G["omega"][k] * tm.kernel_window(kind, delta, e[k], B)[0]
    return out


_scales = {}


def edge_scales(scene):
    """per edge the size of its unweighted J^T J, for the landmark and for the pose (two digits suffice: from the model)"""
    if scene not in _scales:
        G = scene_inputs(scene)
        sL, sP = np.zeros(len(G["eP"])), np.zeros(len(G["eP"]))
        for k in range(len(sL)):
            p, l, st = int(G["eP"][k]), int(G["eL"][k]), bool(G["stereo"][k])
            _, Xc, _ = model_residual(G["q"][p], G["t"][p], G["cam"][p], G["X"][l], G["meas"][k], st)
            JP, JL = model_jacobians(Xc, quat_to_rot(G["q"][p]), np.asarray(G["cam"][p], dtype=np.float64), st)
            sL[k], sP[k] = (np.abs(JL).T @ np.abs(JL)).max(), (np.abs(JP).T @ np.abs(JP)).max()
        _scales[scene] = (sL, sP)
    return _scales[scene]


def window_of_blocks(G, name, pairs, dw, w, s_edge):
    """4 sum omega dw s / sum omega w s per block (module docstring)"""
    out = []
    for ks in edges_of_blocks(G, name, pairs):
        den = float((G["omega"][ks] * w[ks] * s_edge[ks]).sum())
        out.append(4.0 * float((dw[ks] * s_edge[ks]).sum()) / den if den > 0 else 0.0)
    return np.array(out)


def regimes_of_blocks(scene, name, S, pairs):
    """the regime of every block of a family"""
    group = "residual" if name == "e" else "direct" if name in DIRECT else "schur"
    if not scene.startswith("regimes"):
        n = {"hoff": len(pairs), "e": len(S["e"])}.get(name, S["sizes"][1] if name in LANDMARK_FAMILIES else S["sizes"][0])
        return [(group, "counts")] * int(n)
    variant = scene.split("/")[1]
    if name == "e":
        tiers = S["ptier"][S["eP"]]
    elif name in LANDMARK_FAMILIES:
        tiers = S["ltier"][:S["sizes"][1]]
    elif name == "hoff":
        tiers = S["ptier"][pairs[:, 0]]
    else:
        tiers = S["ptier"][:S["sizes"][0]]
    return [(group, int(g), variant) for g in tiers]


def families(scene):
    return ("e", "Hll", "bl", "Hpp", "bp", "inv", "hdiag", "bsc", "hoff", "xl")


def compare(scene, s, got, precision="f64", select=None):
    """[(family, block, regime, error, what it may be)] of a scene's outputs under kernel setting s against the fixture.
    got: {family: array} in the fixture's layout (Hpp of the counts scene: the rows of mode0_poses)"""
    S = sub(scene)
    G = scene_inputs(scene)
    pairs = S["pairs"]
    setting = kernels_of(scene, s)
    pre = "s%d/" % s
    rows = []
    robust = setting[0][0] != rf.NONE or setting[1][0] != rf.NONE
    wref = S[pre + "w"] if pre + "w" in S else np.array([rf.weight(*(setting[1] if G["stereo"][k] else setting[0]), S["e"][k]) for k in range(len(S["e"]))])
    for name in select or families(scene):
        want = S["e"] if name == "e" else S[pre + name]
        scale = np.abs(S["e"]) if name == "e" else S[pre + name + "_abs"].astype(np.float64)
        regs = regimes_of_blocks(scene, name, S, pairs)
        err = block_errors(name, got[name], want, scale)
        may = np.array([bound(r, precision) for r in regs])
        if robust and name != "e":
            for B in sorted(set(may)):
                dw = windows(G, S["e"], wref, setting, B)
                win = window_of_blocks(G, name, pairs, dw, wref, edge_scales(scene)[0 if name in LANDMARK_FAMILIES else 1])
                may = np.where(may == B, B + win, may)
        rows += [(name, k, regs[k], float(err[k]), float(may[k])) for k in range(len(err))]
    return rows


def worst_per_regime(rows):
    worst = {}
    for name, k, reg, err, may in rows:
        if err > worst.get(reg, (-1.0,))[0]:
            worst[reg] = (err, name, k, may)
    return worst


# ---- the models over the fixture -----------------------------------------------------------------------------------------------------------
_model = {}


def model_outputs(scene, s, mutant=None, T=np.float64):
    key = (scene, s, mutant, T)
    if key not in _model:
        S, G = sub(scene), scene_inputs(scene)
        xp = S["xp"] if "xp" in S else chosen_xp(G["Pf"])
        out = model_system(G, kernels_of(scene, s), S["s%d/lam" % s][0], [tuple(p) for p in S["pairs"]], xp, T, mutant)
        if scene == "counts":
            out["Hpp"] = out["Hpp"][G["mode0_poses"]]
        _model[key] = out
    return _model[key]


LINEAR_SCENES = ("regimes/near", "regimes/moved", "counts")


def model_rows(mutant=None, scenes=LINEAR_SCENES):
    rows = []
    for scene in scenes:
        for s in settings_of(scene):
            rows += [(scene, s) + r for r in compare(scene, s, model_outputs(scene, s, mutant))]
    return rows


def update_errors(q_new, t_new):
    """per case max(|q - q_ref|, |t - t_ref| / (|V upsilon| + |t|))"""
    U = sub("update")
    eq = np.abs(np.asarray(q_new) - U["q_new"]).max(axis=1)
    et = np.abs(np.asarray(t_new) - U["t_new"]).max(axis=1) / U["t_scale"]
    return np.nan_to_num(np.maximum(eq, et), nan=np.inf)


def model_update(T, mutant=None):
    U = sub("update")
    Pf = int(U["sizes"][0])
    new = [model_pose_update(U["xp"][p], U["q"][p], U["t"][p], T, mutant) for p in range(Pf)]
    return np.array([np.asarray(a, dtype=np.float64) for a, _ in new]), np.array([np.asarray(b, dtype=np.float64) for _, b in new])


def model_objective_after(T):
    """sum rho at the model's updated estimate, and the updated landmarks"""
    U = sub("update")
    G = scene_inputs("update")
    qn, tn = model_update(T)
    Xn = (np.asarray(U["X"], dtype=T) + np.asarray(U["xl"], dtype=T)).astype(np.float64)
    G = dict(G, q=np.vstack([qn, U["q"][-1:]]), t=np.vstack([tn, U["t"][-1:]]), X=Xn)
    return model_system(G, kernels_of("update", 0), 1.0, [], None, T)["F"], Xn


def landmark_errors(X_new):
    U = sub("update")
    return np.abs(np.asarray(X_new) - U["X_new"]).max(axis=1) / (np.abs(U["X"]).max(axis=1) + np.abs(U["xl"]).max(axis=1))


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------
def test_the_table_regenerates_bit_for_bit():
    pytest.importorskip("mpmath")
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_reprojection_cases
    new = make_golden_reprojection_cases.generate()          # (its own assertions: every branch and every count is there at least twice)
    with np.load(PATH) as z:
        assert sorted(z.files) == sorted(new)
        for key in z.files:
            assert z[key].dtype == np.asarray(new[key]).dtype and z[key].shape == np.asarray(new[key]).shape and z[key].tobytes() == np.asarray(new[key]).tobytes(), key


def test_the_counts_scene_has_its_counts():
    assert_counts(scene_inputs("counts"))


def test_models_against_the_reference():
    worst = worst_per_regime([r[2:] for r in model_rows()])
    print()
    for reg in MODEL_ERROR:
        err, name, k, _ = worst[reg]
        print("%-28s model error %.1e (%s of block %d)  recorded %.1e  bound fp64 %.1e  fp32 %.1e" % (reg, err, name, k, MODEL_ERROR[reg], bound(reg), bound(reg, "f32")))
    for reg in MODEL_ERROR:
        assert MODEL_ERROR[reg] / 3 <= worst[reg][0] <= 3 * MODEL_ERROR[reg], (reg, worst[reg])


def test_model_sums_and_scalars_against_the_reference():
    """F = sum rho, the largest diagonal entry and the gain-ratio denominator of the model"""
    for scene in LINEAR_SCENES:
        S = sub(scene)
        for s in settings_of(scene):
            m = model_outputs(scene, s)
            Bd, Bs = scene_bounds(scene)
            lam, maxdiag, scale, scale_abs = S["s%d/lam" % s]
            assert abs(m["maxdiag"] - maxdiag) <= Bd * maxdiag
            assert abs(m["F"] - S["s%d/F" % s][0]) <= objective_slack(scene, s, Bd)
            assert abs(m["scale"] - scale) <= Bs * scale_abs, (scene, s, m["scale"], scale, scale_abs)
            assert lam == 2.0 ** round(np.log2(lam)) and 0.5e-4 < lam / maxdiag < 2e-4 and np.float32(lam) == lam


def scene_bounds(scene, precision="f64"):
    """(the largest direct bound, the largest schur bound) of a scene's regimes: what a number that sums over the whole scene is held to"""
    last = scene.split("/")[1] if "/" in scene else "counts"
    return tuple(max(bound(r, precision) for r in MODEL_ERROR if r[-1] == last and r[0] in groups) for groups in (("residual", "direct"), ("schur",)))


def objective_slack(scene, s, B):
    """what sum rho may be off by: per edge B rho (tm.rho_scale) plus the variation of rho over e (1 +- 2 B)"""
    S, G = sub(scene), scene_inputs(scene)
    setting = kernels_of(scene, s)
    tol = 0.0
    for k, e in enumerate(S["e"]):
        kind, delta = setting[1] if G["stereo"][k] else setting[0]
        rho = rf.rho(kind, delta, float(e))
        tol += B * (tm.rho_scale(kind, delta, rho) if kind else rho) + (tm.kernel_window(kind, delta, e, B)[1] if kind else 0.0)
    return tol


def test_kernel_models_against_the_reference():
    """rho' and rho of the model on every side of every threshold (e / delta^2 = 0.25, 1 -+ 1e-9, 4, 1e6)"""
    B, worst = 32 * EPS, 0.0
    for variant in SCENES:
        S = sub("regimes/" + variant)
        for s in (1, 2):
            setting = kernels_of("regimes/" + variant, s)
            for k, e in enumerate(S["e"]):
                kind, delta = setting[1] if S["stereo"][k] else setting[0]
                w, rho = S["s%d/w" % s][k], S["s%d/rho" % s][k]
                dw, dr = tm.kernel_window(kind, delta, e, B)
                ew, er = abs(float(model_weight(kind, delta, np.float64(e))) - w), abs(float(model_rho(kind, delta, np.float64(e))) - rho)
                assert ew <= B * w + dw and er <= B * tm.rho_scale(kind, delta, rho) + dr, (variant, s, k)
                if w > 0 and abs(S["ratio"][k] - 1) > 1e-6:
                    worst = max(worst, ew / w, er / rho)
    print("rho / rho' of the model away from e = delta^2: max rel %.1e" % worst)
    assert worst <= 8 * EPS


def measured_update_errors():
    U = sub("update")
    band = band_of(np.linalg.norm(U["xp"][:, :3], axis=1))
    out = {}
    for prec, T in (("f64", np.float64), ("f32", np.float32)):
        err = update_errors(*model_update(T))
        for b in range(len(BANDS)):
            out[(b, prec)] = float(err[band == b].max())
        F, Xn = model_objective_after(T)
        out[("landmark", prec)] = float(landmark_errors(Xn).max())
        out[("objective", prec)] = abs(F - U["F_new"][0]) / U["F_new"][0]
    return out


def test_update_model_against_the_reference():
    got = measured_update_errors()
    print()
    for b, name in enumerate(BANDS):
        print("%-18s float64 model %.1e (recorded %.1e, bound %.1e)   float32 model %.1e (recorded %.1e, bound %.1e)"
              % (name, got[(b, "f64")], UPDATE_MODEL_ERROR[(b, "f64")], update_bound(b, "f64"), got[(b, "f32")], UPDATE_MODEL_ERROR[(b, "f32")], update_bound(b, "f32")))
    for key in (("landmark", "f64"), ("landmark", "f32"), ("objective", "f64"), ("objective", "f32")):
        print("%-18s %.1e (recorded %.1e)" % (key, got[key], UPDATE_MODEL_ERROR[key]))
    for key, recorded in UPDATE_MODEL_ERROR.items():
        floor = EPS32 if key[1] == "f32" else EPS          # (an error of a rounding or none at all is not held to the factor 3)
        assert got[key] <= 3 * recorded and (recorded / 3 <= got[key] or recorded <= 2 * floor), (key, got[key])
    # the float32 loss of a2 and a3 between 1e-5 and 3.4e-4: two orders above the series branch below it
    assert got[(1, "f32")] > 50 * got[(0, "f32")]


def test_the_update_model_keeps_w_positive_and_the_norm():
    for T, eps in ((np.float64, EPS), (np.float32, EPS32)):
        q, _ = model_update(T)
        assert np.all(q[:, 3] >= 0) and np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 4 * eps


# ---- mutants: the bounds tell a subtly wrong formula from a right one ------------------------------------------------------------------------
LINEAR_MUTANTS = ("stereo JP[2][0] without bf Y / Z^2", "JL from the columns of R", "k02 without d00 d22", "Huber weight delta / e", "Tukey weight u",
                  "65th edge of a pose dropped", "257th edge of a landmark dropped")
UPDATE_MUTANTS = ("a3 = 1 / 6 for every theta", "two Shepperd branches swapped", "no w >= 0 normalisation", "translation te + t")


def test_the_variant_without_a_mutation_is_the_model():
    """mutant = None is the model itself: one code path, and the mutated variants differ from it"""
    a = model_outputs("regimes/near", 1)
    b = model_system(scene_inputs("regimes/near"), kernels_of("regimes/near", 1), sub("regimes/near")["s1/lam"][0], [tuple(p) for p in sub("regimes/near")["pairs"]],
                     sub("regimes/near")["xp"], np.float64, None)
    assert all(np.array_equal(a[k], b[k]) for k in b)
    for T in (np.float64, np.float32):
        q0, t0 = model_update(T)
        q1, t1 = model_update(T, None)
        assert np.array_equal(q0, q1) and np.array_equal(t0, t1)


@pytest.mark.parametrize("name", LINEAR_MUTANTS)
def test_a_mutant_breaks_the_bound(name):
    scenes = ("counts",) if "dropped" in name else ("regimes/near", "regimes/moved")
    caught = [(err / may, scene, s, fam, k) for scene, s, fam, k, reg, err, may in model_rows(name, scenes) if err > may]
    assert caught, name
    ratio, scene, s, fam, k = max(caught)
    print("\n%s: caught by %d blocks, most clearly by %s of block %d (%s, setting %d): %.1e x its bound" % (name, len(caught), fam, k, scene, s, ratio))
    assert ratio > 1e3


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", UPDATE_MUTANTS)
def test_an_update_mutant_breaks_the_bound(name, precision):
    U = sub("update")
    band = band_of(np.linalg.norm(U["xp"][:, :3], axis=1))
    with np.errstate(all="ignore"):          # (a swapped branch divides by its zero pivot)
        err = update_errors(*model_update(np.float32 if precision == "f32" else np.float64, name))
    ratio = np.array([err[p] / update_bound(int(band[p]), precision) for p in range(len(err))])
    assert (ratio > 1).any(), name
    print("\n%s (%s): caught by %d cases, most clearly by case %d (theta %.3g): %.1e x its bound" % (name, precision, (ratio > 1).sum(), ratio.argmax(),
                                                                                                  np.linalg.norm(U["xp"][ratio.argmax(), :3]), ratio.max()))
    assert ratio.max() > 1e3

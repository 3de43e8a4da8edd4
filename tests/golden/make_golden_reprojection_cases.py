"""Generates tests/golden/reprojection_cases.npz: three small bundle-adjustment graphs built edge by edge, and what
tests/reprojection_mp_reference.py (mpmath, 60 digits) makes of them, rounded to fp64.  Data only; needs mpmath and no GPU.  Run from the
repo root: `python tests/golden/make_golden_reprojection_cases.py`.

"regimes/<near|moved>": 24 poses in four groups of six, one group per depth tier (camera-frame Z ~ 0.5, 8, 400, 2e4; a landmark is seen by
    the poses of its own group only, so every landmark, pose and pose pair belongs to one tier), 15 landmarks per group (the last one
    fixed), X / Z of 0 and +-1.5 in the group's first pose, mono and stereo edges mixed, landmarks seen once by a mono edge, a few negated
    quaternions; "moved" is the same graph shifted rigidly by (800, -500, 300).  The measurements are the 60-digit projection minus an
    offset whose length puts e / delta^2 (delta = 1 for mono, 2 for stereo edges) at 0.25, 1 -+ 1e-9, 4 or 1e6; the outputs are recorded
    under the kernel settings (none, none), (Huber, Tukey), (Tukey, Huber) as "<scene>/s<k>/<name>".
"counts": 272 poses and ~200 landmarks with prescribed observation counts (test_reprojection_mp_reference.counts_graph builds the inputs
    from plain IEEE arithmetic; only the outputs are stored), kernels (Huber, Huber).
"update": 64 poses, one increment [omega; upsilon] per free pose (the angles, axes and estimates of UPDATE_THETAS below), three landmarks
    each with increments of 1e-8, 1e-2 and 10, measurements taken at the updated estimate.

Per scene: the inputs the solver takes (q, t, cam, X, eP, eL, stereo, meas, omega, Pf, Lf), lam (a power of two near 1e-4 of the largest
diagonal entry), e per edge, per kernel setting w = rho'(e) (without omega), rho, F = sum rho, and the outputs of reference.system(): Hll,
bl, Hpp, bp, inv, hdiag, bsc (symmetric blocks as their 6 or 21 upper entries), hoff for the listed pairs, xl and scale for the listed xp, each with
`<name>_abs`, the largest sum of absolute terms of the block (float32)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import reprojection_mp_reference as rp  # noqa: E402
import se3_mp_reference as ref  # noqa: E402
import test_reprojection_mp_reference as tr  # noqa: E402

PATH = os.path.join(HERE, "reprojection_cases.npz")
mp, mpf = ref.mp, ref.mpf
SHIFT = np.array([800.0, -500.0, 300.0])
CAM = np.array([500.0, 480.0, 320.0, 240.0, 50.0])
TIERS = (0.5, 8.0, 400.0, 2.0e4)
RATIOS = (0.25, 1 - 1e-9, 0.25, 1 + 1e-9, 0.25, 4.0, 0.25, 0.25, 1e6, 0.25)
DELTA = (1.0, 2.0)          # mono, stereo
SETTINGS = (((rp.NONE, 0.0), (rp.NONE, 0.0)), ((rp.HUBER, DELTA[0]), (rp.TUKEY, DELTA[1])), ((rp.TUKEY, DELTA[0]), (rp.HUBER, DELTA[1])))
NEGATED = (2, 9, 19)
UP, UP3 = np.triu_indices(6), np.triu_indices(3)
TWO_PI_3 = 2 * float(np.pi) / 3
UPDATE_THETAS = (0.0, 1e-9, 0.99e-5, 1.01e-5, 3e-5, 1e-4, 3e-4, 1e-3, 1e-2, 0.25, 1.0, TWO_PI_3 - 1e-6, TWO_PI_3 + 1e-6, 2.5, 2.5, 2.5, 2.5,
                 float(np.pi) - 1e-6, float(np.pi) + 0.5)
UPDATE_AXES = {13: (0.9, 0.3, 0.2), 14: (0.2, 0.9, -0.3), 15: (-0.3, 0.2, 0.9), 16: (0.7, 0.7, 0.1)}


def rot(q):
    return tr.quat_to_rot(np.asarray(q, dtype=np.float64))


def mul(R, v):
    return np.array([R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)])


def power_of_two_near(x):
    return float(2.0 ** int(mp.floor(mp.log(mpf(x), 2) + mp.mpf(1) / 2)))


# ---- scene "regimes" ---------------------------------------------------------------------------------------------------------------------
def regimes_inputs():
    """everything but the measurements: (q, t, X, eP, eL, stereo, omega, ratio, tier of every pose / landmark, Pf, Lf), solver numbering"""
    group_poses = [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 23], [11, 12, 13, 14, 15, 16], [17, 18, 19, 20, 21, 22]]
    q, t, ptier = np.zeros((24, 4)), np.zeros((24, 3)), np.zeros(24, dtype=np.int32)
    for g, poses in enumerate(group_poses):
        base = min(0.05 * TIERS[g], 1.0)
        for k, p in enumerate(poses):
            q[p] = tr.unit([0.1 * g + 0.005 * k, -0.05 + 0.008 * k, 0.2 - 0.004 * k - 0.1 * g, 1.0])
            t[p] = np.array([3.0 - 2.0 * g, 1.0 + g, -4.0 + 3.0 * g]) + k * base * np.array([1.0, 0.3, 0.1])
            ptier[p] = g
    free, fixed, edges = [], [], []          # landmarks as (X, tier); edges as (pose, landmark key, stereo, forced ratio or None)
    for g, poses in enumerate(group_poses):
        R0, t0 = rot(q[poses[0]]), t[poses[0]]
        for j in range(15):
            Z = TIERS[g] * (1 + 0.03 * j)
            Xc = np.array([(0.0, 1.5, -1.5)[j % 3] * Z, (0.0, 0.5, -0.7, 1.1)[j % 4] * Z, Z])
            X = mul(R0.T, Xc - t0)
            key = (g, j)
            (fixed if j == 14 else free).append((key, X, g))
            if j == 0:
                obs = [(k, k % 2 == 1, None) for k in range(6)]
            elif j in (1, 2):
                obs = [(j, False, 0.25)]                                   # seen once by a mono edge: rank-2 Hll
            elif j == 3:
                obs = [(0, True, 4.0), (3, True, 1e6)]                     # weight 0 under Tukey on the stereo edges
            elif j == 5:
                obs = [(1, False, 4.0), (4, False, 1e6)]                   # weight 0 under Tukey on the mono edges
            elif j == 14:
                obs = [(k, k % 2 == 0, None) for k in (0, 2, 3, 4)]        # a fixed landmark: free poses only
            else:
                obs = [((j + d) % 6, (j + d) % 2 == 0, None) for d in (0, 1, 3, 4)[:2 + j % 3]]
            edges += [(poses[k], key, s, ratio) for k, s, ratio in obs]
    lms = free + fixed
    index = {key: n for n, (key, _, _) in enumerate(lms)}
    X = np.array([x for _, x, _ in lms])
    ltier = np.array([g for _, _, g in lms], dtype=np.int32)
    edges.sort(key=lambda e: e[2])          # mono edges first, as flatten() orders them
    eP = np.array([e[0] for e in edges], dtype=np.int32)
    eL = np.array([index[e[1]] for e in edges], dtype=np.int32)
    stereo = np.array([e[2] for e in edges], dtype=bool)
    ratio = np.array([RATIOS[n % len(RATIOS)] if e[3] is None else e[3] for n, e in enumerate(edges)])
    omega = np.array([(1.0, 0.25, 4.0)[n % 3] for n in range(len(edges))])
    q[list(NEGATED)] *= -1.0
    return q, t, X, eP, eL, stereo, omega, ratio, ptier, ltier, 23, len(free)


def offset_direction(n, stereo):
    d = [mpf(x) for x in ((0.6, -0.8, 0.3), (-0.5, 0.4, 0.7), (0.2, 0.9, -0.4))[n % 3][:3 if stereo else 2]]
    norm = mp.sqrt(sum(x * x for x in d))
    return [x / norm for x in d]


def measurements(S, ratio, plain=None):
    """meas with r = projection - meas = s d, omega s^2 = ratio delta^2 (plain: an offset of `plain` pixels instead)"""
    meas = np.zeros((S.E, 3))
    probe = rp.Scene(S.Pf, S.Lf, S.q, S.t, S.cam, S.X, S.eP, S.eL, S.stereo, meas, S.omega)
    for k, (r, _, _, _) in enumerate(rp.geometry(probe)):
        s = mpf(plain[k]) if plain is not None else mpf(DELTA[int(S.stereo[k])]) * mp.sqrt(mpf(ratio[k]) / mpf(S.omega[k]))
        d = offset_direction(k, bool(S.stereo[k]))
        for i in range(len(r)):
            meas[k, i] = float(r[i] - s * d[i])          # (r of the probe is the projection itself)
    return meas


def pack(out, prefix, sysm, names):
    for n in names:
        a = sysm[n]
        s = sysm.get(n + "_abs", np.abs(a))          # ((Hll + lambda I)^-1 is measured against its own largest entry)
        if a.ndim == 3 and n != "hoff":          # symmetric blocks: their upper entries
            a = a[:, UP[0], UP[1]] if a.shape[1] == 6 else a[:, UP3[0], UP3[1]]
        out[prefix + n] = np.ascontiguousarray(a)
        out[prefix + n + "_abs"] = (s.reshape(len(s), -1).max(axis=1) if np.ndim(s) else np.array([s])).astype(np.float32)


def record(out, name, S, settings, pairs, xp, extra=None, jacobian_check=None):
    for key in ("q", "t", "cam", "X", "meas", "omega"):
        out["%s/%s" % (name, key)] = getattr(S, key)
    out[name + "/eP"], out[name + "/eL"], out[name + "/stereo"] = S.eP.astype(np.int32), S.eL.astype(np.int32), S.stereo
    out[name + "/sizes"] = np.array([S.Pf, S.Lf], dtype=np.int32)
    out[name + "/pairs"] = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    out[name + "/xp"] = xp
    geo = rp.geometry(S)
    if jacobian_check:
        for k in jacobian_check:
            bad = rp.check_jacobians(S.q[S.eP[k]], S.t[S.eP[k]], S.cam[S.eP[k]], S.X[S.eL[k]], S.meas[k], bool(S.stereo[k]))
            assert bad < 1e-30, (name, k, bad)          # (h = 1e-25: rounding 1e-60 / h, truncation h^2)
    e = rp.chi(S, geo)
    out[name + "/e"] = rp.fl(e)
    out[name + "/Z"] = rp.fl([g[3][2] for g in geo])
    out[name + "/XZ"] = rp.fl([g[3][0] / g[3][2] for g in geo])
    for s, setting in enumerate(settings):
        w, rho = rp.weights(S, e, setting)
        pre = "%s/s%d/" % (name, s)
        out[pre + "kernels"] = np.array(setting, dtype=np.float64)
        out[pre + "w"] = rp.fl([w[k] / mpf(S.omega[k]) for k in range(S.E)])
        out[pre + "rho"] = rp.fl(rho)
        out[pre + "F"] = np.array([float(sum(rho))])
        lam = power_of_two_near(1e-4 * rp.max_diagonal(S, geo, w))
        sysm = rp.system(S, geo, w, lam, pairs, xp)
        out[pre + "lam"] = np.array([lam, sysm["maxdiag"], sysm["scale"], sysm["scale_abs"]])
        pack(out, pre, sysm, ("Hll", "bl", "Hpp", "bp", "inv", "hdiag", "bsc", "hoff", "xl"))
    if extra:
        for key, v in extra.items():
            out["%s/%s" % (name, key)] = v
    return e


def regimes(out):
    q, t, X, eP, eL, stereo, omega, ratio, ptier, ltier, Pf, Lf = regimes_inputs()
    cam = np.tile(CAM, (24, 1))
    # three pairs per group, among them one with the group's first pose
    pairs = []
    for g0 in (0, 6, 11, 17):
        pairs += [(g0, g0 + 1), (g0 + 1, g0 + 3), (g0 + 2, g0 + 4)]
    for scene in ("near", "moved"):
        if scene == "moved":
            tt = np.array([t[p] - mul(rot(q[p]), SHIFT) for p in range(24)])
            XX = X + SHIFT
        else:
            tt, XX = t, X
        S = rp.Scene(Pf, Lf, q, tt, cam, XX, eP, eL, stereo, np.zeros((len(eP), 3)), omega)
        S.meas = measurements(S, ratio)
        extra = {"ratio": ratio, "ptier": ptier, "ltier": ltier}
        e = record(out, "regimes/" + scene, S, SETTINGS, pairs, tr.chosen_xp(Pf), extra, jacobian_check=range(0, S.E, 7))
        # every branch and every regime is there, at least twice
        x = np.array([float(e[k]) / DELTA[int(stereo[k])] ** 2 for k in range(S.E)])
        assert np.abs(x / ratio - 1).max() < 1e-11
        for r in set(RATIOS):
            for st in (False, True):
                assert ((ratio == r) & (stereo == st)).sum() >= 2, (r, st)
        Z, XZ = out["regimes/%s/Z" % scene], out["regimes/%s/XZ" % scene]
        for g, tier in enumerate(TIERS):
            m = ptier[eP] == g
            assert m.sum() >= 20 and np.all(Z[m] > 0.5 * tier) and np.all(Z[m] < 2.5 * tier)
            assert (np.abs(XZ[m]) > 1.2).sum() >= 2 and (np.abs(XZ[m]) < 0.3).sum() >= 2
        nobs = np.bincount(eL, minlength=len(X))
        assert nobs.max() <= 8 and sum(1 for l in range(Lf) if nobs[l] == 1 and not stereo[eL == l][0]) >= 2
        assert (eL >= Lf).sum() >= 8 and np.all(eP[eL >= Lf] < Pf) and ((eP >= Pf) & (eL < Lf)).sum() >= 2
        assert (q[:, 3] < 0).sum() >= 2 and (np.abs(tt).max() > 500) == (scene == "moved")
        both = [l for l in range(Lf) if stereo[eL == l].any() and (~stereo[eL == l]).any()]
        assert len(both) >= 8
        for s, st in ((1, True), (2, False)):          # landmarks all of whose edges have weight 0, and zero-weight stereo edges
            w = out["regimes/%s/s%d/w" % (scene, s)]
            dead = [l for l in range(Lf) if (eL == l).any() and np.all(w[eL == l] == 0)]
            assert len(dead) >= 2 and ((w == 0) & (stereo == st)).sum() >= 4
            assert np.all(out["regimes/%s/s%d/Hll" % (scene, s)][dead] == 0)


# ---- scene "counts" ----------------------------------------------------------------------------------------------------------------------
def counts(out):
    G = tr.counts_graph()
    S = rp.Scene(G["Pf"], G["Lf"], G["q"], G["t"], G["cam"], G["X"], G["eP"], G["eL"], G["stereo"], G["meas"], G["omega"])
    pairs = [tuple(p) for p in G["listed_pairs"]] + [tuple(p) for p in G["sampled_pairs"]]
    setting = ((rp.HUBER, 1.0), (rp.HUBER, 1.0))
    e = record(out, "counts", S, (setting,), pairs, tr.chosen_xp(S.Pf), jacobian_check=range(0, S.E, 97))
    # (the inputs come from counts_graph(): keep the outputs, the increments and the few numbers the GPU test checks the graph by)
    for key in ("q", "t", "cam", "X", "meas", "omega", "eP", "eL", "stereo", "Z", "XZ", "xp"):
        del out["counts/" + key]
    del out["counts/s0/w"], out["counts/s0/rho"]
    out["counts/checksum"] = np.array([G["meas"].sum(), G["X"].sum(), G["q"].sum(), G["t"].sum()])
    mode0 = G["mode0_poses"]
    out["counts/s0/Hpp"], out["counts/s0/Hpp_abs"] = out["counts/s0/Hpp"][mode0], out["counts/s0/Hpp_abs"][mode0]
    x = rp.fl(e)
    assert (x > 1.0).sum() >= 8 and (x < 1.0).sum() > 0.9 * len(x)
    tr.assert_counts(G)


# ---- scene "update" ----------------------------------------------------------------------------------------------------------------------
def update_plan():
    """per free pose: (q, t, increment [omega; upsilon], nominal theta)"""
    cases = []
    for rep in range(4):
        for n, theta in enumerate(UPDATE_THETAS):
            if rep == 3 and n not in (0, 3, 7, 13, 14, 15):          # 63 cases: a fourth round on six angles
                continue
            c = len(cases)
            axis = tr.unit3(UPDATE_AXES.get(n, ((0.3, -0.5, 0.8), (-0.6, 0.2, 0.5), (0.4, 0.7, -0.3))[c % 3]))
            if rep == 3 and n in (13, 14, 15):          # exactly about x, y, z: any other pivot of the Shepperd branches is 0 here
                axis = np.eye(3)[n - 13]
            w = theta * axis
            size = (1e-3, 1e-2, 0.1, 1.0, 10.0)[c % 5]
            if rep == 1:
                u = size * axis                                                        # omega parallel to upsilon
            elif rep == 0:
                u = size * tr.unit3(np.cross(axis, np.array([0.1, 0.9, 0.4])))         # omega perpendicular to upsilon
            else:
                u = size * tr.unit3(np.array([0.5, -0.3, 0.8]) + 0.1 * (c % 4))
            far = (rep + n) % 2 == 1
            t = np.array([4.0 - 0.3 * n, -2.0 + 0.5 * rep, 6.0 + 0.2 * n]) * (100.0 if far else 1.0)
            if rep == 0:
                q = np.array([0.0, 0.0, 0.0, 1.0]) if n % 2 == 0 else tr.unit([0.2, -0.1, 0.3, 1.0])
            elif rep == 1:
                q = tr.unit([0.1 * (n % 5) - 0.2, 0.3, -0.25, 1.0]) * (-1.0 if n % 2 == 0 else 1.0)
            else:
                q = tr.unit(list(axis) + [0.05])          # nearly a half turn about the increment's axis: the composed w is negative for theta > 0.1
            cases.append((q, t, np.concatenate([w, u]), theta))
    assert len(cases) == 63
    return cases


def update(out):
    cases = update_plan()
    Pf = len(cases)
    q = np.array([c[0] for c in cases] + [tr.unit([0.1, 0.2, -0.1, 1.0])])
    t = np.array([c[1] for c in cases] + [np.array([1.0, 2.0, 3.0])])
    xp = np.array([c[2] for c in cases])
    cam = np.tile(CAM, (Pf + 1, 1))
    camm = [mpf(x) for x in CAM]
    new = [rp.updated_pose(q[p], t[p], xp[p]) for p in range(Pf)]
    poses = [([list(r) for r in ref.quat_rot(qn).tolist()], tn) for qn, tn, _ in new] + [(rp.rotation(q[Pf]), [mpf(x) for x in t[Pf]])]
    X, xl, Xn, eP, eL, meas = [], [], [], [], [], []
    for p in range(Pf + 1):
        R, tn = poses[p]
        for j in range(3):
            Z = (2.0, 8.0, 30.0)[j]
            Xc = [mpf((0.3, -0.8, 0.1)[(p + j) % 3] * Z), mpf((-0.2, 0.4, 0.6)[(p + 2 * j) % 3] * Z), mpf(Z)]
            Xw = [sum(R[k][i] * (Xc[k] - tn[k]) for k in range(3)) for i in range(3)]          # R^T (Xc - t)
            d = (1e-8, 1e-2, 10.0)[(p + j) % 3] * tr.unit3(np.array([0.4, -0.7, 0.5]) + 0.1 * j)
            before = np.array([float(Xw[i] - mpf(d[i])) for i in range(3)])
            after = [mpf(before[i]) + mpf(d[i]) for i in range(3)]
            k = len(eP)
            proj = rp.project(rp.camera_point(R, tn, after), camm, True)
            s = 3.0 if k % 17 == 5 else 0.5
            off = offset_direction(k, True)
            X.append(before), xl.append(d), Xn.append(after), eP.append(p), eL.append(len(X) - 1)
            meas.append([float(proj[i] - mpf(s) * off[i]) for i in range(3)])
    S = rp.Scene(Pf, len(X), q, t, cam, np.array(X), eP, eL, np.ones(len(eP), dtype=bool), np.array(meas), np.ones(len(eP)))
    setting = ((rp.HUBER, 1.0), (rp.HUBER, 1.0))
    e = rp.chi(S, rp.geometry(S, poses, Xn))
    _, rho = rp.weights(S, e, setting)
    pre = "update/"
    for key in ("q", "t", "cam", "X", "meas", "omega"):
        out[pre + key] = getattr(S, key)
    out[pre + "eP"], out[pre + "eL"], out[pre + "stereo"], out[pre + "sizes"] = S.eP.astype(np.int32), S.eL.astype(np.int32), S.stereo, np.array([Pf, S.Lf], dtype=np.int32)
    out[pre + "kernels"] = np.array(setting, dtype=np.float64)
    out[pre + "xp"], out[pre + "xl"] = xp, np.array(xl)
    out[pre + "theta_nominal"] = np.array([c[3] for c in cases])
    out[pre + "q_new"] = np.array([rp.fl(qn) for qn, _, _ in new])
    out[pre + "t_new"] = np.array([rp.fl(tn) for _, tn, _ in new])
    out[pre + "w_composed"] = rp.fl([w for _, _, w in new])
    out[pre + "X_new"] = np.array([rp.fl(x) for x in Xn])
    out[pre + "e_new"], out[pre + "rho_new"], out[pre + "F_new"] = rp.fl(e), rp.fl(rho), np.array([float(sum(rho))])
    # |V upsilon| + |t|: what the error of the translation is measured against
    te = [ref.exp6([mpf(x) for x in xp[p]])[1] for p in range(Pf)]
    out[pre + "t_scale"] = np.array([float(mp.sqrt(sum(te[p][i] ** 2 for i in range(3))) + mp.sqrt(sum(mpf(x) ** 2 for x in t[p]))) for p in range(Pf)])
    # every band, every Shepperd branch and both signs, at least twice
    theta = np.linalg.norm(xp[:, :3], axis=1)
    assert np.abs(theta - out[pre + "theta_nominal"]).max() < 1e-15 * 4
    band = tr.band_of(theta)
    assert all((band == b).sum() >= 2 for b in range(len(tr.BAND_EDGES) + 1))
    branch = tr.shepperd_branch_of(xp[:, :3])
    assert all((branch == b).sum() >= 2 for b in (-1, 0, 1, 2))
    neg = out[pre + "w_composed"] < 0
    assert neg.sum() >= 6 and (~neg).sum() >= 6 and (neg & (q[:Pf, 3] > 0)).sum() >= 2 and (neg & (q[:Pf, 3] < 0)).sum() >= 2
    tn = np.abs(t[:Pf]).max(axis=1)
    assert (tn > 300).sum() >= 10 and (tn < 30).sum() >= 10
    assert all(np.isclose(np.abs(np.array(xl)).max(axis=1) / s, 1, atol=0.5).sum() >= 10 for s in (1e-8, 1e-2, 10.0))
    assert np.all(np.abs(out[pre + "X_new"] - (S.X + np.array(xl))) <= 1e-12 * np.abs(out[pre + "X_new"]))


def generate():
    out = {}
    regimes(out)
    counts(out)
    update(out)
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(PATH, **data)
    print(PATH, len(data), "arrays,", os.path.getsize(PATH), "bytes")

"""numpy fp64 model of the direction factors on the poses (cuba_hip_set_direction_factors) -- TEST INFRASTRUCTURE.

A factor on pose T = [R | t] (world -> camera, quaternion (x, y, z, w)) with a world vector d, the same vector as measured in the camera
frame, m (neither normalised), information Omega (3 x 3, symmetric, rank 2 as a rule) and robust kernel (kind, delta) of the pose factors'
family has the residual r = R d - m, e = r^T Omega r and the objective term rho(e).  Under the solver's update T <- exp(delta) T,
delta = [omega; upsilon], R' = (I + [omega]x) R to first order, so

    r' = r + omega x (R d),     dr/ddelta = [-[R d]x | 0]   (3 x 6)

exactly to first order: r lives in a vector space and needs no J_l, and the translation columns are zero.  (The body-frame form -R [d]x
equals -[R d]x R: wrong unless R = I.)  It is linearised with w = rho'(e) and no second-order term: Hpp += w J^T Omega J,
b_p -= w J^T Omega r (b = minus half the gradient, the convention of the dense system).

A set is (pose[n], d[n, 3], m[n, 3], info[n, 3, 3], kind[n] or None, delta[n] or None) as HipSolver.set_direction_factors takes it, poses
in the solver numbering (free ones first).  dense_lm() is the library's Levenberg-Marquardt loop as in position_factor_reference.dense_lm
on the dense normal equations of the oracle plus the pose factors', landmark priors' and position factors' terms
(position_factor_reference) plus these: all five kinds in one system."""
import numpy as np

import position_factor_reference as pfr
import prior_reference as pr
import robust_pose_factor_reference as rf
from oracle import oracle


def kernel_of(df, k):
    return (rf.NONE, 0.0) if df[4] is None else (int(df[4][k]), float(df[5][k]))


def residual(q, d, m):
    """r = R d - m"""
    R = oracle.quat_to_rot(np.asarray(q, dtype=np.float64))
    return R @ np.asarray(d, dtype=np.float64) - np.asarray(m, dtype=np.float64)


def jacobian(q, d, body_frame=False):
    """dr/ddelta = [-[R d]x | 0]; body_frame = True gives -R [d]x in the rotation columns (the WRONG Jacobian the tests are sized against)"""
    R = oracle.quat_to_rot(np.asarray(q, dtype=np.float64))
    d = np.asarray(d, dtype=np.float64)
    J = np.zeros((3, 6))
    J[:, :3] = -R @ pr.hat(d) if body_frame else -pr.hat(R @ d)
    return J


def factor_terms(df, q, Pf, body_frame=False):
    """per factor (e, rho, w, pose, J, Omega, r) at the estimate q[Pt, 4]; a factor on a fixed pose: (0, 0, 0, p, None, None, None)"""
    out = []
    for k in range(len(df[0])):
        p = int(df[0][k])
        if p >= Pf:
            out.append((0.0, 0.0, 0.0, p, None, None, None))
            continue
        Om = np.asarray(df[3][k], dtype=np.float64).reshape(3, 3)
        Om = 0.5 * (Om + Om.T)
        r = residual(q[p], df[1][k], df[2][k])
        e = float(r @ Om @ r)
        kind, delta = kernel_of(df, k)
        out.append((e, float(rf.rho(kind, delta, e)), float(rf.weight(kind, delta, e)), p, jacobian(q[p], df[1][k], body_frame), Om, r))
    return out


def factor_chi2(df, q, Pf):
    """the plain e of every factor"""
    return np.array([x[0] for x in factor_terms(df, q, Pf)])


def factor_objective(df, q, Pf):
    """sum of rho(e)"""
    return float(sum(x[1] for x in factor_terms(df, q, Pf)))


def factor_system(df, q, Pf, body_frame=False):
    """the factors' part of the dense (6 Pf)^2 pose system: H = sum w J^T Omega J and b = -sum w J^T Omega r, in the set's order"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for _, _, w, p, J, Om, r in factor_terms(df, q, Pf, body_frame):
        if J is None:
            continue
        s = slice(6 * p, 6 * p + 6)
        H[s, s] += w * (J.T @ Om @ J)
        b[s] -= w * (J.T @ Om @ r)
    return H, b


def objective(o, fp, df, pf=None, lmp=None, priors=None, rel=None, kp=None, kr=None):
    F = pfr.objective(o, fp, pf, lmp=lmp, priors=priors, rel=rel, kp=kp, kr=kr)
    if df is not None:
        F += factor_objective(df, o.state()[0], fp.Pf)
    return F


def system(o, fp, df, lam, pf=None, lmp=None, priors=None, rel=None, kp=None, kr=None, body_frame=False):
    """(H + lam I, b) of reprojection edges, pose factors, landmark priors, position factors and direction factors at the oracle's
    current estimate"""
    H, b = pfr.system(o, fp, pf, lam, lmp=lmp, priors=priors, rel=rel, kp=kp, kr=kr)
    if df is not None:
        Hd, bd = factor_system(df, o.state()[0], fp.Pf, body_frame)
        n = 6 * fp.Pf
        H[:n, :n] += Hd
        b[:n] += bd
    return H, b


def gradient(o, fp, df, **others):
    """b at lambda = 0: minus half the gradient of the Gauss-Newton model of F (always with the right Jacobian)"""
    others.pop("body_frame", None)
    return system(o, fp, df, 0.0, **others)[1]


def dense_lm(o, fp, df, niter, **others):
    """the library's LM loop on the dense system; returns dict(chi2 per iteration, lambdas, rejected = trials rejected in all,
    gains = the gain ratio of every trial).  others: pf, lmp, priors, rel, kp, kr, and body_frame (True: the system is built with the wrong
    Jacobian; the objective is the true one)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams, rejected, gains = 2.0, 0.0, [], [], 0, []
    obj = {k: v for k, v in others.items() if k != "body_frame"}
    F = objective(o, fp, df, **obj)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, df, 0.0, **others)
            lam = tau * float(np.max(np.diag(H0)))
        qn, gain = 0, -1.0
        while qn < maxq and gain < 0:
            H, b = system(o, fp, df, lam, **others)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, fp, df, **obj)
            scale = float(x @ (lam * x + b)) + 1e-3
            gain = (F - Fhat) / scale if ok else -1.0
            gains.append(gain)
            qn += 1
            if gain > 0:
                lam *= max(1.0 / 3, min(1 - (2 * gain - 1) ** 3, 2.0 / 3))
                nu = 2.0
                F = Fhat
                break
            rejected += 1
            lam *= nu
            nu *= 2
            o.set_state(*saved)
        chi2.append(F)
        lams.append(lam)
        if qn == maxq or gain <= 0 or not np.isfinite(lam):
            break
    return dict(chi2=np.array(chi2), lambdas=np.array(lams), rejected=rejected, gains=np.array(gains))


def make_factors(fp, poses, seed, sigma=0.05, kind=None, delta=None, rank2=False):
    """factors on `poses`: unit world vectors d, measurements m = R(q0[p]) d + sigma * N(0, 1), normalised, information
    400 I + 100 A A^T (rank2: projected by I - m m^T on both sides); kind / delta: one kernel for all, or None.  Draws, in this order, from
    default_rng(seed): d = N(0, 1) [n, 3] (normalised per row), the noise [n, 3], then per factor A [3, 3]."""
    rng = np.random.default_rng(seed)
    poses = np.asarray(poses, dtype=np.int32)
    n = len(poses)
    q0 = np.asarray(fp.q, dtype=np.float64).reshape(-1, 4)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    noise = sigma * rng.normal(size=(n, 3))
    m = np.array([oracle.quat_to_rot(q0[p]) @ d[k] for k, p in enumerate(poses)]).reshape(n, 3) + noise
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    info = np.empty((n, 3, 3))
    for k in range(n):
        A = rng.normal(size=(3, 3))
        info[k] = 400.0 * np.eye(3) + 100.0 * (A @ A.T)
        if rank2:
            P = np.eye(3) - np.outer(m[k], m[k])
            info[k] = P @ info[k] @ P
    if kind is None:
        return poses, d, m, info, None, None
    return poses, d, m, info, np.full(n, kind, dtype=np.int32), np.full(n, float(delta))

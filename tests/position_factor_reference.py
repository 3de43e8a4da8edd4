"""numpy fp64 model of the position factors on the poses (cuba_hip_set_position_factors) -- TEST INFRASTRUCTURE.

A factor on pose T = [R | t] (world -> camera, quaternion (x, y, z, w)) with measured world position z, lever arm a (the measured point in
the camera frame; zero: the camera centre), information Omega (3 x 3, symmetric) and robust kernel (kind, delta) of the pose factors'
family has the residual r = R^T (a - t) - z, e = r^T Omega r and the objective term rho(e).  Under the solver's update T <- exp(d) T,
d = [omega; upsilon], R' = (I + [omega]x) R and t' = t + omega x t + upsilon to first order, so

    r' = R^T (I - [omega]x) (a - t - omega x t - upsilon) - z = r + R^T [a]x omega - R^T upsilon,     dr/dd = [R^T [a]x | -R^T]   (3 x 6)

exactly to first order: r lives in a vector space and needs no J_l.  It is linearised with w = rho'(e) and no second-order term:
Hpp += w J^T Omega J, b_p -= w J^T Omega r (b = minus half the gradient, the convention of the dense system).

A set is (pose[n], z[n, 3], info[n, 3, 3], arm[n, 3] or None, kind[n] or None, delta[n] or None) as HipSolver.set_position_factors takes
it, poses in the solver numbering (free ones first).  dense_lm() is the library's Levenberg-Marquardt loop as in
landmark_prior_reference.dense_lm (tau = 1e-5, <= 10 trials, g2o's rho / lambda rules, scale += 1e-3) on the dense normal equations of
the oracle plus the pose factors' and landmark priors' terms (landmark_prior_reference) plus these."""
import numpy as np

import landmark_prior_reference as lr
import prior_reference as pr
import robust_pose_factor_reference as rf
from oracle import oracle


def kernel_of(pf, k):
    return (rf.NONE, 0.0) if pf[4] is None else (int(pf[4][k]), float(pf[5][k]))


def arm_of(pf, k):
    return np.zeros(3) if pf[3] is None else np.asarray(pf[3][k], dtype=np.float64)


def residual(q, t, a, z):
    """r = R^T (a - t) - z"""
    R = oracle.quat_to_rot(np.asarray(q, dtype=np.float64))
    return R.T @ (np.asarray(a, dtype=np.float64) - np.asarray(t, dtype=np.float64)) - np.asarray(z, dtype=np.float64)


def jacobian(q, a, rotation_column=True):
    """dr/dd = [R^T [a]x | -R^T]; rotation_column = False drops the first block (the WRONG Jacobian the optimality test is sized against)"""
    R = oracle.quat_to_rot(np.asarray(q, dtype=np.float64))
    J = np.zeros((3, 6))
    if rotation_column:
        J[:, :3] = R.T @ pr.hat(np.asarray(a, dtype=np.float64))
    J[:, 3:] = -R.T
    return J


def factor_terms(pf, q, t, Pf, rotation_column=True):
    """per factor (e, rho, w, pose, J, Omega, r) at the estimate (q[Pt, 4], t[Pt, 3]); a factor on a fixed pose: (0, 0, 0, p, None, None, None)"""
    out = []
    for k in range(len(pf[0])):
        p = int(pf[0][k])
        if p >= Pf:
            out.append((0.0, 0.0, 0.0, p, None, None, None))
            continue
        Om = np.asarray(pf[2][k], dtype=np.float64).reshape(3, 3)
        Om = 0.5 * (Om + Om.T)
        a = arm_of(pf, k)
        r = residual(q[p], t[p], a, pf[1][k])
        e = float(r @ Om @ r)
        kind, delta = kernel_of(pf, k)
        out.append((e, float(rf.rho(kind, delta, e)), float(rf.weight(kind, delta, e)), p, jacobian(q[p], a, rotation_column), Om, r))
    return out


def factor_chi2(pf, q, t, Pf):
    """the plain e of every factor"""
    return np.array([x[0] for x in factor_terms(pf, q, t, Pf)])


def factor_objective(pf, q, t, Pf):
    """sum of rho(e)"""
    return float(sum(x[1] for x in factor_terms(pf, q, t, Pf)))


def factor_system(pf, q, t, Pf, rotation_column=True):
    """the factors' part of the dense (6 Pf)^2 pose system: H = sum w J^T Omega J and b = -sum w J^T Omega r, in the set's order"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for _, _, w, p, J, Om, r in factor_terms(pf, q, t, Pf, rotation_column):
        if J is None:
            continue
        s = slice(6 * p, 6 * p + 6)
        H[s, s] += w * (J.T @ Om @ J)
        b[s] -= w * (J.T @ Om @ r)
    return H, b


def objective(o, fp, pf, lmp=None, priors=None, rel=None, kp=None, kr=None):
    F = lr.objective(o, fp, lmp, priors=priors, rel=rel, kp=kp, kr=kr)
    if pf is not None:
        q, t, _ = o.state()
        F += factor_objective(pf, q, t, fp.Pf)
    return F


def system(o, fp, pf, lam, lmp=None, priors=None, rel=None, kp=None, kr=None, rotation_column=True):
    """(H + lam I, b) of reprojection edges, pose factors, landmark priors and position factors at the oracle's current estimate"""
    H, b = lr.system(o, fp, lmp, lam, priors=priors, rel=rel, kp=kp, kr=kr)
    if pf is not None:
        q, t, _ = o.state()
        Hp, bp = factor_system(pf, q, t, fp.Pf, rotation_column)
        n = 6 * fp.Pf
        H[:n, :n] += Hp
        b[:n] += bp
    return H, b


def gradient(o, fp, pf, **others):
    """b at lambda = 0: minus half the gradient of the Gauss-Newton model of F (always with the full Jacobian)"""
    others.pop("rotation_column", None)
    return system(o, fp, pf, 0.0, **others)[1]


def dense_lm(o, fp, pf, niter, **others):
    """the library's LM loop on the dense system; returns dict(chi2 per iteration, lambdas, rejected = trials rejected in all,
    gains = the gain ratio of every trial).  others: lmp, priors, rel, kp, kr, and rotation_column (False: the system is built with the
    wrong Jacobian; the objective is the true one)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams, rejected, gains = 2.0, 0.0, [], [], 0, []
    obj = {k: v for k, v in others.items() if k != "rotation_column"}
    F = objective(o, fp, pf, **obj)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, pf, 0.0, **others)
            lam = tau * float(np.max(np.diag(H0)))
        qn, gain = 0, -1.0
        while qn < maxq and gain < 0:
            H, b = system(o, fp, pf, lam, **others)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, fp, pf, **obj)
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


def make_factors(fp, poses, seed, sigma=0.2, arm=0.5, kind=None, delta=None):
    """factors on `poses`: lever arms arm * N(0, 1), fixes sigma * N(0, 1) off the antenna's position at the current estimate, information
    50 I + 20 A A^T; kind / delta: one kernel for all, or None.  Draws, in this order, from default_rng(seed): the arms [n, 3], the noise
    [n, 3], then per factor A [3, 3]."""
    rng = np.random.default_rng(seed)
    poses = np.asarray(poses, dtype=np.int32)
    n = len(poses)
    q0, t0 = np.asarray(fp.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp.t, dtype=np.float64).reshape(-1, 3)
    arms = arm * rng.normal(size=(n, 3))
    noise = sigma * rng.normal(size=(n, 3))
    z = np.array([oracle.quat_to_rot(q0[p]).T @ (arms[k] - t0[p]) for k, p in enumerate(poses)]).reshape(n, 3) + noise
    info = np.empty((n, 3, 3))
    for k in range(n):
        A = rng.normal(size=(3, 3))
        info[k] = 50.0 * np.eye(3) + 20.0 * (A @ A.T)
    if kind is None:
        return poses, z, info, arms, None, None
    return poses, z, info, arms, np.full(n, kind, dtype=np.int32), np.full(n, float(delta))

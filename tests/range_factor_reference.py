"""numpy fp64 model of the range factors on the poses (cuba_hip_set_range_factors) -- TEST INFRASTRUCTURE.

A factor on pose T = [R | t] (world -> camera, quaternion (x, y, z, w)) with an anchor b (a known world point), a measured range rbar, a
lever arm a (the ranging antenna in the camera frame; zero: the camera centre), a scalar information Omega = 1 / sigma^2 and robust kernel
(kind, delta) of the pose factors' family has

    u = (a - t) - R b   (camera frame; |u| = |R^T (a - t) - b|),   rho = |u|,   m = u / rho,   r = rho - rbar,   e = Omega r^2

and the objective term rho_k(e).  Under the solver's update T <- exp(d) T, d = [omega; upsilon], the anchor in the camera frame
b_c = R b + t becomes b_c + omega x b_c + upsilon to first order, so d rho = -m . (omega x b_c + upsilon); with b_c = a - rho m,
b_c x m = a x m and

    dr/dd = J = [(m x a)^T | -m^T]   (1 x 6)

It is linearised with w = rho_k'(e) and no second-order term: Hpp += w Omega J^T J (rank 1), b_p -= w Omega r J^T (b = minus half the
gradient, the convention of the dense system).  THE POINT rho = 0 (the antenna at the anchor): m is undefined; the rule, the library's, is
m = 0 when the computed rho is exactly 0, so J = 0: the factor adds nothing to H or b and e = Omega rbar^2.

A set is (pose[n], anchor[n, 3], range[n], info[n], arm[n, 3] or None, kind[n] or None, delta[n] or None) as HipSolver.set_range_factors
takes it, poses in the solver numbering (free ones first).  dense_lm() is the library's Levenberg-Marquardt loop as in
direction_factor_reference.dense_lm on the dense normal equations of the oracle plus the terms of every other kind of factor
(direction_factor_reference) plus these: all six kinds in one system."""
import numpy as np

import direction_factor_reference as dfr
import prior_reference as pr
import robust_pose_factor_reference as rf
from oracle import oracle

RIGHT, WORLD_DIRECTION, NO_ROTATION = "right", "world_direction", "no_rotation"


def kernel_of(rs, k):
    return (rf.NONE, 0.0) if rs[5] is None else (int(rs[5][k]), float(rs[6][k]))


def arm_of(rs, k):
    return np.zeros(3) if rs[4] is None else np.asarray(rs[4][k], dtype=np.float64)


def direction(q, t, a, b):
    """(rho, m): u = (a - t) - R b, rho = |u|, m = u / rho, or 0 when the computed rho is exactly 0"""
    R = oracle.quat_to_rot(np.asarray(q, dtype=np.float64))
    u = (np.asarray(a, dtype=np.float64) - np.asarray(t, dtype=np.float64)) - R @ np.asarray(b, dtype=np.float64)
    rho = float(np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))
    return rho, (u / rho if rho > 0 else np.zeros(3))


def residual(q, t, a, b, rbar):
    """r = |a - t - R b| - rbar"""
    return direction(q, t, a, b)[0] - float(rbar)


def jacobian(q, t, a, b, variant=RIGHT):
    """dr/dd = [(m x a)^T | -m^T] (6,).  The WRONG variants the optimality test is sized against: WORLD_DIRECTION puts the world-frame
    direction R^T m in place of m, NO_ROTATION drops the rotation columns (right only for a = 0)"""
    _, m = direction(q, t, a, b)
    a = np.asarray(a, dtype=np.float64)
    if variant == WORLD_DIRECTION:
        m = oracle.quat_to_rot(np.asarray(q, dtype=np.float64)).T @ m
    J = np.concatenate([np.cross(m, a), -m])
    if variant == NO_ROTATION:
        J[:3] = 0
    return J


def factor_terms(rs, q, t, Pf, variant=RIGHT):
    """per factor (e, rho_k, w, pose, J, Omega, r) at the estimate (q[Pt, 4], t[Pt, 3]); a factor on a fixed pose: (0, 0, 0, p, None, None, None)"""
    out = []
    for k in range(len(rs[0])):
        p = int(rs[0][k])
        if p >= Pf:
            out.append((0.0, 0.0, 0.0, p, None, None, None))
            continue
        Om = float(rs[3][k])
        a = arm_of(rs, k)
        r = residual(q[p], t[p], a, rs[1][k], rs[2][k])
        e = Om * r * r
        kind, delta = kernel_of(rs, k)
        out.append((e, float(rf.rho(kind, delta, e)), float(rf.weight(kind, delta, e)), p, jacobian(q[p], t[p], a, rs[1][k], variant), Om, r))
    return out


def factor_chi2(rs, q, t, Pf):
    """the plain e of every factor"""
    return np.array([x[0] for x in factor_terms(rs, q, t, Pf)])


def factor_objective(rs, q, t, Pf):
    """sum of rho_k(e)"""
    return float(sum(x[1] for x in factor_terms(rs, q, t, Pf)))


def factor_system(rs, q, t, Pf, variant=RIGHT):
    """the factors' part of the dense (6 Pf)^2 pose system: H = sum w Omega J^T J and b = -sum w Omega r J^T, in the set's order"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for _, _, w, p, J, Om, r in factor_terms(rs, q, t, Pf, variant):
        if J is None:
            continue
        s = slice(6 * p, 6 * p + 6)
        H[s, s] += np.outer(J, (w * Om) * J)
        b[s] -= ((w * Om) * J) * r
    return H, b


def objective(o, fp, rs, **others):
    """others: df, pf, lmp, priors, rel, kp, kr"""
    others = dict(others)
    F = dfr.objective(o, fp, others.pop("df", None), **others)
    if rs is not None:
        q, t, _ = o.state()
        F += factor_objective(rs, q, t, fp.Pf)
    return F


def system(o, fp, rs, lam, variant=RIGHT, **others):
    """(H + lam I, b) of reprojection edges and all six kinds of factor at the oracle's current estimate"""
    others = dict(others)
    H, b = dfr.system(o, fp, others.pop("df", None), lam, **others)
    if rs is not None:
        q, t, _ = o.state()
        Hr, br = factor_system(rs, q, t, fp.Pf, variant)
        n = 6 * fp.Pf
        H[:n, :n] += Hr
        b[:n] += br
    return H, b


def gradient(o, fp, rs, **others):
    """b at lambda = 0: minus half the gradient of the Gauss-Newton model of F (always with the right Jacobian)"""
    others.pop("variant", None)
    return system(o, fp, rs, 0.0, **others)[1]


def dense_lm(o, fp, rs, niter, **others):
    """the library's LM loop on the dense system; returns dict(chi2 per iteration, lambdas, rejected = trials rejected in all,
    gains = the gain ratio of every trial).  others: df, pf, lmp, priors, rel, kp, kr, and variant (a wrong one: the system is built with
    the wrong Jacobian; the objective is the true one)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams, rejected, gains = 2.0, 0.0, [], [], 0, []
    obj = {k: v for k, v in others.items() if k != "variant"}
    F = objective(o, fp, rs, **obj)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, rs, 0.0, **others)
            lam = tau * float(np.max(np.diag(H0)))
        qn, gain = 0, -1.0
        while qn < maxq and gain < 0:
            H, b = system(o, fp, rs, lam, **others)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, fp, rs, **obj)
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


def antenna(fp, p, a):
    """the world position R^T (a - t) of the point a of pose p's camera frame at the graph's initial estimate"""
    q0, t0 = np.asarray(fp.q, dtype=np.float64).reshape(-1, 4), np.asarray(fp.t, dtype=np.float64).reshape(-1, 3)
    return oracle.quat_to_rot(q0[p]).T @ (np.asarray(a, dtype=np.float64) - t0[p])


def make_factors(fp, poses, seed, anchors=4, span=8.0, sigma=0.1, arm=0.3, info=100.0, kind=None, delta=None):
    """factors on `poses`, factor k to anchor k % anchors: the anchors span * N(0, 1) about the centroid of the antennas (ranges of metres,
    non-coplanar with probability 1), lever arms arm * N(0, 1), ranges = the distance at the current estimate + sigma * N(0, 1) (absolute
    value), information info * (1 + U(0, 1)); kind / delta: one kernel for all, or None.  Draws, in this order, from default_rng(seed): the
    arms [n, 3], the anchors [anchors, 3], the noise [n], the informations [n]."""
    rng = np.random.default_rng(seed)
    poses = np.asarray(poses, dtype=np.int32)
    n = len(poses)
    arms = arm * rng.normal(size=(n, 3))
    ant = np.array([antenna(fp, p, arms[k]) for k, p in enumerate(poses)]).reshape(n, 3)
    centre = ant.mean(axis=0) if n else np.zeros(3)
    A = centre + span * rng.normal(size=(anchors, 3))
    b = A[np.arange(n) % anchors]
    rng_m = np.abs(np.linalg.norm(ant - b, axis=1) + sigma * rng.normal(size=n))
    Om = info * (1.0 + rng.uniform(size=n))
    if kind is None:
        return poses, b, rng_m, Om, arms, None, None
    return poses, b, rng_m, Om, arms, np.full(n, kind, dtype=np.int32), np.full(n, float(delta))

"""numpy fp64 model of the range factors between two poses (cuba_hip_set_pose_range_factors) -- TEST INFRASTRUCTURE.

A factor between the poses T_i = [R_i | t_i] and T_j = [R_j | t_j] (world -> camera, quaternion (x, y, z, w)), i != j, with lever arms
a_i, a_j (a point in each camera frame; zero: the camera centre), a measured distance rbar, a scalar information Omega = 1 / sigma^2 and a
robust kernel (kind, delta) of the pose factors' family has

    w_i = R_i^T (a_i - t_i)             the world position of the point on pose i
    u   = (a_j - t_j) - R_j w_i         frame j: the unary range factor (range_factor_reference) on pose j with the anchor b = w_i
    rho = |u|,  m_j = u / rho,  m_i = -R_i R_j^T m_j,   r = rho - rbar,   e = Omega r^2

and the objective term rho_k(e).  Under the solver's update T <- exp(d) T, d = [omega; upsilon], each end sees the other end's point as a
fixed anchor to first order, so

    dr/dd_j = J_j = [(m_j x a_j)^T | -m_j^T]      dr/dd_i = J_i = [(m_i x a_i)^T | -m_i^T]      (1 x 6 each)

It is linearised with w = rho_k'(e) and no second-order term: H_ii += w Omega J_i^T J_i, H_jj += w Omega J_j^T J_j, H_ij += w Omega
J_i^T J_j (and its transpose), b_i -= w Omega r J_i^T, b_j -= w Omega r J_j^T.  THE POINT rho = 0: when the computed rho is exactly 0,
m_i = m_j = 0 (both from the one computed u), so the factor adds nothing to H or b and e = Omega rbar^2.  One end fixed: the factor acts
on the free end only; both fixed: it is ignored, e = 0.

A set is (pose_i[n], pose_j[n], range[n], info[n], arm_i[n, 3] or None, arm_j[n, 3] or None, kind[n] or None, delta[n] or None) as
HipSolver.set_pose_range_factors takes it, poses in the solver numbering (free ones first).  dense_lm() is range_factor_reference.dense_lm
with these terms added: all seven kinds in one system."""
import numpy as np

import range_factor_reference as rr
import prior_reference as pr
import robust_pose_factor_reference as rf
from oracle import oracle

RIGHT, WORLD_DIRECTION, NO_ROTATION, WRONG_SIGN = "right", "world_direction", "no_rotation", "wrong_sign"


def kernel_of(ps, k):
    return (rf.NONE, 0.0) if ps[6] is None else (int(ps[6][k]), float(ps[7][k]))


def arms_of(ps, k):
    return (np.zeros(3) if ps[4] is None else np.asarray(ps[4][k], dtype=np.float64),
            np.zeros(3) if ps[5] is None else np.asarray(ps[5][k], dtype=np.float64))


def directions(qi, ti, qj, tj, ai, aj):
    """(rho, m_i, m_j) from the one u; all-zero directions when the computed rho is exactly 0"""
    Ri, Rj = oracle.quat_to_rot(np.asarray(qi, dtype=np.float64)), oracle.quat_to_rot(np.asarray(qj, dtype=np.float64))
    w = Ri.T @ (np.asarray(ai, dtype=np.float64) - np.asarray(ti, dtype=np.float64))
    u = (np.asarray(aj, dtype=np.float64) - np.asarray(tj, dtype=np.float64)) - Rj @ w
    rho = float(np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))
    mj = u / rho if rho > 0 else np.zeros(3)
    return rho, -(Ri @ (Rj.T @ mj)), mj


def residual(qi, ti, qj, tj, ai, aj, rbar):
    return directions(qi, ti, qj, tj, ai, aj)[0] - float(rbar)


def jacobians(qi, ti, qj, tj, ai, aj, variant=RIGHT):
    """(J_i, J_j), (6,) each.  The WRONG variants the optimality test is sized against: WORLD_DIRECTION puts the world-frame directions
    R^T m in place of the camera-frame ones, NO_ROTATION drops the rotation columns (right only for zero arms), WRONG_SIGN takes m_i with
    the opposite sign (the direction of end j carried over without turning it round)"""
    _, mi, mj = directions(qi, ti, qj, tj, ai, aj)
    if variant == WORLD_DIRECTION:
        mi = oracle.quat_to_rot(np.asarray(qi, dtype=np.float64)).T @ mi
        mj = oracle.quat_to_rot(np.asarray(qj, dtype=np.float64)).T @ mj
    if variant == WRONG_SIGN:
        mi = -mi
    Ji = np.concatenate([np.cross(mi, np.asarray(ai, dtype=np.float64)), -mi])
    Jj = np.concatenate([np.cross(mj, np.asarray(aj, dtype=np.float64)), -mj])
    if variant == NO_ROTATION:
        Ji[:3] = 0
        Jj[:3] = 0
    return Ji, Jj


def factor_terms(ps, q, t, Pf, variant=RIGHT):
    """per factor (e, rho_k, w, i, j, J_i, J_j, Omega, r) at the estimate (q[Pt, 4], t[Pt, 3]); both ends fixed: zeros and None"""
    out = []
    for k in range(len(ps[0])):
        i, j = int(ps[0][k]), int(ps[1][k])
        if i >= Pf and j >= Pf:
            out.append((0.0, 0.0, 0.0, i, j, None, None, None, None))
            continue
        Om = float(ps[3][k])
        ai, aj = arms_of(ps, k)
        r = residual(q[i], t[i], q[j], t[j], ai, aj, ps[2][k])
        e = Om * r * r
        kind, delta = kernel_of(ps, k)
        Ji, Jj = jacobians(q[i], t[i], q[j], t[j], ai, aj, variant)
        out.append((e, float(rf.rho(kind, delta, e)), float(rf.weight(kind, delta, e)), i, j, Ji, Jj, Om, r))
    return out


def factor_chi2(ps, q, t, Pf):
    """the plain e of every factor"""
    return np.array([x[0] for x in factor_terms(ps, q, t, Pf)])


def factor_objective(ps, q, t, Pf):
    """sum of rho_k(e)"""
    return float(sum(x[1] for x in factor_terms(ps, q, t, Pf)))


def factor_system(ps, q, t, Pf, variant=RIGHT):
    """the factors' part of the dense (6 Pf)^2 pose system, in the set's order; a fixed end has no rows"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for _, _, w, i, j, Ji, Jj, Om, r in factor_terms(ps, q, t, Pf, variant):
        if Ji is None:
            continue
        ends = [(p, J) for p, J in ((i, Ji), (j, Jj)) if p < Pf]
        for p, J in ends:
            s = slice(6 * p, 6 * p + 6)
            H[s, s] += np.outer(J, (w * Om) * J)
            b[s] -= J * ((w * Om) * r)
        if len(ends) == 2:
            si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
            X = np.outer(Ji, (w * Om) * Jj)
            H[si, sj] += X
            H[sj, si] += X.T
    return H, b


def objective(o, fp, ps, **others):
    """others: rs, df, pf, lmp, priors, rel, kp, kr"""
    others = dict(others)
    F = rr.objective(o, fp, others.pop("rs", None), **others)
    if ps is not None:
        q, t, _ = o.state()
        F += factor_objective(ps, q, t, fp.Pf)
    return F


def system(o, fp, ps, lam, variant=RIGHT, **others):
    """(H + lam I, b) of reprojection edges and all seven kinds of factor at the oracle's current estimate"""
    others = dict(others)
    H, b = rr.system(o, fp, others.pop("rs", None), lam, **others)
    if ps is not None:
        q, t, _ = o.state()
        Hr, br = factor_system(ps, q, t, fp.Pf, variant)
        n = 6 * fp.Pf
        H[:n, :n] += Hr
        b[:n] += br
    return H, b


def gradient(o, fp, ps, **others):
    """b at lambda = 0: minus half the gradient of the Gauss-Newton model of F (always with the right Jacobian)"""
    others.pop("variant", None)
    return system(o, fp, ps, 0.0, **others)[1]


def dense_lm(o, fp, ps, niter, **others):
    """the library's LM loop on the dense system, as range_factor_reference.dense_lm; others: rs, df, pf, lmp, priors, rel, kp, kr, and
    variant (a wrong one: the system is built with the wrong Jacobian; the objective is the true one)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams, rejected, gains = 2.0, 0.0, [], [], 0, []
    obj = {k: v for k, v in others.items() if k != "variant"}
    F = objective(o, fp, ps, **obj)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, ps, 0.0, **others)
            lam = tau * float(np.max(np.diag(H0)))
        qn, gain = 0, -1.0
        while qn < maxq and gain < 0:
            H, b = system(o, fp, ps, lam, **others)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, fp, ps, **obj)
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


def make_factors(fp, pairs, seed, sigma=0.05, arm=0.3, info=100.0, kind=None, delta=None):
    """factors on `pairs` [n, 2]: lever arms arm * N(0, 1), ranges = the distance of the two points at the graph's initial estimate
    + sigma * N(0, 1) (absolute value), information info * (1 + U(0, 1)); kind / delta: one kernel for all, or None.  Draws, in this order,
    from default_rng(seed): arm_i [n, 3], arm_j [n, 3], the noise [n], the informations [n]."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = len(pairs)
    ai, aj = arm * rng.normal(size=(n, 3)), arm * rng.normal(size=(n, 3))
    d = np.array([np.linalg.norm(rr.antenna(fp, i, ai[k]) - rr.antenna(fp, j, aj[k])) for k, (i, j) in enumerate(pairs)]).reshape(n)
    rng_m = np.abs(d + sigma * rng.normal(size=n))
    Om = info * (1.0 + rng.uniform(size=n))
    pi, pj = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    if kind is None:
        return pi, pj, rng_m, Om, ai, aj, None, None
    return pi, pj, rng_m, Om, ai, aj, np.full(n, kind, dtype=np.int32), np.full(n, float(delta))

"""numpy fp64 model of the SE(3) relative-pose edges (cuba_hip_set_relative_pose_edges) -- TEST INFRASTRUCTURE.

An edge between poses i and j (world -> camera, quaternion (x, y, z, w)) with the measurement Zbar of T_j T_i^-1 and information Omega
(6 x 6, [omega, upsilon] order) has the residual r = log(T_j T_i^-1 Zbar^-1) and the objective term r^T Omega r.  Under the solver's update
T <- exp(d) T:  dr/dd_j = J_l(r)^-1,  dr/dd_i = -J_l(r)^-1 Ad(M),  M = T_j T_i^-1.  dense_lm() is prior_reference's Levenberg-Marquardt
loop (same rules) on the dense normal equations of the oracle plus the prior terms plus the relative-pose terms."""
import numpy as np

from oracle import oracle
import prior_reference as pr
from prior_reference import hat, quat_mul, quat_conj, se3_log, se3_jl_inv


def pose_mul(a, b):
    """(qa, ta) o (qb, tb): x -> Ra (Rb x + tb) + ta"""
    qa, ta = a
    qb, tb = b
    return quat_mul(qa, qb), oracle.quat_to_rot(np.asarray(qa, dtype=np.float64)) @ np.asarray(tb, dtype=np.float64) + np.asarray(ta, dtype=np.float64)


def pose_inv(a):
    q, t = a
    qc = quat_conj(np.asarray(q, dtype=np.float64))
    return qc, -(oracle.quat_to_rot(qc) @ np.asarray(t, dtype=np.float64))


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def relative_pose(qi, ti, qj, tj):
    """M = T_j T_i^-1 as (q, t)"""
    q, t = pose_mul((unit(qj), tj), pose_inv((unit(qi), ti)))
    return unit(q), t


def rel_residual(qi, ti, qj, tj, qz, tz):
    """r = log(T_j T_i^-1 Zbar^-1)"""
    q, t = pose_mul(relative_pose(qi, ti, qj, tj), pose_inv((unit(qz), tz)))
    return se3_log(unit(q), t)


def adjoint(q, t):
    """Ad of the pose (q, t) in [omega, upsilon] order: [[R, 0], [[t]x R, R]]"""
    R = oracle.quat_to_rot(unit(q))
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def rel_jacobians(qi, ti, qj, tj, qz, tz, ad_identity=False):
    """(r, dr/dd_i, dr/dd_j); ad_identity = the deliberately wrong dr/dd_i = -J_l(r)^-1 of the gradient test"""
    r = rel_residual(qi, ti, qj, tj, qz, tz)
    Jinv = se3_jl_inv(r)
    Ad = np.eye(6) if ad_identity else adjoint(*relative_pose(qi, ti, qj, tj))
    return r, -Jinv @ Ad, Jinv


def rel_terms(rel, q, t, Pf, ad_identity=False):
    """per edge (chi2, i, j, Ji, Jj, Omega, r) at the estimate (q[Pt, 4], t[Pt, 3]); rel = (pose_i[n], pose_j[n], qz[n, 4], tz[n, 3],
    info[n, 6, 6]) as HipSolver.set_relative_pose_edges takes them.  Ji / Jj is None for a fixed end; both fixed: chi2 0."""
    pi, pj, qz, tz, info = rel
    out = []
    for k in range(len(pi)):
        i, j = int(pi[k]), int(pj[k])
        if i >= Pf and j >= Pf:
            out.append((0.0, i, j, None, None, None, None))
            continue
        r, Ji, Jj = rel_jacobians(q[i], t[i], q[j], t[j], qz[k], tz[k], ad_identity)
        Om = np.asarray(info[k], dtype=np.float64).reshape(6, 6)
        Om = 0.5 * (Om + Om.T)
        out.append((float(r @ Om @ r), i, j, Ji if i < Pf else None, Jj if j < Pf else None, Om, r))
    return out


def rel_chi2(rel, q, t, Pf):
    return np.array([x[0] for x in rel_terms(rel, q, t, Pf)])


def rel_system(rel, q, t, Pf, ad_identity=False):
    """dense (6 Pf)^2 Hessian of the relative-pose edges and their part of b (= -J^T Omega r)"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for _, i, j, Ji, Jj, Om, r in rel_terms(rel, q, t, Pf, ad_identity):
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        if Ji is not None:
            H[si, si] += Ji.T @ Om @ Ji
            b[si] -= Ji.T @ Om @ r
        if Jj is not None:
            H[sj, sj] += Jj.T @ Om @ Jj
            b[sj] -= Jj.T @ Om @ r
        if Ji is not None and Jj is not None:
            X = Ji.T @ Om @ Jj
            H[si, sj] += X
            H[sj, si] += X.T
    return H, b


def objective(o, priors, rel, Pf):
    F = pr.objective(o, priors, Pf)
    if rel is not None:
        q, t, _ = o.state()
        F += float(rel_chi2(rel, q, t, Pf).sum())
    return F


def system(o, fp, priors, rel, lam, ad_identity=False):
    """(H + lam I, b) of edges, priors and relative-pose edges at the oracle's current estimate"""
    H, b = pr.system(o, fp, priors, lam)
    if rel is not None:
        q, t, _ = o.state()
        Hr, br = rel_system(rel, q, t, fp.Pf, ad_identity)
        n = 6 * fp.Pf
        H[:n, :n] += Hr
        b[:n] += br
    return H, b


def gradient(o, fp, priors, rel):
    """b at lambda = 0 with the exact Jacobians: minus half the gradient of F"""
    return system(o, fp, priors, rel, 0.0)[1]


def dense_lm(o, fp, priors, rel, niter, ad_identity=False):
    """prior_reference.dense_lm with the relative-pose terms (tau = 1e-5, <= 10 trials, g2o's rho / lambda rules, scale += 1e-3)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams = 2.0, 0.0, [], []
    F = objective(o, priors, rel, fp.Pf)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, priors, rel, 0.0, ad_identity)
            lam = tau * float(np.max(np.diag(H0)))
        qn, rho = 0, -1.0
        while qn < maxq and rho < 0:
            H, b = system(o, fp, priors, rel, lam, ad_identity)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, priors, rel, fp.Pf)
            scale = float(x @ (lam * x + b)) + 1e-3
            rho = (F - Fhat) / scale if ok else -1.0
            qn += 1
            if rho > 0:
                lam *= max(1.0 / 3, min(1 - (2 * rho - 1) ** 3, 2.0 / 3))
                nu = 2.0
                F = Fhat
                break
            lam *= nu
            nu *= 2
            o.set_state(*saved)
        chi2.append(F)
        lams.append(lam)
        if qn == maxq or rho <= 0 or not np.isfinite(lam):
            break
    return dict(chi2=np.array(chi2), lambdas=np.array(lams))


def measurement(q, t, i, j):
    """the exact relative pose T_j T_i^-1 of an estimate, as (qz, tz)"""
    return relative_pose(q[i], t[i], q[j], t[j])

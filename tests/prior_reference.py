"""numpy fp64 model of the SE(3) pose priors (cuba_hip_set_pose_priors) -- TEST INFRASTRUCTURE.

A prior on pose T = [R | t] (world -> camera, quaternion (x, y, z, w)) with prior pose Tbar and information Omega (6 x 6, [omega, upsilon]
order) has the residual r = log(T Tbar^-1) = [w ; V(w)^-1 (t - R Rbar^T tbar)], w = log(R Rbar^T), and the objective term r^T Omega r.
Under the solver's update T <- exp(d) T the residual moves as log(exp(d) exp(r)), so dr/dd = J_l(r)^-1, the inverse left Jacobian of
SE(3).  dense_lm() is the library's Levenberg-Marquardt loop (tau = 1e-5, <= 10 trials, g2o's rho / lambda rules, scale += 1e-3) on the
dense normal equations of the oracle plus the prior terms."""
import numpy as np

from oracle import oracle
from test_gpu_configs import dense_normal_equations


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def quat_mul(a, b):
    """Hamilton product of (x, y, z, w) quaternions."""
    av, aw, bv, bw = np.asarray(a[:3]), a[3], np.asarray(b[:3]), b[3]
    v = aw * bv + bw * av + np.cross(av, bv)
    return np.array([v[0], v[1], v[2], aw * bw - av @ bv])


def quat_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def so3_log_quat(q):
    """rotation vector of a unit quaternion (any sign), well defined up to theta = pi"""
    q = np.asarray(q, dtype=np.float64)
    if q[3] < 0:
        q = -q
    n = np.linalg.norm(q[:3])
    if n < 1e-4:
        s = 2.0 / q[3] * (1.0 - (n / q[3]) ** 2 / 3.0)
    else:
        s = 2.0 * np.arctan2(n, q[3]) / n
    return s * q[:3]


def so3_jl(w):
    """left Jacobian of SO(3) (= V of the se3 exponential)"""
    th = np.linalg.norm(w)
    W = hat(w)
    if th < 1e-4:
        a2, a3 = 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        a2, a3 = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + a2 * W + a3 * W @ W


def so3_jl_inv(w):
    th = np.linalg.norm(w)
    W = hat(w)
    if th < 0.25:
        d = 1.0 / 12 + th * th / 720 + th ** 4 / 30240 + th ** 6 / 1209600
    else:
        d = (1 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / th ** 2
    return np.eye(3) - 0.5 * W + d * W @ W


def se3_q(w, u):
    """the lower-left block Q(w, u) of the SE(3) left Jacobian in [omega, upsilon] order (Barfoot's Q(rho = u, phi = w))"""
    th = np.linalg.norm(w)
    W, P = hat(w), hat(u)
    if th < 0.25:
        t2 = th * th
        c1 = 1.0 / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880
        c2 = 1.0 / 24 - t2 / 720 + t2 * t2 / 40320 - t2 ** 3 / 3628800
        c3 = 1.0 / 120 - t2 / 2520 + t2 * t2 / 120960 - t2 ** 3 / 9979200
    else:
        s, c = np.sin(th), np.cos(th)
        c1 = (th - s) / th ** 3
        c2 = (th * th / 2 + c - 1) / th ** 4
        c3 = 0.5 * (c2 + 3 * (th - s - th ** 3 / 6) / th ** 5)
    WP, PW, WPW = W @ P, P @ W, W @ P @ W
    return 0.5 * P + c1 * (WP + PW + WPW) + c2 * (W @ WP + PW @ W - 3 * WPW) + c3 * (WPW @ W + W @ WPW)


def se3_jl(r):
    w, u = r[:3], r[3:]
    J = np.zeros((6, 6))
    Jw = so3_jl(w)
    J[:3, :3] = Jw
    J[3:, 3:] = Jw
    J[3:, :3] = se3_q(w, u)
    return J


def se3_jl_inv(r):
    """[[A, 0], [-A Q A, A]], A = J_w^-1"""
    w, u = r[:3], r[3:]
    A = so3_jl_inv(w)
    J = np.zeros((6, 6))
    J[:3, :3] = A
    J[3:, 3:] = A
    J[3:, :3] = -A @ se3_q(w, u) @ A
    return J


def se3_log(q, t):
    """[omega, upsilon] of the pose (q, t)"""
    w = so3_log_quat(q)
    return np.concatenate([w, so3_jl_inv(w) @ np.asarray(t, dtype=np.float64)])


def prior_residual(q, t, qb, tb):
    """r = log(T Tbar^-1)"""
    qb = np.asarray(qb, dtype=np.float64) / np.linalg.norm(qb)
    qr = quat_mul(np.asarray(q, dtype=np.float64), quat_conj(qb))
    qr /= np.linalg.norm(qr)
    Rr = oracle.quat_to_rot(qr)
    return se3_log(qr, np.asarray(t, dtype=np.float64) - Rr @ np.asarray(tb, dtype=np.float64))


def prior_terms(priors, q, t, Pf):
    """per prior (chi2, pose, H = J^T Omega J, g = J^T Omega r) at the estimate (q[Pt, 4], t[Pt, 3]); priors = (pose[n], qb[n, 4], tb[n, 3],
    info[n, 6, 6]) as HipSolver.set_pose_priors takes them"""
    pose, qb, tb, info = priors
    out = []
    for k in range(len(pose)):
        p = int(pose[k])
        if p >= Pf:
            out.append((0.0, p, None, None))
            continue
        r = prior_residual(q[p], t[p], qb[k], tb[k])
        Om = np.asarray(info[k], dtype=np.float64).reshape(6, 6)
        J = se3_jl_inv(r)
        out.append((float(r @ Om @ r), p, J.T @ Om @ J, J.T @ Om @ r))
    return out


def prior_chi2(priors, q, t, Pf):
    return np.array([c for c, _, _, _ in prior_terms(priors, q, t, Pf)])


def prior_system(priors, q, t, Pf):
    """dense (6 Pf)^2 prior Hessian and the prior part of b (= -J^T Omega r)"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for _, p, Hp, gp in prior_terms(priors, q, t, Pf):
        if Hp is None:
            continue
        H[6 * p:6 * p + 6, 6 * p:6 * p + 6] += Hp
        b[6 * p:6 * p + 6] -= gp
    return H, b


def ensure_structure(o):
    if not getattr(o, "_prior_structure", False):
        o.build_structure()
        o._prior_structure = True


def objective(o, priors, Pf):
    ensure_structure(o)
    q, t, _ = o.state()
    return o.compute_errors() + float(prior_chi2(priors, q, t, Pf).sum()) if priors is not None else o.compute_errors()


def system(o, fp, priors, lam):
    """(H + lam I, b) of edges and priors at the oracle's current estimate"""
    ensure_structure(o)
    o.compute_errors()             # (the oracle's build_system reads the residuals of the last evaluation)
    o.build_system()
    H, b = dense_normal_equations(o, fp, lam)
    if priors is not None:
        q, t, _ = o.state()
        Hp, bp = prior_system(priors, q, t, fp.Pf)
        n = 6 * fp.Pf
        H[:n, :n] += Hp
        b[:n] += bp
    return H, b


def gradient(o, fp, priors):
    """b at lambda = 0: minus half the gradient of F (edges robustified as the library's Gauss-Newton model, plus priors)"""
    return system(o, fp, priors, 0.0)[1]


def apply_step(o, fp, x):
    q, t, X = o.state()
    q, t, X = q.copy(), t.copy(), X.copy()
    for i in range(fp.Pf):
        q[i], t[i] = oracle.pose_update(x[6 * i:6 * i + 6], q[i], t[i])
    X[:fp.Lf] += x[6 * fp.Pf:].reshape(fp.Lf, 3)
    o.set_state(q, t, X)


def dense_lm(o, fp, priors, niter):
    """the library's LM loop on the dense system; returns dict(chi2 per iteration, lambdas)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams = 2.0, 0.0, [], []
    F = objective(o, priors, fp.Pf)
    for it in range(niter):
        H0, _ = system(o, fp, priors, 0.0)
        if it == 0:
            lam = tau * float(np.max(np.diag(H0)))
        qn, rho = 0, -1.0
        while qn < maxq and rho < 0:
            H, b = system(o, fp, priors, lam)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            apply_step(o, fp, x)
            Fhat = objective(o, priors, fp.Pf)
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

"""numpy fp64 model of the robust kernels on the pose factors (cuba_hip_set_pose_factor_robust_kernels) -- TEST INFRASTRUCTURE.

A pose prior or relative-pose edge with the kernel (kind, delta) and e = r^T Omega r (residual and Omega of prior_reference /
relative_pose_reference) has the objective term rho(e) and is linearised with w Omega in place of Omega, w = rho'(e), without a
second-order term:

    kind 0  none     rho = e                                                          w = 1
         1  Huber    rho = e (e <= delta^2), 2 delta sqrt(e) - delta^2 beyond         w = 1, delta / sqrt(e)
         2  Tukey    rho = delta^2 / 3 (1 - (1 - e / delta^2)^3), delta^2 / 3 beyond  w = (1 - e / delta^2)^2, 0
         3  Cauchy   rho = delta^2 log1p(e / delta^2)                                 w = 1 / (1 + e / delta^2)

A set's kernels are a pair (kind[n], delta[n]) in the order of the set, or None.  dense_lm() is relative_pose_reference.dense_lm (same
rules) with rho(e) in the objective and w Omega in the system."""
import numpy as np

import prior_reference as pr
import relative_pose_reference as rr

NONE, HUBER, TUKEY, CAUCHY = 0, 1, 2, 3


def rho(kind, delta, e):
    d2 = delta * delta
    if kind == HUBER:
        return e if e <= d2 else 2.0 * np.sqrt(e) * delta - d2
    if kind == TUKEY:
        return d2 / 3.0 * (1.0 - (1.0 - e / d2) ** 3) if e <= d2 else d2 / 3.0
    if kind == CAUCHY:
        return d2 * np.log1p(e / d2)
    return e


def weight(kind, delta, e):
    d2 = delta * delta
    if kind == HUBER:
        return 1.0 if e <= d2 else delta / np.sqrt(e)
    if kind == TUKEY:
        return (1.0 - e / d2) ** 2 if e <= d2 else 0.0
    if kind == CAUCHY:
        return 1.0 / (1.0 + e / d2)
    return 1.0


def _kernel(kern, k):
    return (NONE, 0.0) if kern is None else (int(kern[0][k]), float(kern[1][k]))


def rhos(kern, e):
    """rho(e[k]) under the set's kernels"""
    return np.array([rho(*_kernel(kern, k), float(e[k])) for k in range(len(e))])


def weights(kern, e):
    return np.array([weight(*_kernel(kern, k), float(e[k])) for k in range(len(e))])


def prior_system(priors, kern, q, t, Pf):
    """dense (6 Pf)^2 Hessian of the weighted priors and their part of b (= -w J^T Omega r)"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for k, (e, p, Hp, gp) in enumerate(pr.prior_terms(priors, q, t, Pf)):
        if Hp is None:
            continue
        w = weight(*_kernel(kern, k), e)
        H[6 * p:6 * p + 6, 6 * p:6 * p + 6] += w * Hp
        b[6 * p:6 * p + 6] -= w * gp
    return H, b


def rel_system(rel, kern, q, t, Pf):
    """dense (6 Pf)^2 Hessian of the weighted relative-pose edges and their part of b"""
    H, b = np.zeros((6 * Pf, 6 * Pf)), np.zeros(6 * Pf)
    for k, (e, i, j, Ji, Jj, Om, r) in enumerate(rr.rel_terms(rel, q, t, Pf)):
        if Om is None:
            continue
        Om = weight(*_kernel(kern, k), e) * Om
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


def factor_objective(priors, rel, kp, kr, q, t, Pf):
    """sum of rho(e) over the priors and the relative-pose edges at the estimate (q, t)"""
    F = 0.0
    if priors is not None:
        F += float(rhos(kp, pr.prior_chi2(priors, q, t, Pf)).sum())
    if rel is not None:
        F += float(rhos(kr, rr.rel_chi2(rel, q, t, Pf)).sum())
    return F


def objective(o, priors, rel, kp, kr, Pf):
    pr.ensure_structure(o)
    q, t, _ = o.state()
    return o.compute_errors() + factor_objective(priors, rel, kp, kr, q, t, Pf)


def system(o, fp, priors, rel, kp, kr, lam):
    """(H + lam I, b) of reprojection edges, weighted priors and weighted relative-pose edges at the oracle's current estimate"""
    H, b = pr.system(o, fp, None, lam)
    q, t, _ = o.state()
    n = 6 * fp.Pf
    if priors is not None:
        Hp, bp = prior_system(priors, kp, q, t, fp.Pf)
        H[:n, :n] += Hp
        b[:n] += bp
    if rel is not None:
        Hr, br = rel_system(rel, kr, q, t, fp.Pf)
        H[:n, :n] += Hr
        b[:n] += br
    return H, b


def dense_lm(o, fp, priors, rel, niter, kp=None, kr=None):
    """relative_pose_reference.dense_lm with the kernels kp on the priors and kr on the relative-pose edges (tau = 1e-5, <= 10 trials,
    g2o's rho / lambda rules, scale += 1e-3)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams = 2.0, 0.0, [], []
    F = objective(o, priors, rel, kp, kr, fp.Pf)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, priors, rel, kp, kr, 0.0)
            lam = tau * float(np.max(np.diag(H0)))
        qn, gain = 0, -1.0
        while qn < maxq and gain < 0:
            H, b = system(o, fp, priors, rel, kp, kr, lam)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, priors, rel, kp, kr, fp.Pf)
            scale = float(x @ (lam * x + b)) + 1e-3
            gain = (F - Fhat) / scale if ok else -1.0
            qn += 1
            if gain > 0:
                lam *= max(1.0 / 3, min(1 - (2 * gain - 1) ** 3, 2.0 / 3))
                nu = 2.0
                F = Fhat
                break
            lam *= nu
            nu *= 2
            o.set_state(*saved)
        chi2.append(F)
        lams.append(lam)
        if qn == maxq or gain <= 0 or not np.isfinite(lam):
            break
    return dict(chi2=np.array(chi2), lambdas=np.array(lams))


# ---- the false-closure scenario -----------------------------------------------------------------------------------------------------
CHI2_6DOF_95 = 12.592          # delta^2: the 95 % quantile of chi2 with 6 degrees of freedom


def noisy_edges(fp, pairs, seed, scale):
    """test_gpu_relative_pose.make_rel's edges on `pairs` with its noise (N(0, 0.03 rad), N(0, 0.1 m)) times `scale`"""
    from test_gpu_relative_pose import make_rel
    return make_rel(fp, pairs, seed=seed, rot=0.03 * scale, trans=0.1 * scale)


def join(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def false_closure_scenario(fp):
    """(odometry, closures): odometry on the consecutive free pairs (noise scale 0.1) and two false closures, (3, Pf - 5) and
    (Pf - 8, 5), that no landmark supports (noise scale 6: e of the order of 1e3 delta^2)"""
    odo = noisy_edges(fp, [(p, p + 1) for p in range(fp.Pf - 1)], seed=30, scale=0.1)
    bad = noisy_edges(fp, [(3, fp.Pf - 5), (fp.Pf - 8, 5)], seed=31, scale=6.0)
    return odo, bad


def closure_kernels(n_odo, kind, delta):
    """no kernel on the odometry, (kind, delta) on the two closures behind it"""
    return np.array([NONE] * n_odo + [kind] * 2, dtype=np.int32), np.array([0.0] * n_odo + [delta] * 2)

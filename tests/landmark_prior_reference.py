"""numpy fp64 model of the landmark position priors (cuba_hip_set_landmark_priors) -- TEST INFRASTRUCTURE.

A prior on landmark X with position Xbar, information Omega (3 x 3, symmetric) and robust kernel (kind, delta) of the pose factors'
family has the residual r = X - Xbar, e = r^T Omega r and the objective term rho(e).  Its Jacobian is the identity; it is linearised with
w = rho'(e) and no second-order term: Hll += w Omega, b_l -= w Omega r (b = minus half the gradient, the convention of the dense system).

A set is (landmark[n], xyz[n, 3], info[n, 3, 3], kind[n] or None, delta[n] or None) as HipSolver.set_landmark_priors takes it, landmarks in
the solver numbering (free ones first).  dense_lm() is the library's Levenberg-Marquardt loop as in prior_reference.dense_lm (tau = 1e-5,
<= 10 trials, g2o's rho / lambda rules, scale += 1e-3) on the dense normal equations of the oracle plus the pose factors' terms
(robust_pose_factor_reference) plus these."""
import numpy as np

import prior_reference as pr
import robust_pose_factor_reference as rf


def kernel_of(lmp, k):
    return (rf.NONE, 0.0) if lmp[3] is None else (int(lmp[3][k]), float(lmp[4][k]))


def prior_terms(lmp, X, Lf):
    """per prior (e, rho, w, landmark, Omega, r) at the landmark estimates X[Lt, 3]; a prior on a fixed landmark: (0, 0, 0, l, None, None)"""
    out = []
    for k in range(len(lmp[0])):
        l = int(lmp[0][k])
        if l >= Lf:
            out.append((0.0, 0.0, 0.0, l, None, None))
            continue
        Om = np.asarray(lmp[2][k], dtype=np.float64).reshape(3, 3)
        Om = 0.5 * (Om + Om.T)
        r = np.asarray(X[l], dtype=np.float64) - np.asarray(lmp[1][k], dtype=np.float64)
        e = float(r @ Om @ r)
        kind, delta = kernel_of(lmp, k)
        out.append((e, float(rf.rho(kind, delta, e)), float(rf.weight(kind, delta, e)), l, Om, r))
    return out


def prior_chi2(lmp, X, Lf):
    """the plain e of every prior"""
    return np.array([t[0] for t in prior_terms(lmp, X, Lf)])


def prior_objective(lmp, X, Lf):
    """sum of rho(e)"""
    return float(sum(t[1] for t in prior_terms(lmp, X, Lf)))


def landmark_blocks(lmp, X, Lf):
    """per free landmark the priors' part of Hll (w Omega, [Lf, 3, 3]) and half their gradient (w Omega r, [Lf, 3]; b_l gets minus that)"""
    H, g = np.zeros((Lf, 3, 3)), np.zeros((Lf, 3))
    for _, _, w, l, Om, r in prior_terms(lmp, X, Lf):
        if Om is None:
            continue
        H[l] += w * Om
        g[l] += w * (Om @ r)
    return H, g


def prior_system(lmp, X, Pf, Lf):
    """the priors' part of the dense (6 Pf + 3 Lf)^2 system: H and b (= -w Omega r)"""
    n = 6 * Pf + 3 * Lf
    H, b = np.zeros((n, n)), np.zeros(n)
    Hl, gl = landmark_blocks(lmp, X, Lf)
    for l in range(Lf):
        a = 6 * Pf + 3 * l
        H[a:a + 3, a:a + 3] = Hl[l]
        b[a:a + 3] = -gl[l]
    return H, b


def objective(o, fp, lmp, priors=None, rel=None, kp=None, kr=None):
    F = rf.objective(o, priors, rel, kp, kr, fp.Pf)
    if lmp is not None:
        F += prior_objective(lmp, o.state()[2], fp.Lf)
    return F


def system(o, fp, lmp, lam, priors=None, rel=None, kp=None, kr=None):
    """(H + lam I, b) of reprojection edges, pose factors and landmark priors at the oracle's current estimate"""
    H, b = rf.system(o, fp, priors, rel, kp, kr, lam)
    if lmp is not None:
        Hl, bl = prior_system(lmp, o.state()[2], fp.Pf, fp.Lf)
        H += Hl
        b += bl
    return H, b


def gradient(o, fp, lmp, **pose_factors):
    """b at lambda = 0: minus half the gradient of the Gauss-Newton model of F"""
    return system(o, fp, lmp, 0.0, **pose_factors)[1]


def dense_lm(o, fp, lmp, niter, **pose_factors):
    """the library's LM loop on the dense system; returns dict(chi2 per iteration, lambdas, rejected = trials rejected in all,
    gains = the gain ratio of every trial)"""
    maxq, tau = 10, 1e-5
    nu, lam, chi2, lams, rejected, gains = 2.0, 0.0, [], [], 0, []
    F = objective(o, fp, lmp, **pose_factors)
    for it in range(niter):
        if it == 0:
            H0, _ = system(o, fp, lmp, 0.0, **pose_factors)
            lam = tau * float(np.max(np.diag(H0)))
        qn, gain = 0, -1.0
        while qn < maxq and gain < 0:
            H, b = system(o, fp, lmp, lam, **pose_factors)
            saved = o.state()
            try:
                x = np.linalg.solve(H, b)
                ok = bool(np.all(np.isfinite(x)))
            except np.linalg.LinAlgError:
                x, ok = np.zeros_like(b), False
            pr.apply_step(o, fp, x)
            Fhat = objective(o, fp, lmp, **pose_factors)
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


def make_priors(fp, landmarks, seed=0, sigma=0.3, kind=None, delta=None):
    """priors sigma * N(0, 1) off the current estimate with information 50 I + 20 A A^T; kind / delta: one kernel for all, or None"""
    rng = np.random.default_rng(seed)
    landmarks = np.asarray(landmarks, dtype=np.int32)
    n = len(landmarks)
    X0 = np.asarray(fp.Xw, dtype=np.float64).reshape(-1, 3)
    xyz = X0[landmarks] + sigma * rng.normal(size=(n, 3))
    info = np.empty((n, 3, 3))
    for k in range(n):
        A = rng.normal(size=(3, 3))
        info[k] = 50.0 * np.eye(3) + 20.0 * (A @ A.T)
    if kind is None:
        return landmarks, xyz, info, None, None
    return landmarks, xyz, info, np.full(n, kind, dtype=np.int32), np.full(n, float(delta))

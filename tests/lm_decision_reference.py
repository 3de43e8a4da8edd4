"""The Levenberg-Marquardt decision loop of CudaBundleAdjustmentImpl::optimize (reference src/cuda_bundle_adjustment.cpp:793-857), written
out literally over SCRIPTED trial outcomes, plus the scripts the decision tests share and the exact-zero-residual scene.

reference_run() is what every copy of that loop in this project restates -- lm_decide + LmRun::absorb (the device-decided run), the host
loop of cuba_hip_solver::optimize, dist.partitioned_optimize, the oracle's optimize -- and what the tests hold each of them to.  Plain
Python floats: IEEE doubles, no contraction; the cube is t * t * t, as lm_decide and the host loop write it.  No numpy in the loop."""
import math

MAXQ = 10
NAN = float("nan")


def reference_run(F0, lam0, niter, trials, maxq=MAXQ):
    """trials: [(ok, Fhat, sumLm, sumPose), ...] in the order the run would try them (more than it uses is fine); (ok, Fhat, scale) gives the
    gain ratio's denominator as a whole.
    Returns chi2 (one per iteration), records (one dict per trial RUN: rho, lam, F, accepted after the trial, and nu, rej = the rejections
    in a row still counting, iteration), the final lam / F / nu, used = trials run, per-iteration trial counts and how the run ended:
    'niter', 'maxq', 'rho<=0', 'lambda'."""
    nu = 2.0
    lam = lam0
    F = F0
    chi2, records, counts = [], [], []
    used = 0
    ended = "niter"
    for iteration in range(niter):
        # (F = computeErrors(): the objective at the estimate the last trial left -- F after an accept, F again after a pop)
        q = 0
        rho = -1.0
        n_here = 0
        while q < maxq and rho < 0:
            if used >= len(trials):
                raise IndexError("script exhausted after %d trials" % used)
            if len(trials[used]) == 3:                               # (ok, Fhat, denominator with the 1e-3 in it: a replay of recorded trials)
                ok, Fhat, scale = trials[used]
            else:
                ok, Fhat, sumLm, sumPose = trials[used]
                scale = ((sumLm + sumPose) if ok else 0.0) + 1e-3
            used += 1
            n_here += 1
            rho = (F - Fhat) / scale if ok else -1.0
            if rho > 0:
                t = 2 * rho - 1
                a = 1 - t * t * t
                lam *= max(1. / 3, min(a, 2. / 3))
                nu = 2.0
                F = Fhat
                records.append(dict(rho=rho, lam=lam, F=F, accepted=True, nu=nu, rej=0, iteration=iteration))
                break
            lam *= nu
            nu *= 2
            # (restoreDiagonal(); pop())
            q += 1
            records.append(dict(rho=rho, lam=lam, F=F, accepted=False, nu=nu, rej=q if rho < 0 else 0, iteration=iteration))
        chi2.append(F)
        counts.append(n_here)
        if q == maxq or rho <= 0 or not math.isfinite(lam):
            ended = "maxq" if q == maxq else "rho<=0" if rho <= 0 else "lambda"
            break
    return dict(chi2=chi2, records=records, lam=lam, F=F, nu=nu, used=used, counts=counts, ended=ended)


# ---- scripts -------------------------------------------------------------------------------------------------------------------------
# Every number is an integer below 2^24 (or NaN), so that a GPU test can hand it over as partial sums that add up exactly in fp32 and fp64.
def _acc(F, gain, sumLm=600, sumPose=400):
    return (1, F - gain, sumLm, sumPose)


def _rej(F, loss=100, sumLm=50, sumPose=50):
    return (1, F + loss, sumLm, sumPose)


def _long_script():
    F, out = 1000000, []
    gains = (999, 1500, 100, 940, 2000, 50)          # (scale 1000.001: rho ~ 1, 1.5, 0.1, 0.94, 2, 0.05 -- the clamp holds the damping)
    for k in range(30):
        out += [_rej(F, 10 + k), _rej(F, 1000 + k)]
        g = gains[k % len(gains)]
        out.append(_acc(F, g)); F -= g
    return out


def _scripts():
    s = {}
    # accepted trials only: rho ~ 1 (a ~ 0 -> 1/3), 0.9 (a = 0.488, unclamped), 0.1 (a = 1.512 -> 2/3), 2 (a = -26 -> 1/3)
    s["accepted_only"] = (10000.0, 1.0, 4, [(1, 9000, 600, 400), (1, 8100, 500, 500), (1, 8000, 700, 300), (1, 7000, 300, 200)])
    # attenuation on both sides of 1/3 (rho = 0.93 | 0.94) and of 2/3 (rho = 0.84 | 0.85), and rho = 1.5 (a = -7)
    F, t = 100000, []
    for g in (840, 850, 930, 940, 1500):
        t.append(_acc(F, g)); F -= g
    s["clamp_edges"] = (100000.0, 3.0, 5, t)
    s["reject_then_accept"] = (1000.0, 0.5, 3, [_rej(1000, 200), _rej(1000), (1, 900, 50, 50), _rej(900, 50), (1, 800, 60, 40), (1, 700, 60, 40)])
    s["nine_then_accept"] = (5000.0, 0.25, 2, [_rej(5000, 10 * (k + 1)) for k in range(9)] + [_acc(5000, 500), _acc(4500, 300), _acc(4200, 100)])
    s["ten_rejections"] = (5000.0, 0.25, 3, [_rej(5000, 7 * (k + 1)) for k in range(10)] + [_acc(5000, 500), _acc(4500, 300)])
    s["six_accept_six_accept"] = (8000.0, 2.0, 3, [_rej(8000)] * 6 + [_acc(8000, 900)] + [_rej(7100, 30)] * 6 + [_acc(7100, 850), _acc(6250, 100), _acc(6150, 10)])
    s["zero_after_accept"] = (1000.0, 1.0, 5, [(1, 900, 50, 50), (1, 900, 50, 50), _acc(900, 100), _acc(800, 100)])
    s["zero_first_trial"] = (0.0, 0.125, 5, [(1, 0, 0, 0), (1, 0, 0, 0), (1, 0, 0, 0)])
    s["nan_fhat"] = (1000.0, 1.0, 4, [(1, NAN, 50, 50), _rej(1000), (1, NAN, 50, 50), (1, 900, 50, 50), (1, 850, 30, 30), (1, 800, 30, 30)])
    s["failed_mixed"] = (3000.0, 4.0, 3, [(0, 1, 2, 3), _acc(3000, 700), (0, 5000, 9, 9), (0, 10, 1, 1), _rej(2300), _acc(2300, 300), (0, 0, 0, 0), _acc(2000, 100)])
    s["all_failed"] = (3000.0, 4.0, 3, [(0, 7, 1, 1)] * 13)
    s["infinite_damping"] = (2000.0, 1e300, 2, [_rej(2000, k + 1) for k in range(10)] + [_acc(2000, 100)] * 2)
    s["niter0"] = (1000.0, 1.0, 0, [_acc(1000, 100), _rej(900)])
    s["niter1_rejections"] = (1000.0, 1.0, 1, [_rej(1000), _rej(1000, 3), _rej(1000, 1), _acc(1000, 400), _acc(600, 100)])
    s["longer_than_the_ring"] = (1000000.0, 1e-3, 30, _long_script() + [_acc(900000, 10)])
    # the damping passes FLT_MAX (3.4e38) while the double stays finite
    s["beyond_float_range"] = (4000.0, 1e38, 3, [_rej(4000), _rej(4000, 20), _rej(4000, 30), _acc(4000, 500), _rej(3500), _acc(3500, 900), _acc(2600, 100)])
    return s


SCRIPTS = _scripts()


# ---- the exact-zero-residual scene ---------------------------------------------------------------------------------------------------
def zero_residual_graph():
    """6 poses (identity rotations, dyadic translations, intrinsics 512, 512, 320, 240, bf 256; the first fixed), 24 landmarks at depths 4, 8
    and 16 with coordinates in quarters, three observations each, mono and stereo mixed, measurements from the same formula: every
    operation of the projection is exact in fp32 and fp64, so every residual is exactly 0."""
    import numpy as np
    from cuba_amd.graph import Graph
    P, L = 6, 24
    pose_t = np.array([[0.5 * k - 1.25, 0.25 * (k % 3) - 0.25, 0.0] for k in range(P)])
    pose_q = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (P, 1))
    cam = np.tile(np.array([512.0, 512.0, 320.0, 240.0, 256.0]), (P, 1))
    X = np.array([[((7 * i) % 17 - 8) / 4.0, ((5 * i) % 13 - 6) / 4.0, (4.0, 8.0, 16.0)[i % 3]] for i in range(L)])
    mono, stereo = [], []
    for i in range(L):
        for j, p in enumerate(((i) % P, (i + 1) % P, (i + 3) % P)):
            x, y, z = X[i] + pose_t[p]
            u, v = 512.0 * x / z + 320.0, 512.0 * y / z + 240.0
            if (i + j) % 2 == 0:
                stereo.append((p, P + i, (u, v, u - 256.0 / z)))
            else:
                mono.append((p, P + i, (u, v)))
    fixed = np.zeros(P, dtype=bool); fixed[0] = True
    return Graph(
        pose_ids=np.arange(P), pose_fixed=fixed, pose_q=pose_q, pose_t=pose_t, pose_cam=cam,
        lm_ids=P + np.arange(L), lm_fixed=np.zeros(L, dtype=bool), lm_X=X,
        mono_vp=np.array([m[0] for m in mono]), mono_vl=np.array([m[1] for m in mono]), mono_meas=np.array([m[2] for m in mono]),
        mono_info=np.ones(len(mono)),
        stereo_vp=np.array([m[0] for m in stereo]), stereo_vl=np.array([m[1] for m in stereo]), stereo_meas=np.array([m[2] for m in stereo]),
        stereo_info=np.ones(len(stereo)))

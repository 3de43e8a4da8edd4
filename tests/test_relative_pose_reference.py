"""CPU checks of the SE(3) relative-pose edges: the numpy model of tests/relative_pose_reference.py (which the GPU tests hold the library
to) against central differences and against the pose-prior model, the gradient bar of the GPU test on the CPU (it must tell the right
dr/dd_i from one without Ad(M)), and what builds without a GPU: the two C-ABI symbols and the loop_closure sample."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import prior_reference as pr
import relative_pose_reference as rr
from conftest import ROOT, RK_NONE
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle import oracle
from oracle.oracle import OracleSolver

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "loop_closure")
# residual rotation angles: both sides of the series threshold 0.25, up to 2.5 rad
ANGLES = (0.0, 1e-6, 1e-3, 0.2, 0.2499, 0.2501, 0.3, 1.0, 2.0, 2.5)


def _tangent(theta, rng, trans=1.0):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return np.concatenate([theta * ax, trans * rng.normal(size=3)])


def _case(theta, seed):
    """random poses i, j and a measurement such that the residual is a given tangent of rotation angle theta"""
    rng = np.random.default_rng(seed)
    qi, ti = oracle.se3_exp(_tangent(rng.uniform(0.3, 2.5), rng, 2.0))
    qj, tj = oracle.se3_exp(_tangent(rng.uniform(0.3, 2.5), rng, 2.0))
    r = _tangent(theta, rng)
    # Zbar = exp(-r) T_j T_i^-1  =>  T_j T_i^-1 Zbar^-1 = exp(r)
    qz, tz = rr.pose_mul(oracle.se3_exp(-r), rr.relative_pose(qi, ti, qj, tj))
    return qi, ti, qj, tj, qz, tz, r


@pytest.mark.parametrize("theta", ANGLES)
def test_jacobians_match_central_differences(theta):
    for seed in range(4):
        qi, ti, qj, tj, qz, tz, r = _case(theta, 100 * seed + 7)
        r0, Ji, Jj = rr.rel_jacobians(qi, ti, qj, tj, qz, tz)
        assert np.abs(r0 - r).max() <= 1e-10 * max(1.0, np.abs(r).max())
        h = 1e-6
        Ni, Nj = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            qp, tp = oracle.pose_update(d, qi, ti)
            qm, tm = oracle.pose_update(-d, qi, ti)
            Ni[:, k] = (rr.rel_residual(qp, tp, qj, tj, qz, tz) - rr.rel_residual(qm, tm, qj, tj, qz, tz)) / (2 * h)
            qp, tp = oracle.pose_update(d, qj, tj)
            qm, tm = oracle.pose_update(-d, qj, tj)
            Nj[:, k] = (rr.rel_residual(qi, ti, qp, tp, qz, tz) - rr.rel_residual(qi, ti, qm, tm, qz, tz)) / (2 * h)
        ei, ej = np.abs(Ji - Ni).max() / np.abs(Ji).max(), np.abs(Jj - Nj).max() / np.abs(Jj).max()
        print("theta %g seed %d: dr/dd_i %.2e dr/dd_j %.2e of the max-norm" % (theta, seed, ei, ej))
        assert ei <= 1e-7 and ej <= 1e-7


def test_edge_with_pose_i_fixed_is_a_prior_on_pose_j():
    rng = np.random.default_rng(3)
    Pf, Pt = 3, 5
    q = np.array([oracle.se3_exp(_tangent(rng.uniform(0.2, 2.0), rng))[0] for _ in range(Pt)])
    t = rng.normal(size=(Pt, 3))
    pi, pj = np.array([3, 4, 4]), np.array([1, 0, 2])          # (the second and third given as (fixed, free) too)
    qz, tz, info, qb, tb = [], [], [], [], []
    for k in range(3):
        m = rr.relative_pose(q[pi[k]], t[pi[k]], q[pj[k]], t[pj[k]])
        z = rr.pose_mul(oracle.se3_exp(_tangent(0.4, rng, 0.3)), m)
        qz.append(z[0]); tz.append(z[1])
        A = rng.normal(size=(6, 6))
        info.append(A @ A.T + np.eye(6))
        b = rr.pose_mul(z, (rr.unit(q[pi[k]]), t[pi[k]]))          # Tbar = Zbar T_i
        qb.append(b[0]); tb.append(b[1])
    rel = (pi, pj, np.array(qz), np.array(tz), np.array(info))
    priors = (pj, np.array(qb), np.array(tb), np.array(info))
    Hr, br = rr.rel_system(rel, q, t, Pf)
    Hp, bp = pr.prior_system(priors, q, t, Pf)
    cr, cp = rr.rel_chi2(rel, q, t, Pf), pr.prior_chi2(priors, q, t, Pf)
    assert np.abs(cr - cp).max() <= 1e-12 * cp.max()
    assert np.abs(Hr - Hp).max() <= 1e-12 * np.abs(Hp).max()
    assert np.abs(br - bp).max() <= 1e-12 * np.abs(bp).max()


def gradient_graph():
    """the graph of the gradient test (GPU test and the CPU check below): 12 poses, all but the first free, relative-pose edges between
    poses several keyframes apart (both directions), measurements a few degrees / a decimetre off the start and stiff against the
    observations, so that the optimum has non-zero residuals"""
    g = synth_ba(12, 150, 500, seed=4)
    fp = flatten(g)
    o = OracleSolver(fp, RK_NONE)
    q, t, _ = o.state()
    rng = np.random.default_rng(11)
    pi = np.array([0, 2, 5, 1, 7, 3])
    pj = np.array([6, 9, 0, 8, 2, 10])
    qz, tz = [], []
    for i, j in zip(pi, pj):
        z = rr.pose_mul(oracle.se3_exp(np.concatenate([0.05 * rng.normal(size=3), 0.1 * rng.normal(size=3)])), rr.measurement(q, t, i, j))
        qz.append(z[0]); tz.append(z[1])
    info = np.array([np.diag([4e4, 4e4, 4e4, 1e3, 1e3, 1e3])] * len(pi))
    return fp, (pi, pj, np.array(qz), np.array(tz), info)


def test_gradient_bar_tells_the_right_jacobian_from_one_without_the_adjoint():
    """40 LM iterations of the model bring the gradient below 1e-6 of its start; the same loop with Ad(M) = I in dr/dd_i does not (the
    exact gradient is evaluated in both cases)."""
    fp, rel = gradient_graph()
    o = OracleSolver(fp, RK_NONE)
    g0 = np.linalg.norm(rr.gradient(o, fp, None, rel))
    res = rr.dense_lm(o, fp, None, rel, 40)
    q, t, _ = o.state()
    assert rr.rel_chi2(rel, q, t, fp.Pf).sum() > 1e-3
    right = np.linalg.norm(rr.gradient(o, fp, None, rel)) / g0
    o2 = OracleSolver(fp, RK_NONE)
    rr.dense_lm(o2, fp, None, rel, 40, ad_identity=True)
    wrong = np.linalg.norm(rr.gradient(o2, fp, None, rel)) / g0
    print("gradient after 40 iterations / start: exact Jacobians %.3e, Ad(M) = I %.3e (%d iterations)" % (right, wrong, len(res["chi2"])))
    assert right <= 1e-6
    assert wrong > 1e-6


def test_library_exports_the_relative_pose_symbols():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    names = ("cuba_hip_set_relative_pose_edges", "cuba_hip_relative_pose_chi_squares")
    for name in names:
        assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
    capi.build_library()
    for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
        lib = ctypes.CDLL(path)
        for name in names:
            assert hasattr(lib, name), f"{name} not exported by {path}"


def test_loop_closure_sample_builds_without_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/loop_closure"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout

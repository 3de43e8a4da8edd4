"""CPU checks of the robust kernels on the pose factors: the numpy model of tests/robust_pose_factor_reference.py (which the GPU tests hold
the library to) against central differences, the false-closure scenario the kernels exist for, and what builds without a GPU: the C-ABI
symbol and the robust_loop_closure sample."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import relative_pose_reference as rr
import robust_pose_factor_reference as rb
from conftest import ROOT, RK_HUBER
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba
from oracle.oracle import OracleSolver

HOST = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host")
SAMPLE = os.path.join(HOST, "samples", "robust_loop_closure")
KINDS = (rb.NONE, rb.HUBER, rb.TUKEY, rb.CAUCHY)


@pytest.mark.parametrize("kind", KINDS)
def test_weight_is_the_derivative_of_rho(kind):
    delta = 1.7
    d2 = delta * delta
    # both sides of e = delta^2, from deep inside to far outside
    for x in (1e-3, 0.2, 0.7, 0.95, 1.05, 1.6, 5.0, 40.0):
        e = x * d2
        h = 1e-4 * e
        num = (rb.rho(kind, delta, e + h) - rb.rho(kind, delta, e - h)) / (2 * h)
        w = rb.weight(kind, delta, e)
        print("kind %d e / delta^2 %g: w %.12g, central difference %.12g" % (kind, x, w, num))
        # (step h = 1e-4 e: truncation h^2 rho''' / 6 <= 4e-9 -- Tukey's rho''' = 2 / delta^4, Huber's 3 w / (4 e^2), Cauchy's below
        # Tukey's --, rounding eps max(rho, delta^2 / 3) / h <= 4e-10: Tukey's 1 - (1 - x)^3 carries eps at x = 1e-3)
        assert abs(w - num) <= 1e-8


@pytest.mark.parametrize("kind", KINDS)
def test_rho_is_continuous_at_the_threshold(kind):
    for delta in (0.3, 1.7, 10.6):
        d2 = delta * delta
        below, at, above = (rb.rho(kind, delta, d2 * (1 + s)) for s in (-1e-13, 0.0, 1e-13))
        assert abs(below - at) <= 1e-12 * d2 and abs(above - at) <= 1e-12 * d2
        wb, wa = rb.weight(kind, delta, d2 * (1 - 1e-13)), rb.weight(kind, delta, d2 * (1 + 1e-13))
        assert abs(wb - wa) <= 1e-6          # (Tukey: (1e-13)^2 against 0; Huber: 1 against 1 - 5e-14)
    assert rb.rho(kind, 1.0, 0.0) == 0.0 and rb.weight(kind, 1.0, 0.0) == 1.0


def test_cauchy_weight_never_reaches_zero_and_tukey_does():
    assert rb.weight(rb.CAUCHY, 1.0, 1e12) > 0
    assert rb.weight(rb.TUKEY, 1.0, 1.0 + 1e-12) == 0.0
    assert rb.rho(rb.TUKEY, 3.0, 1e6) == 3.0


def test_false_closures_bend_the_trajectory_only_without_a_kernel():
    """odometry + two false closures on synth_ba(40, 600, 2400, seed=1), 10 LM iterations of the model: Tukey (delta = 3 sqrt(12.592))
    switches the closures off from the start -- F of every iteration is the clean run's plus 2 delta^2 / 3 --, Cauchy leaves less than a
    tenth of the displacement that the plain closures cause"""
    fp = flatten(synth_ba(40, 600, 2400, seed=1))
    odo, bad = rb.false_closure_scenario(fp)
    both, n = rb.join(odo, bad), len(odo[0])
    d = float(np.sqrt(rb.CHI2_6DOF_95))

    def run(rel, kr):
        o = OracleSolver(fp, RK_HUBER)
        res = rb.dense_lm(o, fp, None, rel, 10, kr=kr)
        q, t, _ = o.state()
        return res["chi2"], t.copy(), rb.weights(kr, rr.rel_chi2(rel, q, t, fp.Pf))

    f_clean, t_clean, _ = run(odo, None)
    f_none, t_none, _ = run(both, None)
    f_cauchy, t_cauchy, w_cauchy = run(both, rb.closure_kernels(n, rb.CAUCHY, d))
    f_tukey, t_tukey, w_tukey = run(both, rb.closure_kernels(n, rb.TUKEY, 3 * d))
    off_none, off_cauchy, off_tukey = (float(np.abs(t - t_clean).max()) for t in (t_none, t_cauchy, t_tukey))
    print("max |t - t_clean|: none %.4g, Cauchy %.4g, Tukey %.4g; final weights of the closures: Cauchy %s, Tukey %s; final F: clean %.4f none %.4f "
          "Cauchy %.4f Tukey %.4f" % (off_none, off_cauchy, off_tukey, w_cauchy[-2:], w_tukey[-2:], f_clean[-1], f_none[-1], f_cauchy[-1], f_tukey[-1]))
    assert len(f_tukey) == len(f_clean) == 10
    assert np.abs(f_tukey - (f_clean + 2 * (3 * d) ** 2 / 3)).max() <= 1e-9 * f_clean.min()
    assert np.array_equal(w_tukey[-2:], [0.0, 0.0])
    assert off_none > 0.05 and off_cauchy < 0.1 * off_none
    assert np.all(w_cauchy[-2:] > 0) and np.all(w_cauchy[-2:] < 0.05)


def test_library_exports_the_robust_kernel_symbol():
    from cuba_amd import capi
    header = open(os.path.join(ROOT, "include", "cuba_hip.h")).read()
    name = "cuba_hip_set_pose_factor_robust_kernels"
    assert re.search(r"^int\s+%s\s*\(" % name, header, re.M), name + " is not declared in cuba_hip.h"
    capi.build_library()
    for path in (capi.LIB_PATH, capi.LIB_PATH_F32):
        assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {path}"


def test_robust_loop_closure_sample_builds_without_gpu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cuda-bundle-adjustment_amd", "csrc"), "-s", "all"])
    subprocess.check_call(["make", "-C", HOST, "-s", "samples/robust_loop_closure"])
    assert os.access(SAMPLE, os.X_OK)
    out = subprocess.run([SAMPLE], capture_output=True, text=True)
    assert out.returncode == 0 and "usage" in out.stdout

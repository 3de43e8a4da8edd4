"""Landmark triangulation on the device (cuba_hip_triangulate_landmarks) against tests/triangulation_reference.py.

Statuses and counts are compared exactly: every such comparison first asserts ON THE REFERENCE ALONE that no tested quantity (the parallax
number, a chi2, a depth) lies within 1e-6 (relative) of its threshold, the condition of the gating tests.  The thresholds for which that
holds, checked on the CPU: chi2_max = (5.991, 7.815) and min_parallax_deg = 1 (smallest margin: 6.2e-6 on the small graph at the true
poses, 5.9e-6 from its perturbed start, 3.8e-5 on the zoo), 2 degrees on the graph with big landmarks (test_workgroup_class), and 2.08 and
1.794 degrees on the mono-only graph (test_mono_only_graph).

Positions, fp64 library: per landmark |X_dev - X_ref|_inf <= 8 D max(1, |X_ref|_inf), D = the reference's own largest distance from its
60-digit twin ON THE SAME LANDMARKS (tests/test_triangulation_reference.py measures the same number): the reference runs the same formulas,
so its distance to the model is a sample of the same error; 8 for the other summation order (internal pose order, the workgroup class)
and fma contraction.  fp32 library: the reference is fed the float-rounded poses, cameras, measurements, information and kernel widths the
handle holds; the same bound plus one float rounding of the stored result."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import triangulation_reference as T  # noqa: E402

from conftest import RK_HUBER, RK_TUKEY  # noqa: E402
from cuba_amd.capi import TRI_STATUS_NAMES, CubaHipError, HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402

pytestmark = pytest.mark.gpu

CHI2_MAX = (5.991, 7.815)
PARALLAX_DEG = 1.0
MARGIN = 1e-6
# tukey_wide: widths for which no landmark of the small graph is left with a matrix of rank 2 (checked on the CPU: the smallest determinant
# is 9.2e-5 of its diagonal's product over 0, 1 and 5 steps, as with Huber; with conftest's 4 / 5 px five or six landmarks have 1e-16)
KERNELS = dict(huber=RK_HUBER, tukey=RK_TUKEY, tukey_wide=((2, 300.0), (2, 400.0)))
F32_EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def true_fp():
    """small_fp's twin at the true poses and points"""
    from cuba_amd.synth import synth_ba
    return flatten(synth_ba(40, 600, 2400, seed=1, perturb=False))


@pytest.fixture(scope="module")
def big_fp():
    from test_gpu_parity import graph_with_big_landmarks
    g, n_big = graph_with_big_landmarks()
    fp = flatten(g)
    assert (np.bincount(fp.eL, minlength=fp.Lt) > 64).sum() == n_big >= 3
    return fp


@pytest.fixture(scope="module")
def zoo():
    return T.zoo_problem()


_refs = {}


def reference(key, fp, iters, rk, landmarks, state=None, select=None, omega=None, f32=False, chi2_max=CHI2_MAX, parallax=PARALLAX_DEG):
    """(reference result, D over `landmarks`), computed once per key; f32: on the float-rounded inputs"""
    if key not in _refs:
        if f32:
            fp, state = T.float_rounded(fp, state)
            rk = T.float_rounded_kernels(rk)
            omega = None if omega is None else np.asarray(omega, dtype=np.float32).astype(np.float64)
        ref = T.triangulate(fp, state=state, select=select, refine_iterations=iters, rk=rk, omega=omega, chi2_max=chi2_max,
                            min_parallax_deg=parallax)
        D, _ = T.model_distance(fp, ref, landmarks, iters, rk, state=state, omega=omega)
        _refs[key] = (ref, D)
    return _refs[key]


def check(got, ref, D, landmarks, what, f32=False, rank_deficient=0):
    """statuses and counts exactly (under the margin condition), positions of `landmarks` within the bound.
    rank_deficient: how many landmarks may have a determinant that is rounding noise (T.determinant_margin; conftest's Tukey widths only).
    Whether such a landmark is SINGULAR or what the huge step leads to depends on the noise's sign, on the device as in the reference: it
    is left out of the exact comparison, but it must be rejected on the device too (SINGULAR, BEHIND_CAMERA or CHI2) and keep its position,
    and statuses and counts over all other landmarks are compared exactly."""
    margin = T.threshold_margin(ref).min()
    sure = T.determinant_margin(ref) > MARGIN
    print(f"\n[triangulation] {what}: margin {margin:.2e}, D {D:.2e}, counts {ref['counts']}, landmarks with a determinant in the noise {(~sure).sum()}")
    assert margin > MARGIN and (~sure).sum() <= rank_deficient
    assert np.array_equal(got["status"][sure], ref["status"][sure]), np.flatnonzero(got["status"] != ref["status"])
    assert [got[k] for k in TRI_STATUS_NAMES] == list(np.bincount(got["status"], minlength=8)) and sum(ref["counts"].values()) == len(ref["status"])
    assert list(np.bincount(got["status"][sure], minlength=8)) == list(np.bincount(ref["status"][sure], minlength=8))        # (all landmarks unless rank_deficient)
    rejected = (T.SINGULAR, T.BEHIND_CAMERA, T.CHI2)
    assert all(s in rejected for s in got["status"][~sure]) and all(s in rejected for s in ref["status"][~sure])
    assert np.array_equal(got["xyz"][~sure], ref["xyz"][~sure])
    landmarks = [l for l in landmarks if sure[l]]
    ok = [l for l in landmarks if ref["status"][l] == T.OK]
    assert len(ok) >= 1
    scale = np.maximum(1.0, np.abs(ref["xyz"][ok]).max(1))
    err = np.abs(got["xyz"][ok] - ref["xyz"][ok]).max(1)
    bound = 8 * D * scale + (F32_EPS * np.abs(ref["xyz"][ok]).max(1) if f32 else 0.0)
    print(f"[triangulation] {what}: largest |X_dev - X_ref| / max(1, |X_ref|) = {(err / scale).max():.2e}, 8 D = {8 * D:.2e}")
    assert np.all(err <= bound), (float((err / scale).max()), 8 * D)
    rest = (ref["status"] != T.OK) & sure
    assert np.array_equal(got["xyz"][rest], ref["xyz"][rest])        # the unchanged current position of every other landmark


def bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


FIRST100 = range(100)


# ---- 1. statuses, counts, positions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(landmark_reorder=0, pose_reorder=0), dict(device_setup=0)], ids=["default", "caller_order", "host_setup"])
def test_true_poses_over_options(true_fp, opts):
    ref, D = reference(("true", 5, "huber"), true_fp, 5, RK_HUBER, FIRST100)
    assert ref["counts"]["ok"] == 487 and ref["counts"]["low_parallax"] == 3 and ref["counts"]["behind_camera"] == 2 and ref["counts"]["chi2"] == 108
    h = HipSolver(true_fp, RK_HUBER, **opts)
    got = h.triangulate_landmarks(chi2_max=CHI2_MAX, min_parallax_deg=PARALLAX_DEG)
    check(got, ref, D, FIRST100, f"true poses {opts}")
    assert np.array_equal(h.state()[2], got["xyz"])


@pytest.mark.parametrize("kernel", ["huber", "tukey", "tukey_wide"])
@pytest.mark.parametrize("iters", [0, 1, 5])
def test_true_poses_over_iterations_and_kernels(true_fp, iters, kernel):
    ref, D = reference(("true", iters, kernel), true_fp, iters, KERNELS[kernel], FIRST100)
    h = HipSolver(true_fp, KERNELS[kernel])
    # the Tukey kernel (widths 4 and 5 px) gives every edge but one mono edge the weight 0 on five landmarks of 600 (one step; six: five
    # steps): H of rank 2, determinants of 2e-17 ... 3e-16 of the diagonal's product where the next smallest is 9.6e-5
    check(h.triangulate_landmarks(refine_iterations=iters, chi2_max=CHI2_MAX, min_parallax_deg=PARALLAX_DEG), ref, D, FIRST100, f"true poses, {iters} iterations, {kernel}",
          rank_deficient=6 if kernel == "tukey" and iters else 0)
    if kernel == "tukey_wide" and iters:
        assert not np.array_equal(ref["xyz"], reference(("true", iters, "huber"), true_fp, iters, RK_HUBER, FIRST100)[0]["xyz"])       # (the kernel does weigh)


@pytest.mark.parametrize("deg", [2.08, 1.794])
def test_mono_only_graph(deg):
    """stereo_frac = 0: every landmark takes the parallax test, the mono rows of the linear start and the mono refinement.  The parallax
    numbers of this graph lie dense: at 0.5, 1 and 2 degrees one of them is 1.4e-7, 2.5e-7, 5.0e-7 from the threshold.  The angles here
    sit in the two widest gaps between 0.3 and 2.5 degrees, found on the CPU: margin 2.75e-6 at 2.08 degrees (369 of 600 LOW_PARALLAX,
    178 OK, 52 CHI2, 1 BEHIND_CAMERA), 1.68e-6 at 1.794 (315 LOW_PARALLAX)."""
    from cuba_amd.synth import synth_ba
    fp = flatten(synth_ba(40, 600, 2400, seed=1, stereo_frac=0.0, perturb=False))
    assert (fp.eDim == 2).all()
    lms = range(150)
    ref, D = reference(("mono", deg), fp, 5, RK_HUBER, lms, parallax=deg)
    assert ref["counts"]["low_parallax"] == (369 if deg == 2.08 else 315) and np.isfinite(ref["c"]).sum() == fp.Lt
    h = HipSolver(fp, RK_HUBER)
    check(h.triangulate_landmarks(chi2_max=CHI2_MAX, min_parallax_deg=deg), ref, D, lms, f"mono-only graph at {deg} degrees")


def test_perturbed_start_ends_mostly_as_chi2(small_fp):
    ref, D = reference(("perturbed", 5, "huber"), small_fp, 5, RK_HUBER, FIRST100)
    assert ref["counts"]["chi2"] > 500 and ref["counts"]["ok"] == 47
    h = HipSolver(small_fp, RK_HUBER)
    check(h.triangulate_landmarks(chi2_max=CHI2_MAX, min_parallax_deg=PARALLAX_DEG), ref, D, FIRST100, "perturbed start")


def test_workgroup_class(big_fp):
    """no chi2 test here (the graph's start is a perturbed one): every landmark of more than 64 edges is accepted and stored.  The parallax
    angle is 2 degrees: at 1 degree a landmark of this graph has its parallax number 4.0e-7 from the threshold, at 2 degrees the smallest
    margin is 1.1e-5 (0.75: 6.8e-6, 1.25: 3.3e-6, 1.5: 1.4e-6)"""
    fp = big_fp
    big = [int(l) for l in np.flatnonzero(np.bincount(fp.eL, minlength=fp.Lt) > 64)]
    lms = big + list(range(60))
    inf = (np.inf, np.inf)
    ref, D = reference(("big", 5, "huber"), fp, 5, RK_HUBER, lms, chi2_max=inf, parallax=2.0)
    assert (ref["status"][big] == T.OK).all()
    h = HipSolver(fp, RK_HUBER)
    check(h.triangulate_landmarks(chi2_max=inf, min_parallax_deg=2.0), ref, D, lms, "graph with big landmarks")
    sel = np.zeros(fp.Lt, bool); sel[big[0]] = True
    one = h.triangulate_landmarks(select=sel, chi2_max=inf, dry_run=True)
    assert one["ok"] == 1 and one["not_selected"] == fp.Lt - 1 and one["status"][big[0]] == T.OK


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("iters", [0, 1, 5])
def test_zoo(zoo, iters, precision):
    fp, idx, select, edge_mask = zoo
    f32 = precision == "f32"
    lms = [l for l in range(fp.Lt) if l != idx["overflow"]]
    ref, D = reference(("zoo", iters, precision), fp, iters, RK_HUBER, lms, select=select, omega=np.where(edge_mask, fp.omega, 0.0), f32=f32)
    want = dict(one_stereo=T.OK, no_disparity=T.FEW_OBSERVATIONS, parallel=T.LOW_PARALLAX, behind=T.BEHIND_CAMERA, overflow=T.SINGULAR, outlier=T.CHI2,
                fixed=T.FIXED, gated=T.FEW_OBSERVATIONS, fill0=T.NOT_SELECTED, **{f"n{n}": T.OK for n in T.ZOO_COUNTS})
    assert {k: int(ref["status"][idx[k]]) for k in want} == want and all(v > 0 for v in ref["counts"].values())
    assert [int(np.bincount(fp.eL)[idx[f"n{n}"]]) for n in T.ZOO_COUNTS] == list(T.ZOO_COUNTS)
    h = HipSolver(fp, RK_HUBER, precision=precision)
    h.set_edge_active(edge_mask)
    got = h.triangulate_landmarks(select=select, refine_iterations=iters, chi2_max=CHI2_MAX, min_parallax_deg=PARALLAX_DEG)
    check(got, ref, D, lms, f"zoo, {iters} iterations, {precision}", f32=f32)
    if iters == 5 and not f32:
        # without the parallax test the two parallel rays have a matrix of determinant exactly 0
        assert h.triangulate_landmarks(select=select, min_parallax_deg=0.0, dry_run=True)["status"][idx["parallel"]] == T.SINGULAR


def test_fp32_library_on_the_small_graph(true_fp):
    ref, D = reference(("true-f32", 5, "huber"), true_fp, 5, RK_HUBER, FIRST100, f32=True)
    h = HipSolver(true_fp, RK_HUBER, precision="f32")
    got = h.triangulate_landmarks(chi2_max=CHI2_MAX, min_parallax_deg=PARALLAX_DEG)
    check(got, ref, D, FIRST100, "true poses, fp32 library", f32=True)
    assert np.array_equal(h.state()[2], got["xyz"])


# ---- 2. what a call touches ---------------------------------------------------------------------------------------------------------
def test_only_accepted_selected_landmarks_change(small_fp, true_fp):
    fp = true_fp
    h = HipSolver(fp, RK_HUBER)
    h.set_state(fp.q, fp.t, small_fp.Xw)                      # (a start that is not the answer)
    select = np.arange(fp.Lt) % 2 == 0
    q0, t0, X0 = h.state()
    got = h.triangulate_landmarks(select=select)
    q1, t1, X1 = h.state()
    ok = got["status"] == T.OK
    assert bits_equal(q0, q1) and bits_equal(t0, t1)
    assert (got["status"][~select] == T.NOT_SELECTED).all() and ok.sum() > 200 and (~ok & select).sum() > 20
    assert bits_equal(X1[~ok], X0[~ok]) and bits_equal(X1[ok], got["xyz"][ok]) and bits_equal(got["xyz"][~ok], X0[~ok])
    assert not np.array_equal(X1[ok], X0[ok])


def test_the_start_is_never_read(true_fp):
    fp = true_fp
    select = np.arange(fp.Lt) % 3 != 0
    a = HipSolver(fp, RK_HUBER)
    ra = a.triangulate_landmarks(select=select)
    X = fp.Xw.copy(); X[select] = np.nan
    b = HipSolver(fp, RK_HUBER)
    b.set_state(fp.q, fp.t, X)
    rb = b.triangulate_landmarks(select=select)
    ok = ra["status"] == T.OK
    assert np.array_equal(ra["status"], rb["status"]) and bits_equal(ra["xyz"][ok], rb["xyz"][ok]) and bits_equal(a.state()[2][ok], b.state()[2][ok])
    assert np.isnan(b.state()[2][select & ~ok]).all() and (select & ~ok).sum() > 20         # a rejected landmark keeps its start, NaN or not


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_dry_run_changes_nothing(small_fp, precision):
    h = HipSolver(small_fp, RK_HUBER, precision=precision)
    before = h.state()
    dry = h.triangulate_landmarks(dry_run=True)
    assert all(bits_equal(a, b) for a, b in zip(h.state(), before))
    real = h.triangulate_landmarks()
    assert np.array_equal(dry["status"], real["status"]) and bits_equal(dry["xyz"], real["xyz"]) and dry["ok"] == real["ok"] > 0
    assert bits_equal(h.state()[2], real["xyz"]) and not bits_equal(h.state()[2], before[2])


def test_gated_edges_are_out(true_fp):
    import edge_gate_reference as G
    fp = true_fp
    mask = G.mask_keeping_two_per_landmark(fp, np.random.default_rng(7), fraction=0.3)
    mask[fp.eL == 5] = False                                    # and a landmark left without any
    ref, D = reference(("true-gated", 5, "huber"), fp, 5, RK_HUBER, FIRST100, omega=np.where(mask, fp.omega, 0.0))
    assert ref["status"][5] == T.FEW_OBSERVATIONS and not np.array_equal(ref["status"], reference(("true", 5, "huber"), fp, 5, RK_HUBER, FIRST100)[0]["status"])
    h = HipSolver(fp, RK_HUBER)
    h.set_edge_active(mask)
    check(h.triangulate_landmarks(chi2_max=CHI2_MAX, min_parallax_deg=PARALLAX_DEG), ref, D, FIRST100, "gated")
    assert np.array_equal(h.edge_active(), mask)


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_optimize_after_triangulation_equals_a_handle_set_to_that_state(small_fp, precision):
    fp = small_fp
    h = HipSolver(fp, RK_HUBER, precision=precision)
    got = h.triangulate_landmarks(chi2_max=(np.inf, np.inf))
    assert got["ok"] > 500
    twin = HipSolver(fp, RK_HUBER, precision=precision)
    twin.set_state(*h.state())
    assert all(bits_equal(a, b) for a, b in zip(h.state(), twin.state()))
    a, b = h.optimize(5)["chi2"], twin.optimize(5)["chi2"]
    assert len(a) == len(b) > 0 and bits_equal(a, b) and all(bits_equal(x, y) for x, y in zip(h.state(), twin.state()))


# ---- 3. errors --------------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(CubaHipError) as e:
        call()
    return int(re.match(r"status (\d+)", str(e.value)).group(1))


def test_errors_and_the_handle_afterwards(small_fp):
    fp = small_fp
    STATE, ARG = 3, 1
    assert status_of(HipSolver(None, RK_HUBER).triangulate_landmarks) == STATE
    for part in (lambda s: s.set_partition(0, fp.Lt // 2), lambda s: s.set_graph(fp, landmark_range=(0, fp.Lt // 2))):
        p = HipSolver(fp, RK_HUBER)
        part(p)
        assert status_of(p.triangulate_landmarks) == STATE
    h = HipSolver(fp, RK_HUBER)
    before = h.state()
    for bad in (dict(refine_iterations=-1), dict(refine_iterations=17), dict(min_parallax_deg=np.nan), dict(chi2_max=(np.nan, 7.815)), dict(chi2_max=(5.991, np.nan))):
        assert status_of(lambda: h.triangulate_landmarks(**bad)) == ARG
    assert h.lib.cuba_hip_triangulate_landmarks(h.h, None, 5, 1.0, None, 0, None, None, None) == ARG        # chi2_max NULL
    with pytest.raises(ValueError):
        h.triangulate_landmarks(select=np.ones(fp.Lt + 1, bool))
    assert all(bits_equal(a, b) for a, b in zip(h.state(), before))
    # every output is optional, 16 iterations are allowed, and the handle goes on
    assert h.lib.cuba_hip_triangulate_landmarks(h.h, None, 16, 1.0, (2 * C.c_double)(np.inf, np.inf), 0, None, None, None) == 0
    got = h.triangulate_landmarks(refine_iterations=16, chi2_max=(np.inf, np.inf), dry_run=True)
    assert bits_equal(got["xyz"], h.state()[2]) and got["ok"] > 500 and sum(got[k] for k in TRI_STATUS_NAMES) == fp.Lt
    chi2 = h.optimize(5)["chi2"]
    assert len(chi2) > 1 and chi2[-1] < chi2[0]

"""The kernels of the range factors between two poses (csrc/ba_factor.hip: pose_range_linearize_kernel, pair_gather_kernel<DevicePoseRanges>,
factor_chi2_kernel<DevicePoseRanges>) against the 60-digit reference recorded in tests/golden/pose_range_cases.npz
(tests/golden/make_golden_pose_range_cases.py), by the method of tests/test_gpu_range_factor_regimes.py: relative rotations of 1e-8
(nearly identical orientations), 1 and pi - 1e-6 and a negated quaternion x distances rho of 1e-9 ("near"), 1 ("unit") and 1e6 ("far")
of the poses' own scale, residuals |r| / rho of 0, 1e-9 (far below rho), 1e-3 and 1 (rbar = 0), arms a thousand times longer than rho,
and e / delta^2 at 0.25, 1 -+ 1e-9 and 4 under Huber and Tukey, 1 -+ 1e-9 and 4 under Cauchy.  This module reads the fixture only (no mpmath).

METHOD.  The 60-pose synthetic graph with the fixture's pose estimates, one case per pair of free poses (2 k, 2 k + 1) -- the odd cases
name them as (i, j) = (2 k + 1, 2 k), so half of the off-diagonal blocks are stored transposed --, a handle with the factors and its
factor-free twin.  The reprojection edges' information is scaled by 2^-40, which puts every plain block far below the smallest factor term
(asserted: < 1e-3): (with factors) - (plain) is then the factors' own term to rounding, and every error is taken relative to that term
alone.  Compared after build_system() + assemble() (mode 0) and after set_lambda(0) + schur() (mode 1): the two diagonal blocks (upper
triangle), bp and bsc of both ends and in mode 1 the pair's off-diagonal block; everything else must keep the plain handle's bits.  Then
the per-factor chi2 and compute_errors() against sum rho_k.  Every case is asserted without kernels (the ROBUST = false instantiations)
and with (ROBUST = true: kind none on 18 of the 29 cases), on the fp64 and on the fp32 library.

ERROR MEASURE (that of tests/test_se3_mp_reference.py).  Per case and quantity (H_ii, H_jj, H_ij = Omega J_a^T J_b, g_i, g_j =
Omega r J^T, e = Omega r^2): max |got - want| / max |want| over the entries of that quantity alone.  A case whose g and e vanish up to the
rounding of its inputs -- a prescribed zero residual, or a residual below eps L of the library's precision -- has g measured against
sqrt(max|H| Omega) L and e against Omega L^2, L = max(1, |t_i|, |t_j|, |a_i|, |a_j|) (infinity norms), under the bound of the "zero" regime
of its distance.

REGIMES AND BOUNDS.  A regime is the distance ("near", "unit", "far", or "arms" for the long lever arms at the unit distance) x the size
of the residual ("zero", "1e-09", "0.001", "1").  The condition of the direction m = u / rho is (|t_i| + |t_j| + |a_i| + |a_j|) / rho -- what
u cancels down from --, that of the residual the same over |r|, and the rotation columns m x a add |a| / |m x a| (large at the far
distance, where a_j is all but parallel to m_j): eps times that is what fp64 formulas of this kind give, and the numpy model
(pose_range_factor_reference) shows it.  The fixture holds the model's largest error per regime, measured on the CPU when it was
generated (test_the_model_errors_are_the_fixtures keeps it honest within a factor 3, and test_the_model_errors_are_eps_times_the_condition
within the condition's reach); the bound the kernels are held to is 16 x that, at least 32 eps, x 2^29 on the fp32 library:

    regime        model error   bound (fp64)   bound (fp32)      worst on the MI355X: fp64     fp32
    near/zero      4.3e-07       6.9e-06        3.7e+03           3.3e-07                       1.3
    near/0.001     4.3e-04       7.0e-03        (zero residual)   4.7e-04                       —
    unit/zero      4.7e-16       7.5e-15        4.0e-06           6.2e-16                       4.2e-07
    unit/1e-09     1.9e-07       3.0e-06        (zero residual)   4.5e-07                       —
    unit/0.001     3.6e-13       5.7e-12        3.1e-03           3.6e-13                       2.7e-04
    unit/1         4.0e-16       7.1e-15        3.8e-06           5.2e-16                       4.6e-07
    arms/0.001     3.2e-10       5.0e-09        2.7               2.1e-10                       8.0e-02
    far/0.001      1.2e-09       1.9e-08        10                1.2e-09                       3.9

(worst: over both modes and both instantiations, of the cases whose weight is at least 1e-3; every test prints its own.)  The fp64 kernels
sit at the numpy model's error -- the same formulas.

BOUNDS THAT DETECT NOTHING.  Where the rule gives a bound above 1, passing says nothing about the kernels: on the fp32 library the whole
near distance (rho = 1e-9 L is a hundredth of eps32 L: the fp32 copies of the inputs do not hold the two points apart, H, g and e could be
entirely wrong without the test noticing; its residuals count as zero residuals there: bounds 3.7e3 and 3.7e6), the far distance
(16 x 1.2e-9 x 2^29 = 10: the rotation columns' condition |a_j| / |m_j x a_j| = 1e6 is more than fp32 holds) and the long arms (2.7: the
same cross product, |a| = 1000 rho); the residual of 1e-9 rho at the unit distance counts as a zero residual on the fp32 library and is
held by that regime's bound (4.0e-6).  On the fp64 library none exceeds 1 (asserted); the near
distance's bounds (eps64 L / rho = 2e-7 L / L0 for the direction, 1e3 times that for a residual of 1e-3 rho) are the loosest.  What
holds the near and far distances and the long arms is the fp64 library; the fp32 code is held by the unit-distance cases (21 of the 29:
every rotation, every residual, every kernel; bounds 3.8e-6 ... 3.1e-3).  Every GPU test
prints "detects nothing" next to such a bound.  The library shifts nothing; a caller who ranges that close at that scale subtracts a local origin.

A weighted term w H may be off by (B w + dw) max|H|, dw the variation of rho_k' over e (1 +- 2 B) alone
(test_se3_mp_reference.kernel_window), plus 2 eps max|plain block|, the rounding of the subtraction itself; sum rho_k likewise."""
import dataclasses
import os

import numpy as np
import pytest

import pose_range_factor_reference as pp
import test_se3_mp_reference as tm
from conftest import RK_NONE

from cuba_amd.capi import HipSolver
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba

PATH = os.path.join(tm.GOLDEN, "pose_range_cases.npz")
OMEGA_SCALE = 2.0 ** -40
PRECISIONS = ("f64", "f32")
EPS_OF = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
UP = np.triu(np.ones((6, 6), dtype=bool))
ALL = np.ones((6, 6), dtype=bool)
DISTANCE_NAMES = {-9: "near", 0: "unit", 6: "far"}
QUANTITIES = ("Hii", "Hjj", "Hij", "gi", "gj")

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def fixture():
    def make():
        with np.load(PATH) as z:
            return {k: z[k] for k in z.files}
    return cached("fixture", make)


def length_scale(C):
    big = lambda x: np.abs(x).max(axis=1)  # noqa: E731
    return np.maximum(1.0, np.maximum(np.maximum(big(C["arm_i"]), big(C["arm_j"])), np.maximum(big(C["t"][C["pose_i"]]), big(C["t"][C["pose_j"]]))))


def condition(C):
    """(|t_i| + |t_j| + |a_i| + |a_j|) / rho: what u cancels down from, over what it cancels down to"""
    big = lambda x: np.abs(x).max(axis=1)  # noqa: E731
    return (big(C["t"][C["pose_i"]]) + big(C["t"][C["pose_j"]]) + big(C["arm_i"]) + big(C["arm_j"])) / C["rho"]


def below_resolution(C, precision="f64"):
    """cases whose prescribed residual is smaller than the rounding of their inputs in the library's precision (eps L)"""
    return (C["rratio"] > 0.0) & (np.abs(C["r"]) <= EPS_OF[precision] * length_scale(C))


def zero_residual(C, precision="f64"):
    """cases whose g and e vanish up to the rounding of their inputs"""
    return (C["rratio"] == 0.0) | below_resolution(C, precision)


def regime_of(C, k, precision="f64"):
    where = "arms" if C["long"][k] else DISTANCE_NAMES[int(C["distance"][k])]
    return where + "/" + ("zero" if zero_residual(C, precision)[k] else "%g" % C["rratio"][k])


def case_errors(C, got):
    """the error measure of the module docstring: got = {"Hii", "Hjj", "Hij", "gi", "gj", "e"} shaped like the fixture's outputs -> per case
    the largest error"""
    n = len(C["e"])
    zero, L = zero_residual(C), length_scale(C)
    om = C["info"]
    worst = np.zeros(n)
    for k in range(n):
        hs = max(float(np.abs(C[h][k]).max()) for h in ("Hii", "Hjj"))
        errs = [tm.relmax(got[h][k], C[h][k]) for h in ("Hii", "Hjj", "Hij")]
        errs += [tm.relmax(got[g][k], C[g][k], np.sqrt(hs * om[k]) * L[k] if zero[k] else None) for g in ("gi", "gj")]
        errs.append(tm.relmax(got["e"][k], C["e"][k], om[k] * L[k] ** 2 if zero[k] else None))
        worst[k] = max(errs)
    return worst


def model_outputs(C, variant=pp.RIGHT):
    n = len(C["e"])
    out = {"e": np.zeros(n), "Hii": np.zeros((n, 6, 6)), "Hjj": np.zeros((n, 6, 6)), "Hij": np.zeros((n, 6, 6)), "gi": np.zeros((n, 6)), "gj": np.zeros((n, 6))}
    s = (C["pose_i"], C["pose_j"], C["range"], C["info"], C["arm_i"], C["arm_j"], None, None)
    for k, (e, _, _, _, _, Ji, Jj, Om, r) in enumerate(pp.factor_terms(s, C["q"], C["t"], len(C["q"]) - 1, variant)):
        out["e"][k] = e
        out["Hii"][k], out["Hjj"][k], out["Hij"][k] = np.outer(Ji, Om * Ji), np.outer(Jj, Om * Jj), np.outer(Ji, Om * Jj)
        out["gi"][k], out["gj"][k] = (Om * Ji) * r, (Om * Jj) * r
    return out


def model_errors(C, variant=pp.RIGHT):
    """{regime: the numpy model's largest error over the regime's cases}"""
    worst = case_errors(C, model_outputs(C, variant))
    out = {}
    for k in range(len(worst)):
        out[regime_of(C, k)] = max(out.get(regime_of(C, k), 0.0), float(worst[k]))
    return out


def bound(C, reg, precision="f64"):
    """what a kernel may be off by in a regime: 16 x the model's error there, at least 32 eps; x 2^29 = eps32 / eps64 on the fp32 library"""
    return max(16.0 * float(C["model_error/" + reg]), 32.0 * tm.EPS) * (2.0 ** 29 if precision == "f32" else 1.0)


def describe(C, k):
    return "case %d (relative theta %.7g, sign %g, distance 1e%d, |r| / rho %g, long arm %d, kernel %d, ratio %g)" % (
        k, C["theta"][k], C["sign"][k], C["distance"][k], C["rratio"][k], C["long"][k], C["kind"][k], C["ratio"][k])


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_every_regime():
    C = fixture()
    n = len(C["e"])
    assert n == 29 and 2 * n <= len(C["q"]) - 1
    k = np.arange(n)
    even = k % 2 == 0
    assert np.array_equal(C["pose_i"], np.where(even, 2 * k, 2 * k + 1)) and np.array_equal(C["pose_j"], np.where(even, 2 * k + 1, 2 * k))
    for th, sign in ((1e-8, 1.0), (1.0, 1.0), (float(np.pi) - 1e-6, 1.0), (1.0, -1.0)):
        for dist in (-9, 0, 6):
            assert ((C["theta"] == th) & (C["sign"] == sign) & (C["distance"] == dist) & (C["rratio"] == 1e-3) & (C["long"] == 0) & (C["kind"] == 0)).sum() == 1
    for rratio in (0.0, 1e-9, 1.0):
        assert ((C["rratio"] == rratio) & (C["distance"] == 0)).sum() == 1
    assert ((C["rratio"] == 0.0) & (C["distance"] == -9)).sum() == 1
    assert (C["long"] == 1).sum() == 2 and set(C["theta"][C["long"] == 1]) == {1.0, float(np.pi) - 1e-6}
    # the prescribed relative angles are those of q_j q_i^-1, and one estimate in four of the rotation sweep is given as -q
    qi, qj = C["q"][C["pose_i"]], C["q"][C["pose_j"]]
    dot = np.abs((qi * qj).sum(axis=1))
    cross = np.linalg.norm(qi[:, 3:] * qj[:, :3] - qj[:, 3:] * qi[:, :3] - np.cross(qj[:, :3], qi[:, :3]), axis=1)
    assert np.abs(2 * np.arctan2(cross, dot) - C["theta"]).max() <= 1e-15 * np.pi + 1e-22
    assert (C["sign"] < 0).sum() == 3
    # rho / L0 and |r| / rho as prescribed; rbar = 0 exactly where |r| = rho
    L0 = np.maximum(1.0, np.maximum(np.abs(C["t"][C["pose_i"]]).max(axis=1), np.abs(C["t"][C["pose_j"]]).max(axis=1)))
    assert np.abs(C["rho"] / (10.0 ** C["distance"] * L0) - 1).max() <= 1e-3          # (a_j is rounded to fp64: eps L / rho <= 1e-6 * some hundreds)
    one, none = C["rratio"] == 1.0, C["rratio"] == 0.0
    assert not C["range"][one].any() and np.array_equal(C["r"][one], C["rho"][one])
    assert np.abs(C["r"][none]).max() <= tm.EPS * C["rho"][none].max() and (C["range"] >= 0).all()
    mid = ~one & ~none
    assert np.abs(C["r"][mid] / (C["rratio"][mid] * C["rho"][mid]) - 1).max() <= 1e-6      # (rbar is rounded to fp64: eps / 1e-9)
    # the cancellation is real: at the near distance the points' coordinates are 1e8 times rho; the long arms are 1000 rho long
    near = C["distance"] == -9
    assert (condition(C)[near] >= 1e8).all()
    assert (np.abs(C["arm_i"][C["long"] == 1]).max(axis=1) >= 500 * C["rho"][C["long"] == 1]).all()
    for kind in (1, 2, 3):
        for ratio in (0.25, 1 - 1e-9, 1 + 1e-9, 4.0)[1 if kind == 3 else 0:]:
            k, = np.nonzero((C["kind"] == kind) & (C["ratio"] == ratio))
            assert len(k) == 1 and abs(C["e"][k[0]] / C["delta"][k[0]] ** 2 / ratio - 1) <= 1e-15
    # every H has rank 1, H_ij included, and the g are parallel to its columns: [J_i J_j]^T Omega [J_i J_j]
    for k in range(n):
        full = np.block([[C["Hii"][k], C["Hij"][k]], [C["Hij"][k].T, C["Hjj"][k]]])
        ev = np.linalg.eigvalsh(full)
        assert ev[-1] > 0 and np.abs(ev[:-1]).max() <= 1e-13 * ev[-1]


def test_the_table_regenerates_bit_for_bit():
    """(the model errors, which a BLAS may round differently, are held within a factor 3 by the next test)"""
    pytest.importorskip("mpmath")
    import sys
    if tm.GOLDEN not in sys.path:
        sys.path.insert(0, tm.GOLDEN)
    import make_golden_pose_range_cases
    new, C = make_golden_pose_range_cases.generate(), fixture()
    assert sorted(C) == sorted(new)
    for key in C:
        if not key.startswith("model_error/"):
            assert C[key].dtype == new[key].dtype and C[key].shape == new[key].shape and C[key].tobytes() == new[key].tobytes(), key


def test_the_model_errors_are_the_fixtures():
    """the numpy model against the 60-digit values: per regime within a factor 3 of what the fixture records (and the bounds derive from)"""
    C = fixture()
    got = model_errors(C)
    assert sorted("model_error/" + r for r in got) == sorted(k for k in C if k.startswith("model_error/"))
    for reg in sorted(got):
        rec = float(C["model_error/" + reg])
        print("%-16s model error %.2e (recorded %.2e), bound fp64 %.1e, fp32 %.1e" % (reg, got[reg], rec, bound(C, reg), bound(C, reg, "f32")))
        assert got[reg] <= 3 * max(rec, tm.EPS) and rec <= 3 * max(got[reg], tm.EPS)
    # on the fp64 library every bound can detect something; every regime a case falls into on either library is recorded
    assert all(bound(C, reg) < 1 for reg in got)
    for precision in PRECISIONS:
        assert {regime_of(C, k, precision) for k in range(len(C["e"]))} <= set(got)


def test_the_model_errors_are_eps_times_the_condition():
    """the recorded errors are what the formulas' conditioning allows, not more: per case at most 64 eps x the larger of
    (|t_i| + |t_j| + |a_i| + |a_j|) / rho (the direction: what u cancels down from) and |a| / |m x a| of either end (the rotation columns:
    a far point's arm is all but parallel to the direction, |a_j| = 1e6 L0 against |m_j x a_j| of the poses' scale), over |r| / rho for a
    case with a residual (g and e carry r = rho - rbar)"""
    C = fixture()
    worst = case_errors(C, model_outputs(C))
    zero = zero_residual(C)
    for k in range(len(worst)):
        cond = condition(C)[k]
        for arm, H in ((C["arm_i"][k], C["Hii"][k]), (C["arm_j"][k], C["Hjj"][k])):
            cross = np.sqrt(np.trace(H[:3, :3]) / C["info"][k])          # |m x a| from Omega J^T J
            if np.linalg.norm(arm) > 0:
                cond = max(cond, np.linalg.norm(arm) / cross)
        cond /= 1.0 if zero[k] else min(1.0, abs(C["r"][k]) / C["rho"][k])
        assert worst[k] <= 64 * tm.EPS * max(cond, 1.0), (describe(C, k), worst[k], cond)


@pytest.mark.parametrize("variant", [pp.WORLD_DIRECTION, pp.NO_ROTATION, pp.WRONG_SIGN])
def test_the_wrong_jacobians_break_the_bounds(variant):
    """world-frame directions: off by O(1) wherever the rotations are not the identity (every case: pose i is turned by a radian); no
    rotation columns: off wherever an arm is not zero (a_j never is); m_i of the wrong sign: H_ij and g_i change sign -- beyond the regime's
    fp64 bound by > 1e3 on every case whose bound is below 1e-3"""
    C = fixture()
    worst = case_errors(C, model_outputs(C, variant))
    hit = np.array([bound(C, regime_of(C, k)) < 1e-3 for k in range(len(worst))])
    assert hit.sum() >= 20
    for k in np.nonzero(hit)[0]:
        assert worst[k] >= 1e3 * bound(C, regime_of(C, k)), describe(C, k)


def test_the_plain_system_is_negligible_on_the_cpu():
    """what the GPU test asserts of the plain handle, on the oracle: with the edges' information x 2^-40 every diagonal block of Hpp (which
    bounds the reduced blocks) is below 1e-3 of the smallest factor term -- the turned cameras still see their landmarks in front of them"""
    from oracle.oracle import OracleSolver
    C = fixture()
    fp = scene_graph()
    H = pp.system(OracleSolver(fp, RK_NONE), fp, None, 0.0)[0]
    smallest = min(float(np.abs(C[h]).max(axis=(1, 2)).min()) for h in ("Hii", "Hjj", "Hij"))
    largest = max(float(np.abs(H[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max()) for p in range(fp.Pf))
    print("largest plain diagonal block entry %.3g, smallest factor term %.3g" % (largest, smallest))
    assert largest <= 1e-3 * smallest


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------------
def scene_graph():
    def make():
        C = fixture()
        fp = flatten(synth_ba(60, 900, 3600, seed=2))
        assert fp.Pt == len(C["q"]) and fp.Pf == fp.Pt - 1
        n = 2 * len(C["e"])          # (the poses without a case keep the synthesised estimate)
        assert np.array_equal(np.asarray(fp.q).reshape(-1, 4)[n:], C["q"][n:]) and np.array_equal(np.asarray(fp.t).reshape(-1, 3)[n:], C["t"][n:])
        return dataclasses.replace(fp, q=np.ascontiguousarray(C["q"]), t=np.ascontiguousarray(C["t"]),
                                   omega=np.ascontiguousarray(np.asarray(fp.omega) * OMEGA_SCALE))
    return cached("graph", make)


def readings(with_factors, precision, robust):
    """everything the tests compare, of one handle: per mode the blocks by (row, column) in the caller's numbering, bp and bsc, then the
    per-factor chi2 and the objective.  The plain twin carries the same factors with information 0: the same block pattern, no term"""
    def make():
        C = fixture()
        h = HipSolver(scene_graph(), RK_NONE, precision=precision)
        info = C["info"] if with_factors else np.zeros_like(C["info"])
        h.set_pose_range_factors(C["pose_i"], C["pose_j"], C["range"], info, C["arm_i"], C["arm_j"], *((C["kind"], C["delta"]) if robust else (None, None)))
        out = {"F": h.compute_errors(), "chi": h.pose_range_factor_chi_squares()}
        for mode in (0, 1):
            if mode == 0:
                h.build_system()
                h.assemble()
            else:
                h.set_lambda(0.0)
                h.schur()
            rp, ci, v = h.hsc()
            out[mode] = {"blocks": {(r, int(ci[x])): v[x].copy() for r in range(len(rp) - 1) for x in range(rp[r], rp[r + 1])},
                         "bp": h.array("bp").reshape(-1, 6).copy(), "bsc": h.array("bsc").reshape(-1, 6).copy()}
        h.close()
        return out
    return cached(("readings", with_factors, precision, robust), make)


def weights(C, precision, robust):
    """per case (B, w, dw, rho_k, drho): the regime's bound, the expected weight and objective term and how far the kernel's conditioning
    lets them be off"""
    out = []
    for k in range(len(C["e"])):
        B = bound(C, regime_of(C, k, precision), precision)
        if robust:
            dw, drho = tm.kernel_window(C["kind"][k], C["delta"][k], C["e"][k], B)
            out.append((B, float(C["w"][k]), dw, float(C["rhok"][k]), B * tm.rho_scale(C["kind"][k], C["delta"][k], C["rhok"][k]) + drho))
        else:
            out.append((B, 1.0, 0.0, float(C["e"][k]), B * float(C["e"][k])))
    return out


def check(precision, robust):
    """-> {regime: worst error relative to its own term} over the cases with a weight that resolves it, and the failures of every case"""
    C = fixture()
    n = len(C["e"])
    plain, got = readings(False, precision, False), readings(True, precision, robust)
    W = weights(C, precision, robust)
    eps = EPS_OF[precision]
    zero, L = zero_residual(C, precision), length_scale(C)
    om = C["info"]
    worst, failures = {}, []
    smallest = min(float(np.abs(C[h]).max(axis=(1, 2)).min()) for h in ("Hii", "Hjj", "Hij"))
    ends = {int(C["pose_i"][k]): (k, "i") for k in range(n)}
    ends.update({int(C["pose_j"][k]): (k, "j") for k in range(n)})
    pair_of = {(min(int(C["pose_i"][k]), int(C["pose_j"][k])), max(int(C["pose_i"][k]), int(C["pose_j"][k]))): k for k in range(n)}

    def note(name, mode, k, err, may, scale):
        reg = regime_of(C, k, precision)
        if W[k][1] >= 1e-3 and not (zero[k] and name in ("bp", "bsc")):
            worst[reg] = max(worst.get(reg, 0.0), err / scale if scale > 0 else 0.0)
        if not err <= may:
            failures.append("%s mode %d of %s: %.2e of its term, %.1f x what it may be" % (name, mode, describe(C, k), err / scale, err / may))

    for mode in (0, 1):
        a, b = plain[mode], got[mode]
        assert sorted(a["blocks"]) == sorted(b["blocks"])
        for key, base in a["blocks"].items():
            have = b["blocks"][key]
            assert np.isfinite(have).all()
            assert np.abs(base).max() <= 1e-3 * smallest
            if key[0] == key[1] and key[0] in ends:
                k, end = ends[key[0]]
                want, sel, name = C["Hii" if end == "i" else "Hjj"][k], UP, "H" + end + end
                assert np.array_equal(have[~UP], base[~UP])
            elif mode == 1 and key in pair_of:
                k = pair_of[key]
                want, sel, name = C["Hij"][k] if C["pose_i"][k] < C["pose_j"][k] else C["Hij"][k].T, ALL, "Hij"
            else:
                # what the factors do not own keeps its bits
                assert np.array_equal(have, base), key
                continue
            B, w, dw, _, _ = W[k]
            hs = float(np.abs(want).max())
            err = float(np.abs((have - base)[sel] - w * want[sel]).max())
            note(name, mode, k, err, (B * w + dw) * hs + 2 * eps * float(np.abs(base).max()), w * hs)
        for name in ("bp", "bsc")[:mode + 1]:
            assert np.isfinite(b[name]).all()
            for p in range(len(a[name])):
                if p not in ends:
                    assert np.array_equal(a[name][p], b[name][p])
                    continue
                k, end = ends[p]
                B, w, dw, _, _ = W[k]
                g = C["g" + end][k]
                hs = max(float(np.abs(C[h][k]).max()) for h in ("Hii", "Hjj"))
                gs = float(np.sqrt(hs * om[k]) * L[k]) if zero[k] else float(np.abs(g).max())
                err = float(np.abs(-(b[name][p] - a[name][p]) - w * g).max())
                note(name, mode, k, err, (B * w + dw) * gs + 2 * eps * float(np.abs(a[name][p]).max()), w * gs)
    # the per-factor chi2 and the objective
    tolF = 0.0
    for k in range(n):
        B, _, _, _, drho = W[k]
        scale = om[k] * L[k] ** 2 if zero[k] else float(C["e"][k])
        err = abs(got["chi"][k] - C["e"][k]) / scale
        if not zero[k]:
            worst[regime_of(C, k, precision)] = max(worst.get(regime_of(C, k, precision), 0.0), err)
        if not err <= B:
            failures.append("chi2 of %s: %.2e, bound %.1e" % (describe(C, k), err, B))
        tolF += drho + (B * scale if zero[k] else 0.0)
    wantF = sum(x[3] for x in W)
    dF = got["F"] - plain["F"]
    assert plain["F"] <= 1e-3 * wantF and not plain["chi"].any()
    if not abs(dF - wantF) <= tolF + 4 * eps * (plain["F"] + wantF):
        failures.append("objective: %.17g against %.17g, may be off by %.2e" % (dF, wantF, tolF))
    return worst, failures


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "robust"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_pose_range_terms_against_the_reference(precision, robust):
    C = fixture()
    worst, failures = check(precision, robust)
    for reg in sorted(worst):
        B = bound(C, reg, precision)
        print("pose range %s %s: %s worst %.2e (bound %.1e%s)" % (precision, "robust" if robust else "plain", reg, worst[reg], B, ", detects nothing" if B >= 1 else ""))
    assert not failures, "\n".join(failures)

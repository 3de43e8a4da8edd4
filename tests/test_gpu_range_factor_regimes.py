"""The range-factor kernels (csrc/ba_factor.hip: range_linearize_kernel, factor_chi2_kernel<DeviceRangeFactors>) against the 60-digit
reference recorded in tests/golden/range_cases.npz (tests/golden/make_golden_range_cases.py), by the method of
tests/test_gpu_direction_factor_regimes.py: pose rotations of 1e-8, 1 and pi - 1e-6 and a negated quaternion x distances rho of 1e-6, 1
and 1e6 of the pose's own scale x residuals |r| / rho of 0, 1e-9, 1e-3 and 1 (rbar = 0), and e / delta^2 at 0, 0.25, 1 -+ 1e-9, 4 and 1e6
under every kernel.  This module reads the fixture only (no mpmath).

METHOD.  The 60-pose synthetic graph with the fixture's pose estimates, one case per free pose, a handle with the factors and its
factor-free twin.  The reprojection edges' information is scaled by 2^-40, which puts every plain diagonal block far below the smallest
factor term (asserted: < 1e-3): (with factors) - (plain) is then the factors' own term to rounding, and every error is taken relative to
that term alone.  Compared after build_system() + assemble() (mode 0) and after set_lambda(0) + schur() (mode 1): the diagonal blocks
(upper triangle), bp and bsc of the poses with a case; everything else must keep the plain handle's bits.  Then the per-factor chi2 and
compute_errors() against sum rho_k.  Every case is asserted without kernels (the ROBUST = false instantiations) and with (ROBUST = true:
kind none on 30 of the 48 cases), on the fp64 and on the fp32 library; the two instantiations must agree with each other to the same
bounds.

ERROR MEASURE (that of tests/test_se3_mp_reference.py).  Per case and quantity (H = Omega J^T J, g = Omega r J^T, e = Omega r^2):
max |got - want| / max |want| over the entries of that quantity alone.  A case whose g and e vanish up to the rounding of its inputs -- a
prescribed zero residual (|r| / rho = 0), or a residual below eps L of the library's precision (on the fp32 library: |r| / rho = 1e-9
everywhere and 1e-3 at the near distance) -- has g measured against sqrt(max|H| Omega) L and e against Omega L^2,
L = max(1, |a|, |t|, |b|) (infinity norms), under the bound of its distance's "zero" regime.

REGIMES AND BOUNDS.  A regime is the distance -- what a - t - R b cancels down to: "near" rho = 1e-6 of the pose's scale, "unit", "far"
1e6 (L is then the anchor's own size) -- x the size of the residual -- what rho - rbar cancels down to: "zero", "1e-09", "0.001", "1".  The
fixture holds the largest error of the numpy model (range_factor_reference) per regime, measured on the CPU when it was generated
(test_the_model_errors_are_the_fixtures keeps it honest within a factor 3); the bound the kernels are held to is 16 x that, at least
32 eps, x 2^29 on the fp32 library:

    regime        model error   bound (fp64)   bound (fp32)     worst on the MI355X: fp64     fp32
    near/zero      1.5e-10       2.4e-09        1.3              1.8e-10                       0.15
    near/1e-09     0.20          3.1            (zero residual)  0.28                          —
    near/0.001     2.9e-07       4.7e-06        (zero residual)  2.9e-07                       —
    near/1         1.7e-10       2.7e-09        1.4              1.8e-10                       0.18
    unit/zero      1.8e-16       7.1e-15        3.8e-06          1.8e-16                       4.8e-07
    unit/1e-09     5.6e-07       8.9e-06        (zero residual)  5.6e-07                       —
    unit/0.001     4.0e-13       6.4e-12        3.4e-03          2.5e-13                       2.5e-04
    unit/1         7.8e-16       1.2e-14        6.7e-06          1.1e-15                       2.3e-07
    far/zero       3.8e-16       7.1e-15        3.8e-06          3.6e-16                       2.3e-07
    far/1e-09      3.4e-07       5.4e-06        (zero residual)  3.4e-07                       —
    far/0.001      2.2e-13       3.5e-12        1.9e-03          2.2e-13                       1.3e-04
    far/1          2.9e-16       7.1e-15        3.8e-06          4.3e-16                       3.2e-07

(worst: over both modes and both instantiations, of the cases whose weight is at least 1e-3; every test prints its own.)  The fp64 kernels
sit at the numpy model's error -- the same formulas: eps L / rho for the direction (the near distance), eps L / |r| for the residual.
near/1e-09 is a residual of 1e-15 L, five roundings of the inputs: neither the model nor the kernels resolve it, and its bound says so.
Four bounds that the rule gives can detect nothing, and passing them says nothing about the kernels: near/1e-09 on the fp64 library
(3.1 relative) and, on the fp32 library, near/zero (1.3), near/1 (1.4) and whatever is measured under them -- there rho is 8 eps32 L, and
H, g and e could be entirely wrong without the test noticing; the measured errors, 0.15 and 0.18, are the resolution of the inputs.  What
holds the near distance is the fp64 library (1.8e-10 against 2.4e-09) and, for the fp32 code, the unit and far distances.  The library
shifts nothing; a caller who ranges that close at that scale subtracts a local origin.  The two instantiations agree bit for bit on
the fp64 library and to 7.1e-2 of the bound on the fp32 one.

A weighted term w H may be off by (B w + dw) max|H|, dw the variation of rho_k' over e (1 +- 2 B) alone
(test_se3_mp_reference.kernel_window), plus 2 eps max|plain block|, the rounding of the subtraction itself; sum rho_k likewise."""
import dataclasses
import os

import numpy as np
import pytest

import range_factor_reference as rr
import test_se3_mp_reference as tm
from conftest import RK_NONE

from cuba_amd.capi import HipSolver
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba

PATH = os.path.join(tm.GOLDEN, "range_cases.npz")
OMEGA_SCALE = 2.0 ** -40
PRECISIONS = ("f64", "f32")
EPS_OF = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
UP = np.triu(np.ones((6, 6), dtype=bool))
DISTANCE_NAMES = {-6: "near", 0: "unit", 6: "far"}

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
    n = len(C["e"])
    return np.maximum(1.0, np.maximum(np.maximum(np.abs(C["arm"]).max(axis=1), np.abs(C["t"][:n]).max(axis=1)), np.abs(C["anchor"]).max(axis=1)))


def below_resolution(C, precision="f64"):
    """cases whose prescribed residual is smaller than the rounding of their inputs in the library's precision (eps L): on the fp32
    library |r| / rho = 1e-9 at every distance and 1e-3 at the near one -- the fp32 copies of t and b do not hold such a residual, whatever
    the kernel does; none on the fp64 library"""
    return (C["rratio"] > 0.0) & (np.abs(C["r"]) <= EPS_OF[precision] * length_scale(C))


def zero_residual(C, precision="f64"):
    """cases whose g and e vanish up to the rounding of their inputs"""
    return (C["rratio"] == 0.0) | below_resolution(C, precision)


def regime_of(C, k, precision="f64"):
    return DISTANCE_NAMES[int(C["distance"][k])] + "/" + ("zero" if zero_residual(C, precision)[k] else "%g" % C["rratio"][k])


def case_errors(C, got):
    """the error measure of the module docstring: got = {"H", "g", "e"} shaped like the fixture's outputs -> per case the largest error"""
    n = len(C["e"])
    zero, L = zero_residual(C), length_scale(C)
    om = C["info"]
    worst = np.zeros(n)
    for k in range(n):
        worst[k] = max(tm.relmax(got["H"][k], C["H"][k]),
                       tm.relmax(got["g"][k], C["g"][k], np.sqrt(np.abs(C["H"][k]).max() * om[k]) * L[k] if zero[k] else None),
                       tm.relmax(got["e"][k], C["e"][k], om[k] * L[k] ** 2 if zero[k] else None))
    return worst


def model_outputs(C, variant=rr.RIGHT):
    n = len(C["e"])
    out = {"e": np.zeros(n), "H": np.zeros((n, 6, 6)), "g": np.zeros((n, 6))}
    s = (C["pose"], C["anchor"], C["range"], C["info"], C["arm"], None, None)
    for k, (e, _, _, _, J, Om, r) in enumerate(rr.factor_terms(s, C["q"], C["t"], len(C["q"]) - 1, variant)):
        out["e"][k], out["H"][k], out["g"][k] = e, np.outer(J, Om * J), (Om * J) * r
    return out


def model_errors(C, variant=rr.RIGHT):
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
    return "case %d (theta %.7g, sign %g, distance 1e%d, |r| / rho %g, kernel %d, ratio %g)" % (k, C["theta"][k], C["sign"][k], C["distance"][k],
                                                                                            C["rratio"][k], C["kind"][k], C["ratio"][k])


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_every_regime():
    C = fixture()
    n = len(C["e"])
    assert np.array_equal(C["pose"], np.arange(n)) and n <= len(C["q"]) - 1
    for th, sign in ((1e-8, 1.0), (1.0, 1.0), (float(np.pi) - 1e-6, 1.0), (1.0, -1.0)):
        for dist in (-6, 0, 6):
            for rratio in (0.0, 1e-9, 1e-3, 1.0):
                assert ((C["theta"] == th) & (C["sign"] == sign) & (C["distance"] == dist) & (C["rratio"] == rratio)).sum() == 1
    # the prescribed angles are those of the estimates, and a quarter of the estimates are given as -q
    ang = 2 * np.arctan2(np.linalg.norm(C["q"][:n, :3], axis=1), np.abs(C["q"][:n, 3]))
    assert np.abs(ang - C["theta"]).max() <= 1e-15 * np.pi + 1e-22
    assert np.array_equal(C["q"][:n, 3] < 0, C["sign"] < 0) and (C["sign"] < 0).sum() == 12
    # rho / L and |r| / rho as prescribed (L0 = max(1, |a|, |t|) of the generator); rbar = 0 exactly where |r| = rho
    L0 = np.maximum(1.0, np.maximum(np.abs(C["arm"]).max(axis=1), np.abs(C["t"][:n]).max(axis=1)))
    assert np.abs(C["rho"] / (10.0 ** C["distance"] * L0) - 1).max() <= 1e-9          # (the anchor is rounded to fp64: eps L / rho <= 1e-10 * few)
    one, none = C["rratio"] == 1.0, C["rratio"] == 0.0
    assert not C["range"][one].any() and np.array_equal(C["r"][one], C["rho"][one])
    assert np.abs(C["r"][none]).max() <= tm.EPS * C["rho"][none].max() and (C["range"] >= 0).all()
    mid = ~one & ~none
    assert np.abs(C["r"][mid] / (C["rratio"][mid] * C["rho"][mid]) - 1).max() <= 1e-6      # (rbar is rounded to fp64: eps / 1e-9)
    # the cancellation is real: near the antenna |R b| is a million times rho
    near = C["distance"] == -6
    assert (np.abs(C["anchor"][near]).max(axis=1) >= 1e5 * C["rho"][near]).all()
    # lever arms: zero on the cases 1 mod 4, half a unit vector elsewhere
    assert not C["arm"][1::4].any() and np.abs(np.linalg.norm(np.delete(C["arm"], np.s_[1::4], axis=0), axis=1) - 0.5).max() <= 1e-15
    for kind in (1, 2, 3):
        for ratio in (0.0, 0.25, 1 - 1e-9, 1 + 1e-9, 4.0, 1e6):
            k, = np.nonzero((C["kind"] == kind) & (C["ratio"] == ratio))
            assert len(k) == 1
            if ratio > 0:
                assert abs(C["e"][k[0]] / C["delta"][k[0]] ** 2 / ratio - 1) <= 1e-15
    # H = Omega J^T J has rank 1 and g = Omega r J^T is parallel to its columns
    for k in range(n):
        ev = np.linalg.eigvalsh(C["H"][k])
        assert ev[-1] > 0 and np.abs(ev[:-1]).max() <= 1e-14 * ev[-1]


def test_the_table_regenerates_bit_for_bit():
    """(the model errors, which a BLAS may round differently, are held within a factor 3 by the next test)"""
    pytest.importorskip("mpmath")
    import sys
    if tm.GOLDEN not in sys.path:
        sys.path.insert(0, tm.GOLDEN)
    import make_golden_range_cases
    new, C = make_golden_range_cases.generate(), fixture()
    assert sorted(C) == sorted(new)
    for key in C:
        if not key.startswith("model_error/"):
            assert C[key].dtype == new[key].dtype and C[key].shape == new[key].shape and C[key].tobytes() == new[key].tobytes(), key


def test_the_model_errors_are_the_fixtures():
    """the numpy model against the 60-digit values: per regime within a factor 3 of what the fixture records (and the bounds derive from)"""
    C = fixture()
    got = model_errors(C)
    assert sorted("model_error/" + r for r in got) == sorted(k for k in C if k.startswith("model_error/"))
    assert len(got) == 12
    for reg in sorted(got):
        rec = float(C["model_error/" + reg])
        print("%-16s model error %.2e (recorded %.2e), bound fp64 %.1e, fp32 %.1e" % (reg, got[reg], rec, bound(C, reg), bound(C, reg, "f32")))
        assert got[reg] <= 3 * max(rec, tm.EPS) and rec <= 3 * max(got[reg], tm.EPS)


@pytest.mark.parametrize("variant", [rr.WORLD_DIRECTION, rr.NO_ROTATION])
def test_the_wrong_jacobians_break_the_bounds(variant):
    """the world-frame direction R^T m for m: off by O(1) in H and g wherever the rotation is not the identity; no rotation columns: off
    by O(|a|^2) in H wherever the arm is not zero -- beyond the regime's fp64 bound by > 1e3 on every such case.  (Not in the regime
    near/1e-09: a residual of 1e-15 L is five roundings of the inputs, the model's own error there is 0.2 and the bound above 1, which
    nothing can break; the same rotations and arms are held by the three other residuals of the near distance)"""
    C = fixture()
    worst = case_errors(C, model_outputs(C, variant))
    hit = C["theta"] >= 1.0 if variant == rr.WORLD_DIRECTION else np.abs(C["arm"]).max(axis=1) > 0
    hit &= np.array([bound(C, regime_of(C, k)) < 1e-3 for k in range(len(hit))])
    assert hit.sum() >= 32
    for k in np.nonzero(hit)[0]:
        assert worst[k] >= 1e3 * bound(C, regime_of(C, k)), describe(C, k)


def test_the_plain_system_is_negligible_on_the_cpu():
    """what the GPU test asserts of the plain handle, on the oracle: with the edges' information x 2^-40 every diagonal block of Hpp (which
    bounds the reduced block) is below 1e-3 of the smallest factor term -- the turned cameras still see their landmarks in front of them"""
    from oracle.oracle import OracleSolver
    C = fixture()
    fp = scene_graph()
    H = rr.system(OracleSolver(fp, RK_NONE), fp, None, 0.0)[0]
    smallest = float(np.abs(C["H"]).max(axis=(1, 2)).min())
    largest = max(float(np.abs(H[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max()) for p in range(fp.Pf))
    print("largest plain diagonal block entry %.3g, smallest factor term %.3g" % (largest, smallest))
    assert largest <= 1e-3 * smallest


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------------
def scene_graph():
    def make():
        C = fixture()
        fp = flatten(synth_ba(60, 900, 3600, seed=2))
        assert fp.Pt == len(C["q"]) and fp.Pf == fp.Pt - 1
        n = len(C["e"])          # (the poses without a case keep the synthesised estimate)
        assert np.array_equal(np.asarray(fp.q).reshape(-1, 4)[n:], C["q"][n:]) and np.array_equal(np.asarray(fp.t).reshape(-1, 3)[n:], C["t"][n:])
        return dataclasses.replace(fp, q=np.ascontiguousarray(C["q"]), t=np.ascontiguousarray(C["t"]),
                                   omega=np.ascontiguousarray(np.asarray(fp.omega) * OMEGA_SCALE))
    return cached("graph", make)


def readings(with_factors, precision, robust):
    """everything the tests compare, of one handle: per mode the diagonal blocks [Pf, 6, 6], all blocks, bp and bsc, then the per-factor
    chi2 and the objective"""
    def make():
        C = fixture()
        h = HipSolver(scene_graph(), RK_NONE, precision=precision)
        if with_factors:
            h.set_range_factors(C["pose"], C["anchor"], C["range"], C["info"], C["arm"], *((C["kind"], C["delta"]) if robust else (None, None)))
        out = {"F": h.compute_errors(), "chi": h.range_factor_chi_squares() if with_factors else None}
        for mode in (0, 1):
            if mode == 0:
                h.build_system()
                h.assemble()
            else:
                h.set_lambda(0.0)
                h.schur()
            rp, ci, v = h.hsc()
            diag = rp[:-1]
            out[mode] = {"diag": v[diag].copy(), "off": np.delete(v, diag, axis=0), "bp": h.array("bp").reshape(-1, 6).copy(),
                         "bsc": h.array("bsc").reshape(-1, 6).copy()}
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
    smallest = float(np.abs(C["H"]).max(axis=(1, 2)).min())

    def note(name, mode, k, err, may, scale):
        reg = regime_of(C, k, precision)
        if W[k][1] >= 1e-3 and not (zero[k] and name != "Hpp"):
            worst[reg] = max(worst.get(reg, 0.0), err / scale if scale > 0 else 0.0)
        if not err <= may:
            failures.append("%s mode %d of %s: %.2e of its term, %.1f x what it may be" % (name, mode, describe(C, k), err / scale, err / may))

    for mode in (0, 1):
        a, b = plain[mode], got[mode]
        # what the factors do not own keeps its bits
        if mode == 1:
            assert np.array_equal(a["off"], b["off"])
        assert np.array_equal(a["diag"][n:], b["diag"][n:])
        assert np.isfinite(b["diag"][:, UP]).all()
        for name in ("bp", "bsc")[:mode + 1]:
            assert np.array_equal(a[name][n:], b[name][n:]) and np.isfinite(b[name]).all()
        for k in range(n):
            B, w, dw, _, _ = W[k]
            rel = B * w + dw
            base = a["diag"][k]
            assert np.abs(base).max() <= 1e-3 * smallest
            hs = float(np.abs(C["H"][k]).max())
            err = float(np.abs((b["diag"][k] - base)[UP] - w * C["H"][k][UP]).max())
            note("Hpp", mode, k, err, rel * hs + 2 * eps * float(np.abs(base).max()), w * hs)
            gs = float(np.sqrt(hs * om[k]) * L[k]) if zero[k] else float(np.abs(C["g"][k]).max())
            for name in ("bp", "bsc")[:mode + 1]:
                err = float(np.abs(-(b[name][k] - a[name][k]) - w * C["g"][k]).max())
                note(name, mode, k, err, rel * gs + 2 * eps * float(np.abs(a[name][k]).max()), w * gs)
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
    assert plain["F"] <= 1e-3 * wantF
    if not abs(dF - wantF) <= tolF + 4 * eps * (plain["F"] + wantF):
        failures.append("objective: %.17g against %.17g, may be off by %.2e" % (dF, wantF, tolF))
    return worst, failures


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "robust"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_range_terms_against_the_reference(precision, robust):
    C = fixture()
    worst, failures = check(precision, robust)
    for reg in sorted(worst):
        print("range %s %s: %s worst %.2e (bound %.1e)" % (precision, "robust" if robust else "plain", reg, worst[reg], bound(C, reg, precision)))
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_two_instantiations_agree_without_a_kernel(precision):
    """kind none under ROBUST = true is ROBUST = false, to the regime's bound, on every pose whose case carries no kernel"""
    C = fixture()
    a, b = readings(True, precision, False), readings(True, precision, True)
    worst = 0.0
    plain = np.nonzero(C["kind"] == 0)[0]
    assert 0 < len(plain) < len(C["e"])
    zero, L = zero_residual(C, precision), length_scale(C)
    om = C["info"]
    for k in plain:
        B = bound(C, regime_of(C, k, precision), precision)
        # (relative to the factor's own terms, as check() measures them: the plain part of a block or vector is far smaller)
        hs = float(np.abs(C["H"][k]).max())
        gs = float(np.sqrt(hs * om[k]) * L[k]) if zero[k] else float(np.abs(C["g"][k]).max())
        for mode in (0, 1):
            pairs = [(a[mode]["diag"][k][UP], b[mode]["diag"][k][UP], hs)] + [(a[mode][name][k], b[mode][name][k], gs) for name in ("bp", "bsc")[:mode + 1]]
            for x, y, scale in pairs:
                err = float(np.abs(x - y).max()) / scale
                worst = max(worst, err / B)
                assert err <= B, (describe(C, k), err)
        if not zero[k]:
            assert abs(a["chi"][k] - b["chi"][k]) <= B * b["chi"][k]
    print("range %s: the instantiations differ by at most %.2e of the bound" % (precision, worst))

"""The direction-factor kernels (csrc/ba_factor.hip: direction_linearize_kernel, factor_chi2_kernel<DeviceDirectionFactors>) against the 60-digit reference
recorded in tests/golden/direction_cases.npz (tests/golden/make_golden_direction_cases.py), by the method of
tests/test_gpu_factor_regimes.py: pose rotations of 1e-8, 1 and pi - 1e-6, a negated quaternion, residuals |r| of 1e-8, 0.1 and 2
(m = -R d), rank-2 and full information, and e / delta^2 at 0, 0.25, 1 -+ 1e-9, 4 and 1e6 under every kernel.  This module reads the
fixture only (no mpmath).

METHOD.  The 60-pose synthetic graph with the fixture's pose estimates, one case per free pose, a handle with the factors and its
factor-free twin.  The reprojection edges' information is scaled by 2^-40, which puts every plain diagonal block far below the smallest
factor term (asserted: < 1e-3): (with factors) - (plain) is then the factors' own term to rounding, and every error is taken relative to
that term alone.  Compared after build_system() + assemble() (mode 0) and after set_lambda(0) + schur() (mode 1): the rotation 3 x 3 of
the diagonal blocks (upper triangle) and bp[0..3) / bsc[0..3); everything else of the blocks, bp and bsc must keep the plain handle's
bits.  Then the per-factor chi2 and compute_errors() against sum rho.  Every case is asserted without kernels (the ROBUST = false
instantiations) and with (ROBUST = true: kind none on the regime cases), on the fp64 and on the fp32 library; the two instantiations
must agree with each other to the same bounds.

ERROR MEASURE (that of tests/test_se3_mp_reference.py).  Per case and quantity (H = J^T Omega J, g = J^T Omega r, e = r^T Omega r):
max |got - want| / max |want| over the entries of that quantity alone.  A case whose g and e vanish up to the rounding of its inputs -- a
prescribed zero residual (ratio 0), r parallel to m under the rank-2 information (|r| = 2), or a residual below eps L of the library's
precision (|r| = 1e-8 on the fp32 library: its fp32 copies of d and m do not hold it) -- has g measured against
sqrt(max|H| max|Omega|) L and e against max|Omega| L^2, L = max(1, |d|_inf, |m|_inf), under the bound of the "unit" regime.

REGIMES AND BOUNDS.  A regime is the size of the residual -- what the difference R d - m cancels down to: "tiny" 1e-8, "unit" 0.1 (and the
zero residuals), "opposite" 2 -- x the rank of the information.  The fixture holds the largest error of the numpy model
(direction_factor_reference) per regime, measured on the CPU when it was generated (test_the_model_errors_are_the_fixtures keeps it
honest within a factor 3); the bound the kernels are held to is 16 x that, at least 32 eps, x 2^29 on the fp32 library:

    regime            model error   bound (fp64)   bound (fp32)     worst on the MI355X: fp64     fp32
    tiny/full          1.1e-08       1.7e-07        (zero residual)  1.1e-08                       —
    tiny/rank2         1.4e-07       2.2e-06        (zero residual)  1.4e-07                       —
    unit/full          2.8e-15       4.5e-14        2.4e-05          3.0e-15                       1.7e-06
    unit/rank2         8.2e-14       1.3e-12        7.0e-04          7.6e-14                       1.8e-05
    opposite/full      1.2e-15       1.9e-14        1.0e-05          8.0e-16                       3.3e-07
    opposite/rank2     4.4e-16       7.1e-15        3.8e-06          4.4e-16                       1.2e-07

(worst: over both modes and both instantiations, of the cases whose weight is at least 1e-3; every test prints its own.)  The fp64 kernels
sit at the numpy model's error -- the same formulas; in the "tiny" regime both are the conditioning of the difference, eps |d| / |r|, the
rank-2 projector adding its own cancellation.  On the fp32 library |r| = 1e-8 is below eps32 L: those cases are zero residuals there.  The
two instantiations agree bit for bit on the fp64 library and to 6.1e-3 of the bound on the fp32 one.

A weighted term w H may be off by (B w + dw) max|H|, dw the variation of rho' over e (1 +- 2 B) alone
(test_se3_mp_reference.kernel_window), plus 2 eps max|plain block|, the rounding of the subtraction itself; sum rho likewise."""
import dataclasses
import os

import numpy as np
import pytest

import direction_factor_reference as dr
import test_se3_mp_reference as tm
from conftest import RK_NONE

from cuba_amd.capi import HipSolver
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba

PATH = os.path.join(tm.GOLDEN, "direction_cases.npz")
OMEGA_SCALE = 2.0 ** -40
PRECISIONS = ("f64", "f32")
EPS_OF = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
ROT = np.zeros((6, 6), dtype=bool)
ROT[:3, :3] = True
UP = np.triu(np.ones((6, 6), dtype=bool))

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
    return np.maximum(1.0, np.maximum(np.abs(C["d"]).max(axis=1), np.abs(C["m"]).max(axis=1)))


def below_resolution(C, precision="f64"):
    """cases whose prescribed residual is smaller than the rounding of their inputs in the library's precision (eps L): |r| = 1e-8 on the
    fp32 library, where eps32 L >= 1.2e-7 -- the fp32 copies of d and m do not hold such a residual, whatever the kernel does; none on the
    fp64 library (eps L <= 2.2e-15)"""
    return (C["rnorm"] > 0.0) & (C["rnorm"] <= EPS_OF[precision] * length_scale(C))


def regime_of(C, k, precision="f64"):
    rn = float(C["rnorm"][k])
    tiny = 0.0 < rn < 1e-4 and not below_resolution(C, precision)[k]          # (below the resolution: a zero residual of the "unit" regime)
    return ("tiny" if tiny else "opposite" if rn >= 1.0 else "unit") + "/" + ("rank2" if C["rank2"][k] else "full")


def zero_residual(C, precision="f64"):
    """cases whose g and e vanish up to the rounding of their inputs"""
    return (C["ratio"] == 0.0) | (C["rank2"] & (C["rnorm"] == 2.0)) | below_resolution(C, precision)


def case_errors(C, got):
    """the error measure of the module docstring: got = {"H", "g", "e"} shaped like the fixture's outputs -> per case the largest error"""
    n = len(C["e"])
    zero, L = zero_residual(C), length_scale(C)
    om = np.abs(C["info"]).reshape(n, -1).max(axis=1)
    worst = np.zeros(n)
    for k in range(n):
        worst[k] = max(tm.relmax(got["H"][k], C["H"][k]),
                       tm.relmax(got["g"][k], C["g"][k], np.sqrt(np.abs(C["H"][k]).max() * om[k]) * L[k] if zero[k] else None),
                       tm.relmax(got["e"][k], C["e"][k], om[k] * L[k] ** 2 if zero[k] else None))
    return worst


def model_outputs(C, body_frame=False):
    n = len(C["e"])
    out = {"e": np.zeros(n), "H": np.zeros((n, 6, 6)), "g": np.zeros((n, 6))}
    s = (C["pose"], C["d"], C["m"], C["info"], None, None)
    for k, (e, _, _, _, J, Om, r) in enumerate(dr.factor_terms(s, C["q"], len(C["q"]) - 1, body_frame)):
        out["e"][k], out["H"][k], out["g"][k] = e, J.T @ Om @ J, J.T @ Om @ r
    return out


def model_errors(C, body_frame=False):
    """{regime: the numpy model's largest error over the regime's cases}"""
    worst = case_errors(C, model_outputs(C, body_frame))
    out = {}
    for k in range(len(worst)):
        out[regime_of(C, k)] = max(out.get(regime_of(C, k), 0.0), float(worst[k]))
    return out


def bound(C, reg, precision="f64"):
    """what a kernel may be off by in a regime: 16 x the model's error there, at least 32 eps; x 2^29 = eps32 / eps64 on the fp32 library"""
    return max(16.0 * float(C["model_error/" + reg]), 32.0 * tm.EPS) * (2.0 ** 29 if precision == "f32" else 1.0)


def describe(C, k):
    return "case %d (theta %.7g, |r| %g, %s, kernel %d, ratio %g)" % (k, C["theta"][k], C["rnorm"][k], "rank 2" if C["rank2"][k] else "full rank",
                                                                      C["kind"][k], C["ratio"][k])


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_every_regime():
    C = fixture()
    n = len(C["e"])
    assert np.array_equal(C["pose"], np.arange(n)) and n <= len(C["q"]) - 1
    regime_cases = C["kind"] == 0
    for th in (1e-8, 1.0, float(np.pi) - 1e-6):
        for rn in (1e-8, 0.1, 2.0):
            for rank2 in (False, True):
                assert (regime_cases & (C["theta"] == th) & (C["rnorm"] == rn) & (C["rank2"] == rank2)).sum() >= 1
    # the prescribed angles are those of the estimates, and two estimates are given as -q
    ang = 2 * np.arctan2(np.linalg.norm(C["q"][:n, :3], axis=1), np.abs(C["q"][:n, 3]))
    have = C["theta"] == C["theta"]
    assert np.abs(ang[have] - C["theta"][have]).max() <= 1e-15 * np.pi + 1e-22
    assert (C["q"][:n, 3][have] < 0).sum() == 2
    # |r| as prescribed; m = -R d where |r| = 2 |d|; the rank-2 information annihilates m
    rn = np.linalg.norm(C["r"], axis=1)
    opp = C["rnorm"] == 2.0
    assert np.abs(rn[~opp] - C["rnorm"][~opp]).max() <= 1e-14          # (m is rounded to fp64: half an ulp of |d| <= 9.81)
    assert np.abs(rn[opp] - 2 * np.linalg.norm(C["d"][opp], axis=1)).max() <= 1e-13
    for k in np.nonzero(C["rank2"])[0]:
        assert np.abs(C["info"][k] @ C["m"][k]).max() <= 1e-12 * np.abs(C["info"][k]).max() * np.abs(C["m"][k]).max()
    for kind in (1, 2, 3):
        for ratio in (0.0, 0.25, 1 - 1e-9, 1 + 1e-9, 4.0, 1e6):
            k, = np.nonzero((C["kind"] == kind) & (C["ratio"] == ratio))
            assert len(k) == 1
            if ratio > 0:
                assert abs(C["e"][k[0]] / C["delta"][k[0]] ** 2 / ratio - 1) <= 1e-15
    # the translation columns are exactly zero
    assert not C["H"][:, 3:, :].any() and not C["H"][:, :, 3:].any() and not C["g"][:, 3:].any()


def test_the_table_regenerates_bit_for_bit():
    """(the model errors, which a BLAS may round differently, are held within a factor 3 by the next test)"""
    pytest.importorskip("mpmath")
    import sys
    if tm.GOLDEN not in sys.path:
        sys.path.insert(0, tm.GOLDEN)
    import make_golden_direction_cases
    new, C = make_golden_direction_cases.generate(), fixture()
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


def test_the_body_frame_jacobian_breaks_every_bound():
    """-R [d]x for -[R d]x: off by O(1) in H and g wherever the rotation is not the identity -- beyond every regime's bound by > 1e5 on the
    fp64 library"""
    C = fixture()
    worst = case_errors(C, model_outputs(C, body_frame=True))
    rotated = C["theta"] >= 1.0
    assert rotated.sum() >= 14
    for k in np.nonzero(rotated)[0]:
        assert worst[k] >= 1e5 * bound(C, regime_of(C, k)), describe(C, k)


def test_the_plain_system_is_negligible_on_the_cpu():
    """what the GPU test asserts of the plain handle, on the oracle: with the edges' information x 2^-40 every diagonal block of Hpp (which
    bounds the reduced block) is below 1e-3 of the smallest factor term -- the turned cameras still see their landmarks in front of them"""
    from conftest import RK_NONE as rk
    from oracle.oracle import OracleSolver
    C = fixture()
    fp = scene_graph()
    H = dr.system(OracleSolver(fp, rk), fp, None, 0.0)[0]
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
        kept = ~(C["theta"] == C["theta"])          # (the kernel cases and the poses without a case keep the synthesised estimate)
        kept = np.concatenate([kept, np.ones(fp.Pt - len(kept), dtype=bool)])
        assert np.array_equal(np.asarray(fp.q).reshape(-1, 4)[kept], C["q"][kept]) and np.array_equal(np.asarray(fp.t).reshape(-1, 3)[kept], C["t"][kept])
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
            h.set_direction_factors(C["pose"], C["d"], C["m"], C["info"], *((C["kind"], C["delta"]) if robust else (None, None)))
        out = {"F": h.compute_errors(), "chi": h.direction_factor_chi_squares() if with_factors else None}
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
    """per case (B, w, dw, rho, drho): the regime's bound, the expected weight and objective term and how far the kernel's conditioning
    lets them be off"""
    out = []
    for k in range(len(C["e"])):
        B = bound(C, regime_of(C, k, precision), precision)
        if robust:
            dw, drho = tm.kernel_window(C["kind"][k], C["delta"][k], C["e"][k], B)
            out.append((B, float(C["w"][k]), dw, float(C["rho"][k]), B * tm.rho_scale(C["kind"][k], C["delta"][k], C["rho"][k]) + drho))
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
    om = np.abs(C["info"]).reshape(n, -1).max(axis=1)
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
        assert np.array_equal(a["diag"][:, UP & ~ROT], b["diag"][:, UP & ~ROT])
        assert np.array_equal(a["diag"][n:], b["diag"][n:])
        for name in ("bp", "bsc")[:mode + 1]:
            assert np.array_equal(a[name][:, 3:], b[name][:, 3:]) and np.array_equal(a[name][n:], b[name][n:])
        for k in range(n):
            B, w, dw, _, _ = W[k]
            rel = B * w + dw
            base = a["diag"][k]
            assert np.abs(base).max() <= 1e-3 * smallest
            hs = float(np.abs(C["H"][k]).max())
            err = float(np.abs((b["diag"][k] - base)[UP & ROT] - w * C["H"][k][UP & ROT]).max())
            note("Hpp", mode, k, err, rel * hs + 2 * eps * float(np.abs(base).max()), w * hs)
            gs = float(np.sqrt(hs * om[k]) * L[k]) if zero[k] else float(np.abs(C["g"][k]).max())
            for name in ("bp", "bsc")[:mode + 1]:
                err = float(np.abs(-(b[name][k] - a[name][k])[:3] - w * C["g"][k][:3]).max())
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
def test_direction_terms_against_the_reference(precision, robust):
    C = fixture()
    worst, failures = check(precision, robust)
    for reg in sorted(worst):
        print("direction %s %s: %s worst %.2e (bound %.1e)" % (precision, "robust" if robust else "plain", reg, worst[reg], bound(C, reg, precision)))
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
    n = len(C["e"])
    zero, L = zero_residual(C, precision), length_scale(C)
    om = np.abs(C["info"]).reshape(n, -1).max(axis=1)
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
    print("direction %s: the instantiations differ by at most %.2e of the bound" % (precision, worst))

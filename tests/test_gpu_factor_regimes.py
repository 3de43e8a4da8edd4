"""The factor kernels (csrc/ba_factor.hip, csrc/ba_se3.hpp: pose priors, relative-pose edges, position factors, landmark priors and their
robust kernels) against the 60-digit reference recorded in tests/golden/se3_cases.npz, in every branch of the SE(3) code: the logarithm
below and above n = 1e-4, J_l^-1 by series (theta < 0.25) and by closed form up to theta = pi - 1e-6, both signs of the relative
quaternion, negated estimates, pose translations of ~10 ("near") and ~1e3 ("moved"), and e / delta^2 on every side of every kernel.  This
module reads the fixture only (no mpmath); tests/test_se3_mp_reference.py holds the error measure, the regimes and the bounds, and shows
on the CPU that five subtly wrong formulas break these bounds by more than 2e10.

METHOD.  The 60-pose synthetic graph with one case per free pose (or disjoint pose pair), one handle per factor kind and scene plus its
factor-free twin.  The reprojection edges' information is scaled by 2^-40, which puts every plain diagonal block below 1e-6 of the
smallest factor term (asserted: < 1e-3): (with factors) - (plain) is then the factors' own term to rounding, and every error is taken
relative to that term alone.  Compared after build_system() + assemble() (mode 0) and after set_lambda(0) + schur() (mode 1): the diagonal
blocks (upper triangle), the off-diagonal blocks of the pairs (mode 1), bp, bsc (mode 1), the landmark systems, the per-factor chi2 and
compute_errors() against sum rho.  Every case is asserted in every parametrisation: without kernels (the ROBUST = false instantiations),
with kernels (ROBUST = true: kind none on the regime cases, Huber / Tukey / Cauchy at e / delta^2 = 0, 0.25, 1 -+ 1e-9, 4, 1e6 on the
others), on the fp64 and on the fp32 library; the two instantiations must agree with each other to the same bounds.

TOLERANCE.  Per regime B = 16 x the error of the numpy model in that regime, at least 32 eps, x 2^29 on the fp32 library
(test_se3_mp_reference.MODEL_ERROR, measured on the CPU and committed):

    regime            model error   bound (fp64)   bound (fp32)     worst on the MI355X: fp64     fp32
    series / near       9.6e-14       1.5e-12        8.2e-04                           9.6e-14     2.7e-06
    closed / near       9.7e-15       1.6e-13        8.3e-05                           3.5e-14     8.6e-06
    series / moved      9.5e-13       1.5e-11        8.2e-03                           5.5e-13     2.3e-04
    closed / moved      6.5e-13       1.0e-11        5.6e-03                           1.2e-12     7.2e-04
    vector / near       1.3e-14       2.1e-13        1.1e-04                           1.3e-14     1.1e-05
    vector / moved      3.8e-12       6.1e-11        3.3e-02                           3.8e-12     1.0e-03

(worst: over all kinds, modes and both instantiations, of the cases whose weight is at least 1e-3; every test prints its own.)  The
fp64 kernels sit within a factor 4 of the numpy model -- the same formulas; the relative edges compose their poses in another order
(3.5e-14 against 9.7e-15 in closed / near) --, the series row at the truncation of the four-term series just below theta = 0.25 (6.9e-14
for a prior at 0.2499 against 1.3e-15 at 0.2501); the fp32 library is 8 ... 300 x inside its bounds.

A weighted term w H may be off by (B w + dw) max|H|, dw the variation of rho' over e (1 +- 2 B) alone (kernel_window: the conditioning of
the kernel, unbounded at Tukey's double zero; 0 for kind none, which is held to B under either instantiation), plus 2 eps max|plain
block|, the rounding of the subtraction itself; sum rho likewise, B rho + the variation of rho per case."""
import dataclasses

import numpy as np
import pytest

import test_se3_mp_reference as tm
from conftest import RK_NONE
from test_gpu_relative_pose import block_index

from cuba_amd.capi import HipSolver
from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba

pytestmark = pytest.mark.gpu

OMEGA_SCALE = 2.0 ** -40
SHIFT = np.array([800.0, -500.0, 300.0])
PRECISIONS = ("f64", "f32")
EPS_OF = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}
UP = np.triu_indices(6)

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def scene_graph(scene):
    """the 60-pose graph with the fixture's estimates (the synthesised ones, a few quaternions negated; "moved": shifted rigidly) and the
    reprojection edges' information scaled down"""
    def make():
        S = tm.fixture()[scene]
        fp = flatten(synth_ba(60, 900, 3600, seed=2))
        assert fp.Pf == tm.free_poses(S) and fp.Pt == fp.Pf + 1
        if scene == "near":          # the fixture was recorded on this graph
            assert np.array_equal(np.abs(fp.q), np.abs(S["q"])) and np.array_equal(fp.t, S["t"])
        Xw = np.asarray(fp.Xw, dtype=np.float64) + (SHIFT if scene == "moved" else 0.0)
        L = S["landmark"]
        assert np.array_equal(Xw[L["lm"]], L["X"])
        return dataclasses.replace(fp, q=np.ascontiguousarray(S["q"]), t=np.ascontiguousarray(S["t"]), Xw=np.ascontiguousarray(Xw),
                                   omega=np.ascontiguousarray(np.asarray(fp.omega) * OMEGA_SCALE))
    return cached(("graph", scene), make)


def attach(h, kind, C, robust):
    kern = (C["kind"], C["delta"]) if robust else (None, None)
    if kind == "prior":
        h.set_pose_priors(C["pose"], C["qb"], C["tb"], C["info"])
        if robust:
            h.set_pose_factor_robust_kernels(0, *kern)
    elif kind == "relative":
        h.set_relative_pose_edges(C["i"], C["j"], C["qz"], C["tz"], C["info"])
        if robust:
            h.set_pose_factor_robust_kernels(1, *kern)
    elif kind == "position":
        h.set_position_factors(C["pose"], C["z"], C["info"], C["arm"], *kern)
    else:
        h.set_landmark_priors(C["lm"], C["xyz"], C["info"], *kern)


CHI = {"prior": "prior_chi_squares", "relative": "relative_pose_chi_squares", "position": "position_factor_chi_squares", "landmark": "landmark_prior_chi_squares"}


def readings(scene, kind, precision, robust):
    """everything the tests compare, of one handle (kind None: the factor-free twin): per mode the blocks {(row, col): 6 x 6}, bp, bsc and
    lm_sys, then the per-factor chi2 and the objective"""
    def make():
        fp = scene_graph(scene)
        h = HipSolver(fp, RK_NONE, precision=precision)
        if kind is not None:
            attach(h, kind, tm.fixture()[scene][kind], robust)
        out = {"F": h.compute_errors(), "chi": getattr(h, CHI[kind])() if kind is not None else None}
        for mode in (0, 1):
            if mode == 0:
                h.build_system()
                h.assemble()
            else:
                h.set_lambda(0.0)
                h.schur()
            v = h.hsc()[2]
            out[mode] = {"blocks": {key: v[b].copy() for key, b in block_index(h).items()}, "bp": h.array("bp").reshape(-1, 6),
                         "bsc": h.array("bsc").reshape(-1, 6), "lm_sys": h.array("lm_sys").reshape(-1, 9)}
        h.close()
        return out
    return cached(("readings", scene, kind, precision, robust), make)


def weights(kind, scene, C, precision, robust):
    """per case (B, w, dw, rho, drho): the regime's bound, the expected weight and objective term and how far the kernel's conditioning
    lets them be off"""
    out = []
    for k, reg in enumerate(tm.regimes(kind, scene, C)):
        B = tm.bound(reg, precision)
        if robust:
            dw, dr = tm.kernel_window(C["kind"][k], C["delta"][k], C["e"][k], B)
            out.append((B, float(C["w"][k]), dw, float(C["rho"][k]), B * tm.rho_scale(C["kind"][k], C["delta"][k], C["rho"][k]) + dr))
        else:
            out.append((B, 1.0, 0.0, float(C["e"][k]), B * float(C["e"][k])))
    return out


class Sums:
    """an expected sum of weighted terms with the error it may have"""

    def __init__(self, shape):
        self.want, self.tol, self.cases, self.scale = np.zeros(shape), 0.0, [], 0.0

    def add(self, k, term, w, rel, scale=None):
        s = float(np.abs(term).max()) if scale is None else float(scale)
        self.want += w * term
        self.tol += rel * s
        self.scale += w * s
        self.cases.append(k)

    def upper(self):
        """the upper triangle of a 6 x 6 sum"""
        u = Sums(21)
        u.want, u.tol, u.cases, u.scale = self.want[UP], self.tol, self.cases, self.scale
        return u


def expectations(kind, scene, precision, robust):
    """{pose: (H, g)} and {(row, col): X} of a pose-factor kind as Sums; the landmark priors' {landmark: (H packed + b)}"""
    S = tm.fixture()[scene]
    C = S[kind]
    Pf, n = tm.free_poses(S), len(C["e"])
    W = weights(kind, scene, C, precision, robust)
    zero, L = tm.zero_residual(C), tm.length_scale(kind, S, C)
    om = np.abs(C["info"]).reshape(n, -1).max(axis=1)
    diag, grad, cross = {}, {}, {}
    for k in range(n):
        B, w, dw, _, _ = W[k]
        rel = B * w + dw
        if kind == "relative":
            ends = [(int(C["i"][k]), "Hii", "gi"), (int(C["j"][k]), "Hjj", "gj")]
        else:
            ends = [(int(C["lm" if kind == "landmark" else "pose"][k]), "H", "g")]
        for p, hn, gn in ends:
            if kind != "landmark" and p >= Pf:
                continue
            dim = C[gn].shape[1]
            diag.setdefault(p, Sums((dim, dim))).add(k, C[hn][k], w, rel)
            grad.setdefault(p, Sums(dim)).add(k, C[gn][k], w, rel, np.sqrt(np.abs(C[hn][k]).max() * om[k]) * L[k] if zero[k] else None)
        if kind == "relative" and ends[0][0] < Pf and ends[1][0] < Pf:
            i, j = ends[0][0], ends[1][0]
            cross.setdefault((min(i, j), max(i, j)), Sums((6, 6))).add(k, C["Hij"][k] if i < j else C["Hij"][k].T, w, rel)
    return diag, grad, cross, W


def off_by(got, s, floor):
    """(error / what it may be, error relative to the term)"""
    err = float(np.abs(got - s.want).max())
    may = s.tol + floor
    return (0.0 if err == 0 else err / may if may > 0 else np.inf), err / s.scale if s.scale > 0 else 0.0


def check(scene, kind, precision, robust):
    """-> {regime: worst error relative to its own term} over the cases with a weight that resolves it; asserts every case"""
    S = tm.fixture()[scene]
    C = S[kind]
    regs = tm.regimes(kind, scene, C)
    plain, got = readings(scene, None, precision, False), readings(scene, kind, precision, robust)
    diag, grad, cross, W = expectations(kind, scene, precision, robust)
    eps = EPS_OF[precision]
    worst, failures = {}, []

    def note(name, mode, s, ratio, relerr):
        k = s.cases[0]
        if W[k][1] >= 1e-3:
            worst[regs[k]] = max(worst.get(regs[k], 0.0), relerr)
        if not ratio <= 1.0:
            failures.append("%s mode %d of %s: %.2e of its term, %.1f x what it may be" % (name, mode, " + ".join(tm.describe(scene, kind, c) for c in s.cases), relerr, ratio))

    smallest = min(float(np.abs(C[hn]).max(axis=(1, 2))[tm.end_is_free(kind, S, C, end)].min()) for end, (hn, _) in enumerate(tm.ENDS[kind]))
    for mode in (0, 1):
        a, b = plain[mode], got[mode]
        if kind == "landmark":
            for l, s in diag.items():
                floor = 2 * eps * float(np.abs(a["lm_sys"][l]).max())
                if mode == 0:
                    assert np.abs(a["lm_sys"][l, :6]).max() <= 1e-3 * smallest
                    H = b["lm_sys"][l, :6] - a["lm_sys"][l, :6]
                    note("Hll", mode, s, *off_by(np.array([[H[0], H[1], H[2]], [H[1], H[3], H[4]], [H[2], H[4], H[5]]]), s, floor))
                note("bl", mode, grad[l], *off_by(-(b["lm_sys"][l, 6:] - a["lm_sys"][l, 6:]), grad[l], floor))
            continue
        for p, s in diag.items():
            base = a["blocks"][(p, p)]
            assert np.abs(base).max() <= 1e-3 * smallest
            floor = 2 * eps * float(np.abs(base).max())
            d = b["blocks"][(p, p)] - base
            note("Hpp", mode, s, *off_by(d[UP], s.upper(), floor))
            for name in ("bp", "bsc")[:mode + 1]:
                note(name, mode, grad[p], *off_by(-(b[name][p] - a[name][p]), grad[p], 2 * eps * float(np.abs(a[name][p]).max())))
        if mode == 1:
            for key, s in cross.items():
                base = a["blocks"].get(key, np.zeros((6, 6)))
                note("Hpq", mode, s, *off_by(b["blocks"][key] - base, s, 2 * eps * float(np.abs(base).max())))
    # the per-factor chi2 and the objective
    zero, L = tm.zero_residual(C), tm.length_scale(kind, S, C)
    om = np.abs(C["info"]).reshape(len(C["e"]), -1).max(axis=1)
    tolF = 0.0
    for k in range(len(C["e"])):
        B, _, _, _, dr = W[k]
        scale = om[k] * L[k] ** 2 if zero[k] else float(C["e"][k])
        err = abs(got["chi"][k] - C["e"][k]) / scale
        if not zero[k]:
            worst[regs[k]] = max(worst.get(regs[k], 0.0), err)
        if not err <= B:
            failures.append("chi2 of %s: %.2e, bound %.1e" % (tm.describe(scene, kind, k), err, B))
        tolF += dr + (B * scale if zero[k] else 0.0)
    wantF = sum(x[3] for x in W)
    dF = got["F"] - plain["F"]
    assert plain["F"] <= 1e-3 * wantF
    if not abs(dF - wantF) <= tolF + 4 * eps * (plain["F"] + wantF):
        failures.append("objective: %.17g against %.17g, may be off by %.2e" % (dF, wantF, tolF))
    return worst, failures


def test_the_graph_is_the_fixtures():
    for scene in tm.SCENES:
        scene_graph(scene)


@pytest.mark.parametrize("robust", [False, True], ids=["plain", "robust"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", tm.KINDS)
@pytest.mark.parametrize("scene", tm.SCENES)
def test_factor_terms_against_the_reference(scene, kind, precision, robust):
    worst, failures = check(scene, kind, precision, robust)
    for reg in sorted(worst):
        print("%s %s %s %s: %s / %s worst %.2e (bound %.1e)" % (scene, kind, precision, "robust" if robust else "plain", reg[0], reg[1], worst[reg], tm.bound(reg, precision)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", tm.KINDS)
@pytest.mark.parametrize("scene", tm.SCENES)
def test_the_two_instantiations_agree_without_a_kernel(scene, kind, precision):
    """kind none under ROBUST = true is ROBUST = false, to the regime's bound, on every vertex whose cases carry no kernel"""
    S = tm.fixture()[scene]
    C = S[kind]
    a, b = readings(scene, kind, precision, False), readings(scene, kind, precision, True)
    diag, grad, cross, W = expectations(kind, scene, precision, False)
    worst = 0.0

    def agree(x, y, s):
        nonlocal worst
        if any(C["kind"][k] != 0 for k in s.cases):
            return
        err = float(np.abs(x - y).max()) / float(np.abs(y).max())
        worst = max(worst, err / W[s.cases[0]][0])
        assert err <= W[s.cases[0]][0], (tm.describe(scene, kind, s.cases[0]), err)

    for mode in (0, 1):
        for p, s in diag.items():
            if kind == "landmark":
                agree(a[mode]["lm_sys"][p], b[mode]["lm_sys"][p], s)
                continue
            agree(a[mode]["blocks"][(p, p)][UP], b[mode]["blocks"][(p, p)][UP], s)
            for name in ("bp", "bsc")[:mode + 1]:
                agree(a[mode][name][p], b[mode][name][p], s)
        if mode == 1:
            for key, s in cross.items():
                agree(a[mode]["blocks"][key], b[mode]["blocks"][key], s)
    plain = C["kind"] == 0
    assert plain.any() and not plain.all()
    err = np.abs(a["chi"] - b["chi"])[plain] / b["chi"][plain]
    assert np.all(err <= np.array([x[0] for x in W])[plain])
    print("%s %s %s: the instantiations differ by at most %.2e of the bound" % (scene, kind, precision, worst))

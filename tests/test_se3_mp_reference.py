"""The numpy models of the factors (prior_reference, relative_pose_reference, position_factor_reference, landmark_prior_reference and the
kernels of robust_pose_factor_reference) against the 60-digit reference of tests/se3_mp_reference.py, over the case table recorded in
tests/golden/se3_cases.npz (tests/golden/make_golden_se3_cases.py): every branch of the SE(3) logarithm and of J_l^-1, both signs of the
relative quaternion, angles up to pi - 1e-6, pose translations of ~10 ("near") and ~1e3 ("moved"), every side of every robust kernel.

This module also holds what tests/test_gpu_factor_regimes.py shares with it: the fixture's reader, the error measure, the regimes and
their bounds.

ERROR MEASURE.  Per case and quantity (H = J^T Omega J per free end, H_ij, g = J^T Omega r per free end, e = r^T Omega r):
max |got - want| / max |want| over the entries of that quantity alone.  A case with a prescribed ZERO residual (ratio 0 of the kernel
table) has g = e = 0 up to the rounding of its inputs; there g is measured against sqrt(max|H| max|Omega|) L and e against max|Omega| L^2,
L = max(1, the largest coordinate that enters the residual): what an error of the residual of B L, the conditioning of a difference of
numbers of size L, makes of them.

REGIMES AND BOUNDS.  A regime is {series: theta < 0.25, closed: theta >= 0.25} x scene for the SE(3) factors and "vector" x scene for the
position factors and landmark priors (no logarithm).  MODEL_ERROR holds the largest error of the numpy models in each regime, measured by
test_models_against_the_reference below (which keeps the table honest within a factor 3); the bound the GPU kernels are held to is
16 x that, at least 32 eps (the factor covers FMA contraction and the kernels' order in their six-term sums), times 2^29 for the fp32
library.  Measured over the committed table:

    regime            model error   bound (fp64)   bound (fp32)     the model's worst case
    series / near       9.6e-14       1.5e-12        8.2e-04        H_jj of a relative edge at theta = 0.2499 (series truncation)
    closed / near       9.7e-15       1.6e-13        8.3e-05        g_i of a relative edge at theta = 3.1
    series / moved      9.5e-13       1.5e-11        8.2e-03        e of a relative edge at theta = 1e-3 (t - R tbar at |t| ~ 1e3)
    closed / moved      6.5e-13       1.0e-11        5.6e-03        g_i of a relative edge at theta = 0.5
    vector / near       1.3e-14       2.1e-13        1.1e-04        e of a position factor (R^T (a - t) - z at |t| ~ 10, |r| ~ 0.5)
    vector / moved      3.8e-12       6.1e-11        3.3e-02        e of a position factor (the same at |t| ~ 1e3)

Series against closed form at the switch, pose priors alone: 6.8e-14 at theta = 0.2499 against 1.3e-15 at 0.2501 ("near"; 2.6e-13 against
6.0e-14 "moved"): just below the switch the four-term series of d, c1, c2, c3 is 50 x less accurate than the closed form just above it.
That is the truncation of the series (the first dropped term of c1 is theta^8 / 11!, 2.3e-12 of c1 at 0.25), shared by the kernels; it is recorded here, not fixed.

ROBUST KERNELS.  w = rho'(e) and rho(e) inherit the error of e through their own conditioning, which is unbounded at Tukey's double zero
(e / delta^2 = 1 - 1e-9: w = 1e-18, d log w / d log e = 2e9) and undefined at a kink.  kernel_window() therefore allows, besides B
relative, the variation of w / rho over e (1 +- 2 B) (B for e, B for delta^2 in the library's precision): to first order B (1 + kappa)
relative, and across a kink or onto w = 0 exactly what the two sides differ by."""
import os
import sys

import numpy as np
import pytest

import landmark_prior_reference as lr
import position_factor_reference as pfr
import prior_reference as pr
import relative_pose_reference as rr
import robust_pose_factor_reference as rf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "se3_cases.npz")
SCENES = ("near", "moved")
KINDS = ("prior", "relative", "position", "landmark")
EPS = float(np.finfo(np.float64).eps)
SWITCH, LOG_SWITCH = 0.25, 1e-4

# the largest error of the numpy models against the fixture per regime (see the module docstring)
MODEL_ERROR = {
    ("series", "near"): 9.6e-14, ("closed", "near"): 9.7e-15,
    ("series", "moved"): 9.5e-13, ("closed", "moved"): 6.5e-13,
    ("vector", "near"): 1.3e-14, ("vector", "moved"): 3.8e-12,
}


def bound(regime, precision="f64"):
    """what a kernel may be off by in a regime: 16 x the model's error there, at least 32 eps; x 2^29 = eps32 / eps64 on the fp32 library"""
    return max(16.0 * MODEL_ERROR[regime], 32.0 * EPS) * (2.0 ** 29 if precision == "f32" else 1.0)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------------
_fixture = {}


def fixture():
    """{scene: {"q", "t", kind: {name: array}}}, read once"""
    if not _fixture:
        with np.load(PATH) as z:
            for key in z.files:
                parts = key.split("/")
                d = _fixture.setdefault(parts[0], {})
                if len(parts) == 2:
                    d[parts[1]] = z[key]
                else:
                    d.setdefault(parts[1], {})[parts[2]] = z[key]
    return _fixture


def free_poses(S):
    return len(S["q"]) - 1          # (the graph's one fixed pose is the last of the solver numbering)


def thetas(C):
    return np.linalg.norm(C["r"][:, :3], axis=1)


def regimes(kind, scene, C):
    """the regime of every case of a set, from the fixture's r"""
    if kind in ("position", "landmark"):
        return [("vector", scene)] * len(C["e"])
    return [("series" if th < SWITCH else "closed", scene) for th in thetas(C)]


def zero_residual(C):
    return C["ratio"] == 0.0


def length_scale(kind, S, C):
    """L of the module docstring, per case"""
    t = np.abs(S["t"]).max(axis=1)
    if kind == "prior":
        L = np.maximum(t[C["pose"]], np.abs(C["tb"]).max(axis=1))
    elif kind == "relative":
        L = np.maximum(np.maximum(t[C["i"]], t[C["j"]]), np.abs(C["tz"]).max(axis=1))
    elif kind == "position":
        L = np.maximum(t[C["pose"]], np.abs(C["z"]).max(axis=1))
    else:
        L = np.abs(C["X"]).max(axis=1)
    return np.maximum(L, 1.0)


ENDS = {"prior": (("H", "g"),), "relative": (("Hii", "gi"), ("Hjj", "gj")), "position": (("H", "g"),), "landmark": (("H", "g"),)}


def end_is_free(kind, S, C, end):
    if kind == "relative":
        return C["ij"[end]] < free_poses(S)
    return np.ones(len(C["e"]), dtype=bool)


def relmax(got, want, scale=None):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    s = np.abs(want).max() if scale is None else scale
    return float(np.abs(got - want).max() / s) if s > 0 else float(np.abs(got - want).max())


def case_errors(kind, S, C, got):
    """the error measure of the module docstring: got = {name: array} shaped like the fixture's outputs -> per case the largest error over
    the quantities, and which quantity it was"""
    n = len(C["e"])
    zero, L = zero_residual(C), length_scale(kind, S, C)
    om = np.abs(C["info"]).reshape(n, -1).max(axis=1)
    worst, which = np.zeros(n), [""] * n
    for k in range(n):
        errs = {}
        for end, (hn, gn) in enumerate(ENDS[kind]):
            if not end_is_free(kind, S, C, end)[k]:
                continue
            errs[hn] = relmax(got[hn][k], C[hn][k])
            errs[gn] = relmax(got[gn][k], C[gn][k], np.sqrt(np.abs(C[hn][k]).max() * om[k]) * L[k] if zero[k] else None)
        if kind == "relative" and end_is_free(kind, S, C, 0)[k] and end_is_free(kind, S, C, 1)[k]:
            errs["Hij"] = relmax(got["Hij"][k], C["Hij"][k])
        errs["e"] = relmax(got["e"][k], C["e"][k], om[k] * L[k] ** 2 if zero[k] else None)
        which[k] = max(errs, key=errs.get)
        worst[k] = errs[which[k]]
    return worst, which


# ---- robust kernels ----------------------------------------------------------------------------------------------------------------------
def kernel_window(kind, delta, e, B):
    """(dw, drho): the variation of rho'(e) and rho(e) of a kernel over e (1 +- 2 B) -- what an error of B in e and of B in delta^2 may
    move them by, on top of their own relative error B (0 for kind none)"""
    kind, delta, e = int(kind), float(delta), float(e)
    w0, r0 = rf.weight(kind, delta, e), rf.rho(kind, delta, e)
    dw = dr = 0.0
    for x in (e * (1 - 2 * B), e * (1 + 2 * B)):
        dw = max(dw, abs(rf.weight(kind, delta, x) - w0))
        dr = max(dr, abs(rf.rho(kind, delta, x) - r0))
    return dw, dr


def rho_scale(kind, delta, rho):
    """what the relative error of rho(e) refers to: rho itself, except under Tukey, whose form delta^2 / 3 (1 - (1 - e / delta^2)^3) is
    good to eps delta^2 / 3, not to eps rho, as e -> 0"""
    return max(float(rho), float(delta) ** 2 / 3) if int(kind) == rf.TUKEY else float(rho)


# ---- the numpy models over the table -------------------------------------------------------------------------------------------------------
def model_outputs(kind, S, C, ad_identity=False):
    """what the numpy models make of a set's inputs, shaped like the fixture's outputs"""
    Pf, n = free_poses(S), len(C["e"])
    out = {"e": np.zeros(n)}
    for hn, gn in ENDS[kind]:
        out[hn], out[gn] = np.zeros_like(C[hn]), np.zeros_like(C[gn])
    if kind == "prior":
        for k, (e, _, H, g) in enumerate(pr.prior_terms((C["pose"], C["qb"], C["tb"], C["info"]), S["q"], S["t"], Pf)):
            out["e"][k], out["H"][k], out["g"][k] = e, H, g
    elif kind == "relative":
        out["Hij"] = np.zeros_like(C["Hij"])
        for k, (e, _, _, Ji, Jj, Om, r) in enumerate(rr.rel_terms((C["i"], C["j"], C["qz"], C["tz"], C["info"]), S["q"], S["t"], Pf, ad_identity)):
            out["e"][k] = e
            if Ji is not None:
                out["Hii"][k], out["gi"][k] = Ji.T @ Om @ Ji, Ji.T @ Om @ r
            if Jj is not None:
                out["Hjj"][k], out["gj"][k] = Jj.T @ Om @ Jj, Jj.T @ Om @ r
            if Ji is not None and Jj is not None:
                out["Hij"][k] = Ji.T @ Om @ Jj
    elif kind == "position":
        for k, (e, _, _, _, J, Om, r) in enumerate(pfr.factor_terms((C["pose"], C["z"], C["info"], C["arm"], None, None), S["q"], S["t"], Pf)):
            out["e"][k], out["H"][k], out["g"][k] = e, J.T @ Om @ J, J.T @ Om @ r
    else:
        Lf = int(C["lm"].max()) + 1
        X = np.zeros((Lf, 3))
        X[C["lm"]] = C["X"]
        for k, (e, _, _, _, Om, r) in enumerate(lr.prior_terms((C["lm"], C["xyz"], C["info"], None, None), X, Lf)):
            out["e"][k], out["H"][k], out["g"][k] = e, Om, Om @ r
    return out


def model_errors(kinds=KINDS, **how):
    """[(scene, kind, case, regime, error, quantity)] of the numpy models over the table"""
    rows = []
    for scene in SCENES:
        S = fixture()[scene]
        for kind in kinds:
            C = S[kind]
            worst, which = case_errors(kind, S, C, model_outputs(kind, S, C, **how))
            rows += [(scene, kind, k, reg, worst[k], which[k]) for k, reg in enumerate(regimes(kind, scene, C))]
    return rows


def describe(scene, kind, k):
    C = fixture()[scene][kind]
    th = "theta %.7g, " % C["theta"][k] if "theta" in C else ""
    return "%s %s case %d (%skernel %d, ratio %g)" % (scene, kind, k, th, C["kind"][k], C["ratio"][k])


# ---- the fixture itself ----------------------------------------------------------------------------------------------------------------------
def test_the_table_holds_every_branch():
    for scene in SCENES:
        S = fixture()[scene]
        assert (S["q"][:, 3] < 0).any() and (S["q"][:, 3] > 0).any()
        assert np.abs(S["t"]).max() > (500 if scene == "moved" else 1) and (scene == "moved" or np.abs(S["t"]).max() < 100)
        for kind in ("prior", "relative"):
            C = S[kind]
            th = thetas(C)
            n = np.sin(0.5 * th)
            # no case within rounding of a switch: the branch a kernel takes is the one the fixture's r says
            assert np.all(np.abs(th - SWITCH) > 1e-6) and np.all(np.abs(n - LOG_SWITCH) > 1e-6) and np.all(th < np.pi - 1e-7)
            given = ~zero_residual(C)          # the angle that came out is the one prescribed
            assert np.abs(th[given] - C["theta"][given]).max() < 1e-12
            for branch in (n < LOG_SWITCH, n >= LOG_SWITCH, th < SWITCH, th >= SWITCH, C["flip"], ~C["flip"]):
                assert branch.any()
            # both branches of J_l^-1 under both signs, and under a negated estimate
            ends = C["pose"] if kind == "prior" else C["j"]
            neg = S["q"][ends, 3] < 0
            assert (C["flip"] & (th >= SWITCH)).any() and (C["flip"] & (th < SWITCH)).any() and (C["flip"] & (n < LOG_SWITCH)).any() and neg.any()
        P = S["prior"]
        assert sorted(set(np.round(P["theta"][P["kind"] == 0], 12))) == sorted(set(np.round([0.0, 1e-9, 1e-6, 1.9e-4, 2.1e-4, 1e-3, 0.05, 0.2499, 0.2501, 0.5, 2.0, 3.1, np.pi - 1e-6], 12)))
        assert np.any(np.abs(np.linalg.norm(P["qb"], axis=1) - 1.001) < 1e-9)
        R = S["relative"]
        assert set(R["pair"]) == {0, 1, 2, 3, 4} and (R["i"] > R["j"])[R["pair"] == 2].all() and (R["i"] < R["j"])[R["pair"] <= 1].all()
        far = (R["pair"] == 1) & (R["i"] == 0) & (R["j"] == free_poses(S) - 1)          # the far pair: first against last free pose, at an angle
        assert far.sum() == 1 and thetas(R)[far][0] > 1e-4
        assert sorted(set(np.round(R["theta"][R["kind"] == 0], 12))) == sorted({0.0, 1e-3, 0.05, 0.2499, 0.5, 2.0, 3.1})
        th, plain = thetas(R), R["kind"] == 0
        for pk in (0, 1, 2, 3):          # every store meets the series, the closed form at 0.5, 2 and 3.1, and both signs of the quaternion
            m = plain & (R["pair"] == pk)
            assert (th[m] < SWITCH).any() and {0.5, 2.0, 3.1} <= set(np.round(R["theta"][m], 12)) and R["flip"][m].any() and (~R["flip"][m]).any()
        for kern in (rf.HUBER, rf.TUKEY, rf.CAUCHY):          # every kernel weighs a cross block, with and without Schur products
            m = R["kind"] == kern
            assert set(R["pair"][m]) == {0, 1, 3} and sorted(R["ratio"][m & (R["pair"] != 3)]) == [0.25, 4.0]
        fixed = free_poses(S)
        assert ((R["i"] == fixed) & (R["pair"] == 3)).any() and ((R["j"] == fixed) & (R["pair"] == 3)).any()
        assert (np.abs(S["position"]["arm"]).max(axis=1) == 0).any() and (np.abs(S["position"]["arm"]).max(axis=1) > 0).any()
        for kind in KINDS:
            C = S[kind]
            if kind != "relative":          # one case per vertex
                assert len(set(C["lm" if kind == "landmark" else "pose"])) == len(C["e"])
            for kern in (rf.HUBER, rf.TUKEY, rf.CAUCHY):
                m = C["kind"] == kern
                assert sorted(C["ratio"][m]) == [0.0, 0.25, 1 - 1e-9, 1 + 1e-9, 4.0, 1e6]
                x = C["e"][m & ~zero_residual(C)] / C["delta"][m & ~zero_residual(C)] ** 2
                assert np.abs(x / C["ratio"][m & ~zero_residual(C)] - 1).max() < 1e-14          # (safely on its side: the margin is 1e-9)
                assert np.all(C["e"][m & zero_residual(C)] < 1e-20)


def test_the_table_regenerates_bit_for_bit():
    pytest.importorskip("mpmath")
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_se3_cases
    new = make_golden_se3_cases.generate()
    with np.load(PATH) as z:
        assert sorted(z.files) == sorted(new)
        for key in z.files:
            assert z[key].dtype == new[key].dtype and z[key].shape == new[key].shape and z[key].tobytes() == new[key].tobytes(), key


# ---- the models against the table ----------------------------------------------------------------------------------------------------------
def test_models_against_the_reference():
    rows = model_errors()
    measured = {}
    for scene, kind, k, reg, err, which in rows:
        if err > measured.get(reg, (-1.0,))[0]:
            measured[reg] = (err, describe(scene, kind, k), which)
    print()
    for reg in MODEL_ERROR:
        err, where, which = measured[reg]
        print("%-6s / %-5s  model error %.1e (%s of %s)  recorded %.1e  bound fp64 %.1e  fp32 %.1e"
              % (reg[0], reg[1], err, which, where, MODEL_ERROR[reg], bound(reg), bound(reg, "f32")))
    # the series just below the switch against the closed form just above it (the truncation of the four-term series)
    for scene in SCENES:
        for th in (0.2499, 0.2501):
            e = max(err for s, kind, k, _, err, _ in rows if s == scene and kind == "prior" and abs(fixture()[s][kind]["theta"][k] - th) < 1e-9)
            print("priors at theta = %.4f, %s: %.1e" % (th, scene, e))
    for reg in MODEL_ERROR:
        assert MODEL_ERROR[reg] / 3 <= measured[reg][0] <= 3 * MODEL_ERROR[reg], (reg, measured[reg])


def test_kernel_models_against_the_reference():
    B, worst = 32 * EPS, 0.0
    for scene in SCENES:
        for kind in KINDS:
            C = fixture()[scene][kind]
            for k in range(len(C["e"])):
                dw, dr = kernel_window(C["kind"][k], C["delta"][k], C["e"][k], B)
                ew = abs(rf.weight(int(C["kind"][k]), float(C["delta"][k]), float(C["e"][k])) - C["w"][k])
                er = abs(rf.rho(int(C["kind"][k]), float(C["delta"][k]), float(C["e"][k])) - C["rho"][k])
                assert ew <= B * C["w"][k] + dw and er <= B * rho_scale(C["kind"][k], C["delta"][k], C["rho"][k]) + dr, describe(scene, kind, k)
                if C["w"][k] > 0 and abs(C["ratio"][k] - 1) > 1e-6 and C["ratio"][k] != 0.0:
                    worst = max(worst, ew / C["w"][k], er / C["rho"][k] if C["rho"][k] > 0 else 0.0)
    print("rho / rho' of the numpy kernels away from e = delta^2: max rel %.1e" % worst)
    assert worst <= 8 * EPS


# ---- mutants: the bound of the GPU test tells a subtly wrong formula from a right one --------------------------------------------------------
def se3_q_variant(w, u, mutant=None):
    """prior_reference.se3_q, optionally with one deliberate error"""
    th = np.linalg.norm(w)
    W, P = pr.hat(w), pr.hat(u)
    if th < 0.25:
        t2 = th * th
        c1 = 1.0 / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880
        c2 = 1.0 / 24 - t2 / 720 + t2 * t2 / 40320 - t2 ** 3 / 3628800
        c3 = 1.0 / 120 - t2 / 2520 + t2 * t2 / 120960 - t2 ** 3 / 9979200
    else:
        s, c = np.sin(th), np.cos(th)
        c1 = (th - s) / th ** 3
        c2 = (th * th / 2 + c - 1) / th ** 4
        c3 = 0.5 * (c2 + 3 * (th - s - th ** 3 / 6) / th ** 5)
    if mutant == "c3":
        c3 *= 0.98
    WP, PW, WPW = W @ P, P @ W, W @ P @ W
    k = 0.0 if mutant == "wpw" else 3.0
    return 0.5 * P + c1 * (WP + PW + WPW) + c2 * (W @ WP + PW @ W - k * WPW) + c3 * (WPW @ W + W @ WPW)


def so3_jl_inv_cos_one(w):
    """prior_reference.so3_jl_inv with cos -> 1 in the closed form of d"""
    th = np.linalg.norm(w)
    W = pr.hat(w)
    if th < 0.25:
        d = 1.0 / 12 + th * th / 720 + th ** 4 / 30240 + th ** 6 / 1209600
    else:
        d = (1 - 0.5 * th * 1.0 / np.sin(0.5 * th)) / th ** 2
    return np.eye(3) - 0.5 * W + d * W @ W


def so3_log_quat_no_flip(q):
    """prior_reference.so3_log_quat without the sign flip for a negative scalar part"""
    q = np.asarray(q, dtype=np.float64)
    n = np.linalg.norm(q[:3])
    s = 2.0 / q[3] * (1.0 - (n / q[3]) ** 2 / 3.0) if n < 1e-4 else 2.0 * np.arctan2(n, q[3]) / n
    return s * q[:3]


MUTANTS = {
    "wrong c3": ("se3_q", lambda w, u: se3_q_variant(w, u, "c3")),
    "-3 WPW dropped": ("se3_q", lambda w, u: se3_q_variant(w, u, "wpw")),
    "cos -> 1 in d": ("so3_jl_inv", so3_jl_inv_cos_one),
    "no sign flip": ("so3_log_quat", so3_log_quat_no_flip),
    "Ad -> identity": (None, None),
}


def test_the_variant_without_a_mutation_is_the_model():
    rng = np.random.default_rng(0)
    for th in (0.1, 0.7, 3.0):
        w, u = th * np.array([0.6, 0.0, 0.8]), rng.normal(size=3)
        assert np.array_equal(se3_q_variant(w, u), pr.se3_q(w, u))


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_mutant_breaks_the_bound(name, monkeypatch):
    attr, fn = MUTANTS[name]
    if attr is None:
        rows = model_errors(("relative",), ad_identity=True)
    else:
        monkeypatch.setattr(pr, attr, fn)
        rows = model_errors(("prior", "relative"))
    caught = [(err / bound(reg), scene, kind, k, which) for scene, kind, k, reg, err, which in rows if err > bound(reg)]
    assert caught, name
    ratio, scene, kind, k, which = max(caught)
    print("\n%s: caught by %d cases, most clearly by %s: %s off by %.1e x its bound" % (name, len(caught), describe(scene, kind, k), which, ratio))
    # ... and by a margin no rounding explains
    assert ratio > 1e3

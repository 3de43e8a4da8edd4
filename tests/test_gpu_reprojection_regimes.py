"""The reprojection-edge kernels (csrc/ba_math.hpp; the landmark, pose and block passes of csrc/ba_linearize.hip; chi2, back-substitution
and the state update of csrc/ba_edge.hip) against the 60-digit reference recorded in tests/golden/reprojection_cases.npz, stage by stage
through the C ABI: camera-frame depths from 0.5 to 2e4, X / Z of 0 and +-1.5, mono and stereo edges on one landmark, landmarks seen once,
fixed vertices, e / delta^2 on every side of Huber's and Tukey's thresholds per edge type ("regimes", near and moved by ~1e3); landmarks
with 1 ... 63, 64, 65 ... 271 observations, poses with 1, 63, 64, 65 and 129 edges, pose pairs sharing 1, 15, 16, 17, 64 and 65 landmarks,
a pose that sees a landmark twice ("counts"); and pose_exp_update in every branch (theta from 0 to pi + 0.5, the three Shepperd branches,
both signs of the composed quaternion; "update").  This module reads the fixture only (no mpmath; the inputs of the counts scene come from
plain arithmetic and are checked against the fixture's sums); tests/test_reprojection_mp_reference.py holds the error measure, the regimes
and the bounds, and shows on the CPU that eleven subtly wrong formulas break these bounds.

SETTINGS.  The fp64 library, the fp32 library, and the fp64 library with mixed_precision = 1, whose landmark outputs (lm_sys, xl) are held
to the fp64 bounds and whose pose and block outputs (hsc, bp, bsc, and the gain-ratio denominator that sums bp) to the fp32 bounds: their
per-edge arithmetic is float, only the sums are double.  The counts scene runs with landmark_reorder = 0, so that the waves are packed in
the order the scene lists its landmarks (63 + 1 | 2 + 3 + 59 | 64 | the big ones), and once more with device_setup = 0: identical bits.

TOLERANCE.  Per regime max(16 x model error, 32 eps), x 2^29 for fp32 arithmetic (test_reprojection_mp_reference.MODEL_ERROR); the pose
update per band of theta 16 x the error of the model run at the library's precision (UPDATE_MODEL_ERROR).  Worst errors measured on the
MI355X (every test prints its own):

    regime                        model error   bound (fp64)   bound (fp32)     worst on the MI355X: fp64     fp32      mixed
    residual, Z ~ 0.5, near         2.5e-12       4.0e-11        2.1e-02                          2.5e-12   1.2e-03   2.5e-12
    residual, Z ~ 8, near           2.8e-13       4.5e-12        2.4e-03                          4.1e-13   2.5e-04   4.1e-13
    residual, Z ~ 400, near         1.3e-12       2.1e-11        1.1e-02                          1.4e-12   7.8e-04   1.4e-12
    residual, Z ~ 2e4, near         5.8e-13       9.3e-12        5.0e-03                          5.0e-13   3.6e-04   5.0e-13
    residual, Z ~ 0.5, moved        4.2e-10       6.7e-09        3.6e+00                          2.3e-10   1.2e-01   2.3e-10
    residual, Z ~ 8, moved          2.4e-11       3.8e-10        2.1e-01                          2.4e-11   9.7e-03   2.4e-11
    residual, Z ~ 400, moved        1.2e-12       1.9e-11        1.0e-02                          1.7e-12   7.0e-04   1.7e-12
    residual, Z ~ 2e4, moved        5.8e-13       9.3e-12        5.0e-03                          7.6e-13   2.9e-04   7.6e-13
    direct, Z ~ 0.5, near           3.1e-12       5.0e-11        2.7e-02                          3.1e-12   1.2e-03   1.3e-07
    direct, Z ~ 8, near             1.1e-12       1.8e-11        9.4e-03                          1.1e-12   4.0e-04   2.1e-07
    direct, Z ~ 400, near           7.8e-13       1.2e-11        6.7e-03                          7.0e-13   2.9e-04   1.3e-07
    direct, Z ~ 2e4, near           4.7e-13       7.5e-12        4.0e-03                          4.5e-13   2.0e-04   2.0e-07
    direct, Z ~ 0.5, moved          2.1e-10       3.4e-09        1.8e+00                          1.6e-10   2.0e-01   1.3e-07
    direct, Z ~ 8, moved            1.4e-11       2.2e-10        1.2e-01                          1.4e-11   7.5e-03   2.1e-07
    direct, Z ~ 400, moved          8.5e-13       1.4e-11        7.3e-03                          1.0e-12   9.5e-04   1.3e-07
    direct, Z ~ 2e4, moved          1.1e-12       1.8e-11        9.4e-03                          5.3e-13   1.6e-04   2.0e-07
    schur, Z ~ 0.5, near            2.5e-13       4.0e-12        2.1e-03                          2.6e-13   1.9e-04   1.0e-07
    schur, Z ~ 8, near              5.5e-14       8.8e-13        4.7e-04                          9.4e-14   3.8e-05   1.4e-07
    schur, Z ~ 400, near            6.6e-13       1.1e-11        5.7e-03                          7.0e-13   1.9e-04   1.7e-07
    schur, Z ~ 2e4, near            4.5e-13       7.2e-12        3.9e-03                          4.5e-13   1.3e-04   2.0e-07
    schur, Z ~ 0.5, moved           4.3e-11       6.9e-10        3.7e-01                          4.3e-11   1.9e-02   1.0e-07
    schur, Z ~ 8, moved             3.2e-12       5.1e-11        2.7e-02                          3.5e-12   2.4e-03   1.4e-07
    schur, Z ~ 400, moved           6.4e-13       1.0e-11        5.5e-03                          6.4e-13   8.5e-04   1.7e-07
    schur, Z ~ 2e4, moved           6.0e-13       9.6e-12        5.2e-03                          5.3e-13   1.3e-04   2.0e-07
    residual, counts                8.2e-12       1.3e-10        7.0e-02                          6.7e-12   7.9e-03   6.7e-12
    direct, counts                  9.2e-13       1.5e-11        7.9e-03                          6.9e-13   3.8e-04   1.1e-07
    schur, counts                   3.4e-13       5.4e-12        2.9e-03                          3.4e-13   1.2e-04   1.8e-07

    update, band of theta         float64 model   bound     MI355X fp64      float32 model   bound     MI355X fp32
    [0, 1e-5)                       1.5e-16      7.1e-15   2.2e-16          1.1e-07      3.8e-06   1.1e-07
    [1e-5, 3.4e-4)                  6.2e-13      9.9e-12   6.2e-13          1.5e-05      2.4e-04   1.5e-05
    [3.4e-4, 1e-2)                  2.9e-15      4.6e-14   2.9e-15          8.6e-06      1.4e-04   8.6e-06
    [1e-2, 2 pi / 3)                1.1e-15      1.8e-14   6.7e-16          5.4e-07      8.6e-06   4.0e-07
    [2 pi / 3, pi)                  5.4e-16      8.6e-15   5.6e-16          4.0e-07      6.4e-06   2.1e-07
    [pi, ...)                       4.6e-16      7.4e-15   4.5e-16          2.2e-07      3.8e-06   2.2e-07

(mixed: the landmark families are held to the fp64 bound, the pose and block families to the fp32 bound; the update under mixed is the fp64
library's, bit for bit.)
"""
import numpy as np
import pytest

import test_reprojection_mp_reference as tr
from test_gpu_relative_pose import block_index

from cuba_amd.capi import HipSolver
from cuba_amd.dist import _DeviceArray
from cuba_amd.graph import FlatProblem

pytestmark = pytest.mark.gpu

SETTINGS = ("f64", "f32", "mixed")
LIBRARY = {"f64": "f64", "f32": "f32", "mixed": "f64"}
POSE_SIDE = ("Hpp", "bp", "hdiag", "bsc", "hoff")
STAGE_SCENES = [(scene, s) for scene in tr.LINEAR_SCENES for s in tr.settings_of(scene)]

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def flat(G):
    Pt, Lt, E = len(G["q"]), len(G["X"]), len(G["eP"])
    return FlatProblem(Pt=Pt, Pf=G["Pf"], Lt=Lt, Lf=G["Lf"], q=np.ascontiguousarray(G["q"]), t=np.ascontiguousarray(G["t"]), cam=np.ascontiguousarray(G["cam"]),
                       Xw=np.ascontiguousarray(G["X"]), eP=np.asarray(G["eP"], dtype=np.int32), eL=np.asarray(G["eL"], dtype=np.int32),
                       eDim=np.where(G["stereo"], 3, 2).astype(np.uint8), meas=np.ascontiguousarray(G["meas"]), omega=np.ascontiguousarray(G["omega"]),
                       pose_src=np.arange(Pt), lm_src=np.arange(Lt), edge_src=np.arange(E))


def precision_of(setting, name):
    """the precision whose bound a family is held to under a setting"""
    return "f32" if setting == "f32" or (setting == "mixed" and name in POSE_SIDE) else "f64"


def solver(scene, s, setting, **options):
    if scene == "counts":
        options["landmark_reorder"] = 0
    if setting == "mixed":
        options["mixed_precision"] = 1
    return HipSolver(flat(tr.scene_inputs(scene)), tr.kernels_of(scene, s), precision=LIBRARY[setting], **options)


def write_device(h, name, values):
    """values (in the caller's order, as array(name) returns them) -> the device array, whose order is found by a ramp, not assumed"""
    import torch
    ptr, n = h.device_pointer(name)
    dev = torch.as_tensor(_DeviceArray(ptr, n, h.scalar_size), device="cuda")
    dtype = torch.float32 if h.scalar_size == 4 else torch.float64
    dev.copy_(torch.arange(n, dtype=dtype).cuda())
    torch.cuda.synchronize()
    where = h.array(name).astype(np.int64)          # position in the device array of every entry of the caller's array
    assert sorted(where) == list(range(n))
    buf = np.zeros(n)
    buf[where] = np.asarray(values, dtype=np.float64).ravel()
    dev.copy_(torch.from_numpy(buf).to(dtype).cuda())
    torch.cuda.synchronize()
    back = h.array(name)
    assert np.array_equal(back, np.asarray(values, dtype=np.float32 if h.scalar_size == 4 else np.float64).astype(np.float64).ravel())


def diagonal_blocks(h):
    rp, ci, v = h.hsc()
    assert np.array_equal(ci[rp[:-1]], np.arange(len(rp) - 1))
    return v[rp[:-1]]


def readings(scene, s, setting, **options):
    """every stage output the tests compare, of one handle"""
    def make():
        S, G = tr.sub(scene), tr.scene_inputs(scene)
        lam = float(S["s%d/lam" % s][0])
        h = solver(scene, s, setting, **options)
        out = {"F": h.compute_errors(), "e": h.chi_squares()}
        h.build_system()
        out["maxdiag"] = h.max_diagonal()          # (the assembly without damping runs with this call: build_system() alone defers it)
        lm = h.array("lm_sys").reshape(-1, 9)
        out["Hll"], out["bl0"] = tr.sym3_batch(lm[:, :6]), lm[:, 6:].copy()
        out["Hpp"], out["bp"] = diagonal_blocks(h), h.array("bp").reshape(-1, 6)
        if scene == "counts":
            out["Hpp"] = out["Hpp"][G["mode0_poses"]]
        h.set_lambda(lam)
        h.schur()
        lm = h.array("lm_sys").reshape(-1, 9)
        out["inv"], out["bl"] = tr.sym3_batch(lm[:, :6]), lm[:, 6:].copy()
        rp, ci, v = h.hsc()
        index = block_index(h)
        out["hdiag"] = v[rp[:-1]]
        out["hoff"] = np.array([v[index[(int(a), int(b))]] for a, b in S["pairs"]]).reshape(-1, 6, 6)
        out["bsc"], out["bp1"] = h.array("bsc").reshape(-1, 6), h.array("bp").reshape(-1, 6)
        xp = S["xp"] if "xp" in S else tr.chosen_xp(G["Pf"])
        write_device(h, "xp", xp)
        h.back_substitute()
        out["xl"], out["scale"] = h.array("xl").reshape(-1, 3), h.compute_scale(lam)
        out["scale_again"], out["xl_again"] = h.compute_scale(lam), h.array("xl").reshape(-1, 3)
        h.back_substitute()
        out["xl_twice"] = h.array("xl").reshape(-1, 3)
        h.close()
        return out
    return cached((scene, s, setting, tuple(sorted(options.items()))), make)


def report(scene, s, setting, rows):
    worst = tr.worst_per_regime(rows)
    for reg in sorted(worst, key=str):
        err, name, k, may = worst[reg]
        print("%s s%d %s: %s worst %.2e (%s of block %d), may be %.1e" % (scene, s, setting, reg, err, name, k, may))
    return ["%s of block %d in %s: %.2e, may be %.2e" % (name, k, reg, err, may) for name, k, reg, err, may in rows if not err <= may]


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("scene,s", STAGE_SCENES, ids=["%s-s%d" % x for x in STAGE_SCENES])
def test_stage_outputs_against_the_reference(scene, s, setting):
    """chi2 per edge, lm_sys, diagonal blocks and bp after build_system(); the inverse, bl, the diagonal and the listed off-diagonal blocks
    of hsc and bsc after set_lambda() + schur(); xl after back_substitute() with the fixture's xp: every block of every family"""
    got = readings(scene, s, setting)
    rows = []
    for name in tr.families(scene):
        rows += tr.compare(scene, s, got, precision_of(setting, name), select=(name,))
    failures = report(scene, s, setting, rows)
    # bl is the same after either pass, and so is bp (hsc carries no lambda: its diagonal blocks are held to the reference's, which has none)
    again = tr.compare(scene, s, dict(got, bl=got["bl0"]), precision_of(setting, "bl"), select=("bl",)) + tr.compare(scene, s, dict(got, bp=got["bp1"]), precision_of(setting, "bp"), select=("bp",))
    failures += ["(other pass) %s of block %d: %.2e, may be %.2e" % (name, k, err, may) for name, k, _, err, may in again if not err <= may]
    assert not failures, "\n".join(failures[:40])


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("scene,s", STAGE_SCENES, ids=["%s-s%d" % x for x in STAGE_SCENES])
def test_sums_over_the_scene(scene, s, setting):
    """compute_errors() against sum rho, max_diagonal(), and compute_scale() after the back-substitution (twice: idempotent)"""
    S = tr.sub(scene)
    got = readings(scene, s, setting)
    lam, maxdiag, scale, scale_abs = S["s%d/lam" % s]
    Bd, _ = tr.scene_bounds(scene, "f32" if setting == "f32" else "f64")
    Bpose = tr.scene_bounds(scene, precision_of(setting, "bp"))
    slack = tr.objective_slack(scene, s, Bd)
    print("%s s%d %s: F off by %.2e of its slack, max diagonal by %.2e (may be %.1e), scale by %.2e of its terms (may be %.1e)"
          % (scene, s, setting, abs(got["F"] - S["s%d/F" % s][0]) / slack, abs(got["maxdiag"] - maxdiag) / maxdiag, Bpose[0], abs(got["scale"] - scale) / scale_abs, Bpose[1]))
    assert abs(got["F"] - S["s%d/F" % s][0]) <= slack
    assert abs(got["maxdiag"] - maxdiag) <= Bpose[0] * maxdiag
    assert abs(got["scale"] - scale) <= Bpose[1] * scale_abs
    assert got["scale_again"] == got["scale"] and np.array_equal(got["xl_again"], got["xl"]) and np.array_equal(got["xl_twice"], got["xl"])


def test_the_fixed_big_landmark_and_the_zero_weights():
    """counts: the landmark with 100 observations that is fixed takes part in every pose's blocks and has no increment; regimes: a landmark
    all of whose edges have weight 0 has Hll = bl = xl = 0 exactly and the inverse 1 / lambda on its diagonal"""
    G = tr.scene_inputs("counts")
    per_lm = np.bincount(G["eL"], minlength=len(G["X"]))
    assert (per_lm[G["Lf"]:] > 64).any() and readings("counts", 0, "f64")["xl"].shape == (G["Lf"], 3)
    for setting in SETTINGS:
        for s in (1, 2):
            S, got = tr.sub("regimes/near"), readings("regimes/near", s, setting)
            dead = [l for l in range(int(S["sizes"][1])) if np.all(S["s%d/w" % s][S["eL"] == l] == 0)]
            assert len(dead) >= 2
            lam = float(S["s%d/lam" % s][0])
            for l in dead:
                assert not got["Hll"][l].any() and not got["bl"][l].any() and not got["xl"][l].any()
                assert np.allclose(got["inv"][l], np.eye(3) / lam, rtol=1e-6, atol=0)


def test_the_two_setup_pipelines_give_identical_bits():
    a, b = readings("counts", 0, "f64"), readings("counts", 0, "f64", device_setup=0)
    for key in a:
        assert np.array_equal(a[key], b[key]), key


# ---- the update --------------------------------------------------------------------------------------------------------------------------
def updated(setting, with_push_pop=False):
    def make():
        U = tr.sub("update")
        h = solver("update", 0, setting)
        h.build_structure()
        before = h.state()
        if with_push_pop:
            h.push()
        write_device(h, "xp", U["xp"])
        write_device(h, "xl", U["xl"])
        h.update()
        out = {"state": h.state(), "F": h.compute_errors(), "before": before}
        if with_push_pop:
            h.pop()
            out["popped"] = h.state()
        h.close()
        return out
    return cached(("update", setting, with_push_pop), make)


@pytest.mark.parametrize("setting", SETTINGS)
def test_update_against_the_reference(setting):
    U = tr.sub("update")
    prec = LIBRARY[setting]
    q, t, X = updated(setting)["state"]
    Pf = int(U["sizes"][0])
    theta = np.linalg.norm(U["xp"][:, :3], axis=1)
    band = tr.band_of(theta)
    err = tr.update_errors(q[:Pf], t[:Pf])
    failures = []
    for b, name in enumerate(tr.BANDS):
        print("update %s: theta in %s worst %.2e, bound %.1e" % (setting, name, err[band == b].max(), tr.update_bound(b, prec)))
    for p in range(Pf):
        if not err[p] <= tr.update_bound(int(band[p]), prec):
            failures.append("case %d (theta %.3g): %.2e, bound %.1e" % (p, theta[p], err[p], tr.update_bound(int(band[p]), prec)))
    eps = tr.EPS32 if prec == "f32" else tr.EPS
    assert np.all(q[:, 3] >= 0) and np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 4 * eps
    assert np.array_equal(q[Pf:], U["q"][Pf:].astype(np.float32 if prec == "f32" else np.float64)) and np.array_equal(t[Pf:], U["t"][Pf:].astype(np.float32 if prec == "f32" else np.float64))
    lerr = tr.landmark_errors(X)
    print("update %s: landmarks worst %.2e, bound %.1e" % (setting, lerr.max(), tr.update_bound("landmark", prec)))
    assert lerr.max() <= tr.update_bound("landmark", prec)
    ferr = abs(updated(setting)["F"] - U["F_new"][0]) / U["F_new"][0]
    print("update %s: objective at the updated estimate off by %.2e, bound %.1e" % (setting, ferr, tr.update_bound("objective", prec)))
    assert ferr <= tr.update_bound("objective", prec)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("setting", SETTINGS)
def test_push_update_pop_returns_the_state_bit_for_bit(setting):
    a, b = updated(setting), updated(setting, with_push_pop=True)
    for x, y in zip(a["state"], b["state"]):
        assert np.array_equal(x, y)
    assert a["F"] == b["F"]
    for x, y in zip(b["before"], b["popped"]):
        assert np.array_equal(x, y)
    assert not np.array_equal(b["before"][1], b["state"][1])

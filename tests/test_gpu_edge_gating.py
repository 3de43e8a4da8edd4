"""Edge gating on the device (cuba_hip_gate_edges, cuba_hip_set_edge_active, cuba_hip_get_edge_active, cuba_hip_landmark_active_edges)
against tests/edge_gate_reference.py and the zero-information oracle: an OracleSolver on the graph with the gated edges' information set
to 0, which tests/test_edge_gate_reference.py holds to an OracleSolver on the graph without those edges.

Tolerances are the files' they come from: ASM_TOL / CHI2_TOL and compare_lm's bounds (tests/test_gpu_parity.py), BAR (tests/
test_gpu_covariance.py).  Masks and counts are compared exactly: the tests assert on the reference alone that no edge lies within 1e-6
(relative) of its threshold, four orders of magnitude above fp64 rounding of a chi2.  The fp32 library's decisions are compared outside
a band around the threshold of 4 x the largest relative difference, over all edges, between its existing chi_squares() and the oracle's
at the same estimate (the factor 4 covers the gate evaluating at a slightly different estimate); measured: a band of 1.3e-3 at the start
and 8.7e-3 after five iterations -- set by edges of chi2 0.02 and 0.002, whose residuals have lost digits to the subtraction; at or above
half a threshold the largest difference is 1.1e-4 / 1.5e-4 --, which leaves out 4 / 5 of the 2400 edges (cap: 1 %)."""
import copy
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import edge_gate_reference as R  # noqa: E402
from test_gpu_covariance import BAR  # noqa: E402
from test_gpu_parity import ASM_TOL, CHI2_TOL, graph_with_big_landmarks, rel, sym6  # noqa: E402

from conftest import RK_HUBER, RK_NONE, with_fixed  # noqa: E402
from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from oracle.oracle import OracleSolver  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTERS = ("structure_builds", "graph_uploads", "value_bytes_uploaded")


def counts_of(out):
    return {k: out[k] for k in R.COUNT_NAMES}


def check_gate(h, fp, prev=None, with_chi2=True, **kw):
    """gate_edges on h against the reference at h's estimate: mask, six counts, per-landmark counts, chi2.  Returns the reference."""
    ref = R.classify(fp, h.state(), prev=prev, **kw)
    assert R.threshold_margin(fp, ref["chi2"], kw.get("chi2_max", (R.CHI2_MONO, R.CHI2_STEREO))).min() > 1e-6        # (the condition of an exact comparison)
    got = h.gate_edges(with_chi2=with_chi2, **kw)
    assert counts_of(got) == ref["counts"], (counts_of(got), ref["counts"])
    assert np.array_equal(h.edge_active(), ref["mask"])
    assert np.array_equal(h.landmark_active_edges(), ref["per_landmark"])
    if with_chi2:
        ok = np.isfinite(ref["chi2"])
        assert np.all(np.abs(got["chi2"][ok] - ref["chi2"][ok]) <= ASM_TOL * np.maximum(ref["chi2"][ok], 1.0))
        assert not np.isfinite(got["chi2"][~ok]).any()
    return ref


def gated_oracle(fp, mask, state, rk, omega_scale=1.0):
    return OracleSolver(R.with_state(R.zero_information(fp, mask, omega_scale), state), rk)


def compare_gated_lm(h, fp, mask, rk, iters):
    """compare_lm of tests/test_gpu_parity.py from h's estimate, the zero-information oracle in the oracle's place"""
    ref = gated_oracle(fp, mask, h.state(), rk)
    r, g = ref.optimize(iters), h.optimize(iters)
    assert len(g["chi2"]) == len(r["chi2"])
    assert rel(g["chi2"], r["chi2"]) < CHI2_TOL and np.all(np.abs(g["chi2"] - r["chi2"]) <= CHI2_TOL * r["chi2"])
    for a, b, lim in zip(h.state(), ref.state(), (1e-8, 1e-6, 1e-6)):
        assert np.sqrt(((a - b) ** 2).sum(1).mean()) <= lim if len(a) else True
        assert np.abs(a - b).max() < 1e-5
    assert h.pcg_history()[1] == 0
    return r, g


@pytest.fixture(scope="module")
def keep_two_mask(small_fp):
    return R.mask_keeping_two_per_landmark(small_fp, np.random.default_rng(7))


# ---- 1. mask and counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(mixed_precision=1), dict(landmark_reorder=0, pose_reorder=0), dict(device_setup=0)],
                         ids=["default", "mixed_precision", "caller_order", "host_setup"])
def test_mask_counts_and_chi2(small_fp, opts):
    h = HipSolver(small_fp, RK_HUBER, **opts)
    start = check_gate(h, small_fp)
    assert (~start["mask"]).sum() == 2034
    h.set_edge_active(None)
    h.optimize(5)
    after = check_gate(h, small_fp)
    assert (~after["mask"]).sum() == 127 and (after["per_landmark"] == 0).sum() == 6
    assert np.array_equal(h.chi_squares() == 0, ~after["mask"])      # cuba_hip_chi_squares: 0 for a gated edge
    assert rel(h.chi_squares()[after["mask"]], after["chi2"][after["mask"]]) < ASM_TOL


def test_mask_and_counts_fp32_library(small_fp):
    fp = small_fp
    h = HipSolver(fp, RK_HUBER, precision="f32")
    for stage in ("start", "after 5 iterations"):
        ref = R.classify(fp, h.state())
        band = 4 * float((np.abs(h.chi_squares() - ref["chi2"]) / ref["chi2"]).max())
        sure = R.threshold_margin(fp, ref["chi2"]) > band
        print(f"\n[gate fp32] {stage}: band {band:.2e}, edges inside it {(~sure).sum()} of {fp.E}")
        assert (~sure).sum() <= fp.E // 100
        got = h.gate_edges(with_chi2=True)
        mask = h.edge_active()
        assert np.array_equal(mask[sure], ref["mask"][sure])
        # the counts: the reference's up to the edges inside the band
        for k in R.COUNT_NAMES:
            assert abs(got[k] - ref["counts"][k]) <= (~sure).sum(), (k, got[k], ref["counts"][k])
        assert sum(got[k] for k in R.COUNT_NAMES[:5]) == fp.E
        assert np.array_equal(h.landmark_active_edges(), R.landmark_counts(fp, mask))
        assert np.all(np.abs(got["chi2"] - ref["chi2"]) <= band * ref["chi2"])
        h.set_edge_active(None)
        h.optimize(5)


# ---- 2. depth ------------------------------------------------------------------------------------------------------------------------
def behind_cameras(fp):
    """a state with eight landmarks 1 m behind the first pose that sees them and two more in front of one of their poses and behind another"""
    from scipy.spatial.transform import Rotation
    Rm = Rotation.from_quat(fp.q).as_matrix()
    X = fp.Xw.copy()
    first = {}
    for e in range(fp.E):
        first.setdefault(int(fp.eL[e]), int(fp.eP[e]))
    moved = list(range(3, 83, 10))
    for l in moved:
        p = first[l]
        X[l] = Rm[p].T @ (np.array([0.0, 0.0, -1.0]) - fp.t[p])
    split = []
    for l in range(100, fp.Lt):
        ps = fp.eP[fp.eL == l]
        for a in ps:
            cand = Rm[a].T @ (np.array([0.0, 0.0, 0.5]) - fp.t[a])          # half a metre in front of pose a
            z = np.array([(Rm[b] @ cand + fp.t[b])[2] for b in ps])
            if (z > 0).any() and (z < 0).any():
                X[l] = cand; split.append(l)
                break
        if len(split) == 2:
            break
    assert len(split) == 2
    return (fp.q, fp.t, X), moved, split


def test_depth(small_fp):
    fp = small_fp
    assert R.classify(fp)["depth"].min() > 4.0
    state, moved, split = behind_cameras(fp)
    h = HipSolver(fp, RK_HUBER)
    h.set_state(*state)
    inf = (np.inf, np.inf)
    ref = check_gate(h, fp, chi2_max=inf)
    behind = ~ref["depth_ok"]
    assert ref["counts"]["gated_depth"] == behind.sum() >= 10 and np.array_equal(~ref["mask"], behind)
    assert all(behind[np.flatnonzero(fp.eL == l)[0]] for l in moved)                 # behind the first pose that sees them
    assert all(behind[fp.eL == l].any() and not behind[fp.eL == l].all() for l in split)
    both = check_gate(h, fp, prev=ref["mask"])                          # with the chi2 test: a depth failure still counts as one
    assert both["counts"]["gated_depth"] == behind.sum()
    none = check_gate(h, fp, prev=both["mask"], chi2_max=inf, positive_depth=False)
    assert none["counts"]["gated_depth"] == 0 and none["mask"].all()
    # a NaN coordinate gates every edge of its landmark, with and without the depth test
    X = state[2].copy(); X[200, 1] = np.nan
    h.set_state(state[0], state[1], X)
    prev = none["mask"]
    for positive_depth in (True, False):
        ref = check_gate(h, fp, prev=prev, chi2_max=inf, positive_depth=positive_depth)
        prev = ref["mask"]
        assert not ref["mask"][fp.eL == 200].any() and (fp.eL == 200).sum() >= 2
        assert ref["counts"]["gated_depth" if positive_depth else "gated_chi2_stereo"] >= 1


# ---- 3. modes --------------------------------------------------------------------------------------------------------------------------
def test_dry_run_changes_nothing(small_fp, keep_two_mask):
    h = HipSolver(small_fp, RK_HUBER)
    c0 = h.compute_errors()
    ref = R.classify(small_fp, mode="dry_run")
    got = h.gate_edges(mode="dry_run", with_chi2=True)
    assert counts_of(got) == ref["counts"] and got["changed"] == 2034 and rel(got["chi2"], ref["chi2"]) < ASM_TOL
    assert h.compute_errors() == c0 and h.edge_active().all()
    h.set_edge_active(keep_two_mask)
    c1 = h.compute_errors()
    assert c1 < c0
    ref = R.classify(small_fp, mode="dry_run", prev=keep_two_mask)
    assert counts_of(h.gate_edges(mode="dry_run")) == ref["counts"]
    assert h.compute_errors() == c1 and np.array_equal(h.edge_active(), keep_two_mask)


def test_only_remove_never_readmits(small_fp):
    fp = small_fp
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    judged = R.classify(fp, h.state())["mask"]
    prev = np.ones(fp.E, bool); prev[np.flatnonzero(judged)[:20]] = False           # 20 inliers switched off by hand
    h.set_edge_active(prev)
    ref = check_gate(h, fp, prev=prev, mode="only_remove")
    assert not ref["mask"][~prev].any() and np.array_equal(ref["mask"], judged & prev) and ref["counts"]["changed"] == 127
    assert sum(ref["counts"][k] for k in R.COUNT_NAMES[:5]) == fp.E - 20
    again = check_gate(h, fp, prev=ref["mask"], mode="reclassify")                  # judged afresh: the 20 come back
    assert np.array_equal(again["mask"], judged) and again["counts"]["changed"] == 20


def test_reclassify_after_the_flow(small_fp):
    fp = small_fp
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    m5 = check_gate(h, fp)["mask"]
    h.optimize(10)
    c15 = check_gate(h, fp, prev=m5)
    assert (c15["mask"] & ~m5).sum() == 5 and (~c15["mask"] & m5).sum() == 3 and c15["counts"]["changed"] == 8


# ---- 4. round trip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(landmark_reorder=1, pose_reorder=1)], ids=["default", "reorder_on"])
def test_set_and_get_round_trip(small_fp, opts):
    fp = small_fp
    rng = np.random.default_rng(11)
    h = HipSolver(fp, RK_HUBER, **opts)
    for _ in range(2):
        mask = rng.random(fp.E) < 0.7
        h.set_edge_active(mask)
        assert np.array_equal(h.edge_active(), mask)
        assert np.array_equal(h.landmark_active_edges(), R.landmark_counts(fp, mask))
        assert np.array_equal(h.chi_squares() != 0, mask)


def test_round_trip_under_an_internal_pose_order():
    """shuffled pose ids: the library renumbers the poses internally and sorts the edges again after the first structure build"""
    from test_gpu_configs import shuffled_pose_ids
    from cuba_amd.synth import synth_ba
    fp = flatten(shuffled_pose_ids(synth_ba(96, 1200, 4800, seed=5), seed=3))
    rng = np.random.default_rng(12)
    mask = rng.random(fp.E) < 0.7
    h = HipSolver(fp, RK_HUBER)
    h.set_edge_active(mask)
    assert not np.array_equal(h.pcg_config()["pose_order"], np.arange(fp.Pf))        # (the internal order is in force)
    assert np.array_equal(h.edge_active(), mask) and np.array_equal(h.landmark_active_edges(), R.landmark_counts(fp, mask))
    assert h.compute_errors() == pytest.approx(gated_oracle(fp, mask, h.state(), RK_HUBER).compute_errors(), rel=1e-11)
    check_gate(h, fp, prev=mask)
    # ... and a gate set BEFORE the order changes (pose_reorder switched on afterwards: the next structure build sorts again)
    h2 = HipSolver(fp, RK_HUBER, pose_reorder=0)
    h2.set_edge_active(mask)
    c = h2.compute_errors()
    h2.set_option("pose_reorder", 1)
    assert h2.compute_errors() == pytest.approx(c, rel=1e-12) and np.array_equal(h2.chi_squares() != 0, mask)
    assert not np.array_equal(h2.pcg_config()["pose_order"], np.arange(fp.Pf))


def test_clearing_the_gate_gives_a_fresh_handles_bits(small_fp, keep_two_mask):
    fp = small_fp
    fresh = HipSolver(fp, RK_HUBER, heuristics=0)
    want = fresh.optimize(10)["chi2"]
    h = HipSolver(fp, RK_HUBER, heuristics=0)
    c0 = h.compute_errors()
    h.set_edge_active(keep_two_mask)
    assert h.compute_errors() < c0
    h.set_edge_active(None)
    assert h.edge_active().all()
    assert np.array_equal(h.optimize(10)["chi2"], want) and all(np.array_equal(a, b) for a, b in zip(h.state(), fresh.state()))
    ones = HipSolver(fp, RK_HUBER, heuristics=0)
    ones.set_edge_active(np.ones(fp.E, bool))
    assert np.array_equal(ones.optimize(10)["chi2"], want) and all(np.array_equal(a, b) for a, b in zip(ones.state(), fresh.state()))


# ---- 5. LM parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["huber", "none", "fixed", "reduced_solver", "fp32"])
def test_lm_parity_after_a_gate(small_fp, small_graph, case):
    fp, rk, opts = small_fp, RK_HUBER, {}
    if case == "none":
        rk = RK_NONE
    if case == "fixed":
        fp = flatten(with_fixed(small_graph, fixed_pose_rows=[3, 4, 5, 20], fixed_lm_rows=list(range(0, 300, 7))))
    if case == "reduced_solver":
        opts = dict(reduced_solver=1)
    if case == "fp32":
        # the fp32 library against the fp64 oracle ON ITS OWN MASK, at the tolerance of tests/test_gpu_parity.py::test_float32_build_variant
        h = HipSolver(fp, rk, precision="f32")
        h.optimize(5); h.gate_edges()
        mask = h.edge_active()
        r = gated_oracle(fp, mask, h.state(), rk).optimize(10)["chi2"]
        g = h.optimize(10)["chi2"]
        assert len(g) == len(r) and np.all(np.abs(g - r) <= 1e-4 * r)
        return
    h = HipSolver(fp, rk, **opts)
    h.optimize(5)
    ref = check_gate(h, fp, with_chi2=False)
    if case == "huber":
        assert (ref["per_landmark"] == 0).sum() == 6                # landmarks left without any active edge take part
    r, _ = compare_gated_lm(h, fp, ref["mask"], rk, 10)
    if case == "huber":
        assert r["chi2"][0] == pytest.approx(4185.5, abs=0.05) and r["chi2"][-1] == pytest.approx(3884.7, abs=0.05)
    if case == "fixed":
        q, t, X = h.state()
        assert np.array_equal(q[fp.Pf:], fp.q[fp.Pf:]) and np.array_equal(X[fp.Lf:], fp.Xw[fp.Lf:])


def test_lm_parity_with_half_of_a_big_landmark_gated():
    g, n_big = graph_with_big_landmarks()
    fp = flatten(g)
    per_lm = np.bincount(fp.eL, minlength=fp.Lt)
    big = np.flatnonzero(per_lm > 64)
    assert len(big) == n_big
    mask = np.ones(fp.E, bool)
    mask[np.flatnonzero(fp.eL == big[0])[::2]] = False                      # every second edge of one of them
    mask[np.flatnonzero(fp.eL == big[1])[:70]] = False                      # and the first 70 of another: more than a wave's worth
    h = HipSolver(fp, RK_HUBER)
    h.set_edge_active(mask)
    counts = h.landmark_active_edges()
    assert np.array_equal(counts, R.landmark_counts(fp, mask)) and counts[big[0]] == per_lm[big[0]] // 2 > 32
    compare_gated_lm(h, fp, mask, RK_HUBER, 5)
    ref = check_gate(h, fp, prev=mask, with_chi2=False)                     # the workgroup form under a classified mask
    assert (ref["per_landmark"][big] > 64).any()


# ---- 6. stage parity on a gated handle (tests/test_gpu_parity.py::test_stage_parity_small with the zero-information oracle) ----------
def test_stage_parity_on_a_gated_handle(small_fp, keep_two_mask):
    fp, mask = small_fp, keep_two_mask
    o, h = OracleSolver(R.zero_information(fp, mask), RK_HUBER), HipSolver(fp, RK_HUBER, pcg_tol=1e-11)
    h.set_edge_active(mask)
    assert h.compute_errors() == pytest.approx(o.compute_errors(), rel=1e-12)
    o.build_system(); h.build_system()
    md = o.max_diagonal()
    assert h.max_diagonal() == pytest.approx(md, rel=1e-12)
    lm = h.array("lm_sys").reshape(-1, 9)
    assert rel(sym6(lm[:, :6]), o.array("Hll").reshape(-1, 3, 3)) < ASM_TOL
    assert rel(lm[:, 6:], o.array("bl").reshape(-1, 3)) < ASM_TOL
    assert rel(h.array("bp"), o.array("bp")) < ASM_TOL
    lam = 1e-5 * md
    o.set_lambda(lam); h.set_lambda(lam)
    o.schur(); h.schur()
    rpo, cio, vo = o.hsc()
    rp, ci, v = h.hsc()
    assert np.array_equal(rp, rpo) and np.array_equal(ci, cio)
    iu = np.triu_indices(6)
    diag = np.zeros(len(ci), bool); diag[rp[:-1]] = True
    assert rel(v[~diag], vo[~diag]) < ASM_TOL
    vd = v[diag][:, iu[0], iu[1]] + lam * (iu[0] == iu[1])
    assert rel(vd, vo[diag][:, iu[0], iu[1]]) < ASM_TOL
    assert rel(h.array("bsc"), o.array("bsc")) < ASM_TOL
    assert o.solve() and h.solve_reduced()
    h.back_substitute()
    assert rel(h.array("xp"), o.array("xp")) < 1e-6 and rel(h.array("xl"), o.array("xl")) < 1e-6
    assert h.compute_scale(lam) == pytest.approx(o.compute_scale(lam), rel=1e-8)
    o.update(); h.update()
    assert h.compute_errors() == pytest.approx(o.compute_errors(), rel=1e-9)
    assert rel(h.chi_squares(), o.chi_squares()) < 1e-9


# ---- 7. persistence --------------------------------------------------------------------------------------------------------------------
def test_the_mask_outlives_an_upload_of_the_same_edges(small_fp, keep_two_mask):
    fp, mask = small_fp, keep_two_mask
    h = HipSolver(fp, RK_HUBER)
    h.set_edge_active(mask)
    fp2 = copy.copy(fp); fp2.omega = 2.0 * fp.omega
    h.set_graph(fp2)                                     # same edges, found by the library's own comparison; doubled information
    assert np.array_equal(h.edge_active(), mask)
    want = gated_oracle(fp, mask, (fp.q, fp.t, fp.Xw), RK_HUBER, omega_scale=2.0).compute_errors()
    assert h.compute_errors() == pytest.approx(want, rel=1e-11)
    assert np.array_equal(h.chi_squares() != 0, mask)
    h.set_graph(fp2, two_step=True)                      # the two-step upload: the values arrive after the structure analysis
    assert np.array_equal(h.edge_active(), mask) and h.compute_errors() == pytest.approx(want, rel=1e-11)
    h.hint_unchanged(True, False); h.set_graph(fp)       # promised edges, new values
    assert np.array_equal(h.edge_active(), mask)
    assert h.compute_errors() == pytest.approx(gated_oracle(fp, mask, (fp.q, fp.t, fp.Xw), RK_HUBER).compute_errors(), rel=1e-11)
    gated = h.chi_squares()
    h.hint_unchanged(True, True); h.set_graph(fp)        # promised edges and values: the mask is kept, the chi2 is the gated set's
    assert np.array_equal(h.edge_active(), mask) and np.array_equal(h.chi_squares(), gated)
    # gate -> clear -> "same values": the uploaded information, bit for bit, no zero left behind
    h.set_edge_active(None)
    h.hint_unchanged(True, True); h.set_graph(fp)
    fresh = HipSolver(fp, RK_HUBER).chi_squares()
    assert np.array_equal(h.chi_squares(), fresh) and (fresh > 0).all() and h.edge_active().all()
    # ... and with the gate still on while the promise is made: clearing it afterwards finds the uploaded information too
    h.set_edge_active(mask)
    h.hint_unchanged(True, True); h.set_graph(fp)
    h.set_edge_active(None)
    assert np.array_equal(h.chi_squares(), fresh)


def test_other_edges_drop_the_mask(small_fp, keep_two_mask):
    fp = small_fp
    h = HipSolver(fp, RK_HUBER)
    h.set_edge_active(keep_two_mask)
    less = copy.copy(fp)
    less.eP, less.eL, less.eDim, less.meas, less.omega, less.edge_src = (a[:-1].copy() for a in (fp.eP, fp.eL, fp.eDim, fp.meas, fp.omega, fp.edge_src))
    h.set_graph(less)
    assert h.edge_active().shape == (fp.E - 1,) and h.edge_active().all()
    assert np.array_equal(h.chi_squares(), HipSolver(less, RK_HUBER).chi_squares())
    # the same number of edges, one of them on another landmark
    h.set_graph(fp); h.set_edge_active(keep_two_mask)
    other = copy.copy(fp); other.eL = fp.eL.copy()
    e = int(np.flatnonzero(np.bincount(fp.eL, minlength=fp.Lt)[fp.eL] > 2)[0])
    other.eL[e] = (fp.eL[e] + 1) % fp.Lf
    h.set_graph(other)
    assert h.edge_active().all()


def test_gating_touches_no_counter_estimate_or_snapshot(small_fp):
    fp = small_fp
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    h.snapshot_state()
    before = {k: h.counter(k) for k in COUNTERS}
    s5 = h.state()
    h.gate_edges(mode="dry_run"); h.gate_edges(with_chi2=True); h.edge_active(); h.landmark_active_edges()
    assert all(np.array_equal(a, b) for a, b in zip(h.state(), s5))
    h.optimize(10)
    h.gate_edges(mode="only_remove"); h.set_edge_active(np.ones(fp.E, bool)); h.set_edge_active(None)
    assert {k: h.counter(k) for k in COUNTERS} == before
    h.restore_state()
    assert all(np.array_equal(a, b) for a, b in zip(h.state(), s5))


# ---- 8. batch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_batch_of_gated_and_ungated_handles_is_bit_identical_to_solo_runs(small_fp, keep_two_mask, precision):
    fp = small_fp
    masks = [keep_two_mask, R.mask_keeping_two_per_landmark(fp, np.random.default_rng(8), fraction=0.3), None]
    opts = dict(pcg_aggregate=8, precision=precision)            # the class "f32:<=768:cl2" / "f32lib:<=768:cl2" of tests/test_gpu_batch.py

    def make(mask):
        h = HipSolver(fp, RK_HUBER, **opts)
        if mask is not None:
            h.set_edge_active(mask)
        return h
    solo = []
    for m in masks:
        h = make(m)
        solo.append((h.optimize(8)["chi2"], h.state(), h.pcg_history()[0].copy()))
        h.close()
    assert not np.array_equal(solo[0][0], solo[1][0]) and not np.array_equal(solo[0][0], solo[2][0])
    hs = [make(m) for m in masks]
    chi2, batched = optimize_batch(hs, 8)
    assert batched > 0 and hs[0].counter("batch_full_trials") > 0
    for h, m, got, (want, state, hist) in zip(hs, masks, chi2, solo):
        assert np.array_equal(got, want) and all(np.array_equal(a, b) for a, b in zip(h.state(), state))
        assert np.array_equal(h.pcg_history()[0], hist)
        assert np.array_equal(h.edge_active(), np.ones(fp.E, bool) if m is None else m)


# ---- 9. covariance ---------------------------------------------------------------------------------------------------------------------
def test_covariance_sees_the_active_edges_only(small_fp, keep_two_mask):
    fp, mask = small_fp, keep_two_mask
    h = HipSolver(fp, RK_HUBER)
    h.set_edge_active(mask)
    h.optimize(10)
    cut = HipSolver(R.without_edges(fp, mask), RK_HUBER)
    cut.set_state(*h.state())
    a, b = h.covariance(landmarks=True), cut.covariance(landmarks=True)
    assert not a["not_positive_definite"] and not b["not_positive_definite"]
    for key in ("pose", "landmark"):
        err = max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(a[key], b[key]) if np.abs(y).max() > 0)
        print(f"\n[gate covariance] {key}: {err:.2e}")
        assert err <= BAR
    full = HipSolver(fp, RK_HUBER); full.set_state(*h.state())
    assert rel(full.covariance()["pose"], b["pose"]) > 1e-3                 # (the gated edges do matter)
    pairs = [("pose", 1, "pose", 7), ("pose", 2, "landmark", int(fp.eL[np.flatnonzero((fp.eP == 2) & mask)[0]]))]
    (pa, bad_a), (pb, bad_b) = h.covariance_pairs(pairs), cut.covariance_pairs(pairs)
    assert not bad_a and not bad_b and all(rel(x, y) <= BAR for x, y in zip(pa, pb))


# ---- 10. errors ------------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(CubaHipError) as e:
        call()
    return int(re.match(r"status (\d+)", str(e.value)).group(1))


def test_errors(small_fp):
    fp = small_fp
    STATE, ARG = 3, 1
    empty = HipSolver(None, RK_HUBER)
    for call in (empty.gate_edges, lambda: empty.set_edge_active(None), empty.edge_active, empty.landmark_active_edges):
        assert status_of(call) == STATE
    h = HipSolver(fp, RK_HUBER)
    assert status_of(lambda: h.gate_edges(mode=3)) == ARG and status_of(lambda: h.gate_edges(mode=-1)) == ARG
    assert status_of(lambda: h.gate_edges(chi2_max=(np.nan, 7.815))) == ARG and status_of(lambda: h.gate_edges(chi2_max=(5.991, np.nan))) == ARG
    assert h.edge_active().all()                                            # (a refused call leaves no gate behind)
    assert h.gate_edges(chi2_max=(np.inf, np.inf), positive_depth=False)["changed"] == 0
    for part in (lambda s: s.set_partition(0, fp.Lt // 2), lambda s: s.set_graph(fp, landmark_range=(0, fp.Lt // 2))):
        p = HipSolver(fp, RK_HUBER)
        part(p)
        for call in (p.gate_edges, lambda: p.set_edge_active(np.ones(fp.E, bool)), lambda: p.set_edge_active(None), p.edge_active, p.landmark_active_edges):
            assert status_of(call) == STATE
    g = HipSolver(fp, RK_HUBER)
    g.gate_edges()
    assert status_of(lambda: g.set_partition(0, fp.Lt // 2)) == STATE       # a gated handle cannot be partitioned ...
    g.set_edge_active(None)
    g.set_partition(0, fp.Lt // 2)                                          # ... an ungated one can

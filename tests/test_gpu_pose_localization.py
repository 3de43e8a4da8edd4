"""Pose localisation from scratch on the device (cuba_hip_localize_poses) against tests/pose_localization_reference.py.

Inputs (pose_localization_reference.gpu_input): "small", the suite's small graph behind true_fp of the refinement tests (39 free poses of
14 ... 115 edges, mono and stereo mixed, one fixed pose), and "wide", wide_problem with 129 ... 300 edges per pose -- the 256-thread
batches and poses of more than 256 edges are both met --, its poses 0 and 1 made mono-only.  Measurements carry 0.5 px of noise and one
edge in five is a gross outlier of 50 - 200 px.  Every selected pose's value is NaN before a call.  Beside them a tiny hand-made graph of
poses with exactly 3, 4 and 5 usable edges, a pose on collinear landmarks and a pose all of whose edges are gated.

Condition, not measurement: statuses, counts, winner, inliers and edge_inlier are compared EXACTLY.  The seeds were chosen, when these tests
were written, so that FOR THE REFERENCE ALONE every pose with a winner has (a) a relative gap between its best two scores > 1e-6 and (b) no
usable edge within 1e-6 (relative) of its chi2 threshold or of depth 0 at the winner, as the 60-digit twin sees it;
tests/test_pose_localization_reference.py asserts that on the CPU for exactly these inputs, and check() asserts it again here: no pose is
left out at run time.  Seeds tried: "small" 1 ... 9 -- 1 ... 8 each leave a pose whose best sample is drawn a second time in another
order at 256 or 1024 hypotheses (the same pose to rounding, a gap of 1e-12 or none) --, taken: 9 (smallest margins 5.7e-5 / 3.3e-4);
"wide" 1 (two all-outlier candidates of equal score at 1 hypothesis), 2, taken: 2 (5.0e-3 / 1.3e-2).

Poses, fp64 library: pose_distance(device, reference) <= 8 D per pose, D = the reference's own distance from its 60-digit twin for that
pose (the same formulas, so D measures the conditioning of that pose's winning sample); 8 for the device's own cube root, cosine, arc
cosine and division (csrc/ba_localize.hip switches the contraction into fused multiply-adds off, so the rest is the reference's arithmetic).  fp32 library: the
reference is fed the float-rounded landmarks, cameras, measurements and information and rounds its pose to float; the bound is
max(8 D, 2 * 2^-24), one float rounding of the stored result (the floor of check_poses in test_gpu_pose_refinement.py).  cost: rtol 1e-9.

The basin test runs localize_poses(256) -> refine_poses(4, 10, 2) from NaN poses against refine_poses(4, 10, 2) from the true poses.  The
same pipeline in the two numpy references on the CPU ends, for the poses 0 ... 5 of "small", 9.2e-11, 1.6e-12, 3.7e-17, 7.1e-16, 1.5e-17
and 4.8e-15 apart (statuses and inlier masks equal).  As in the long runs of test_gpu_pose_refinement.py that distance is no smooth number
pose by pose: the last trials of a converged round change F by 1e-20 of itself, so whether they are taken is rounding noise, and two
starts end one such step apart or not (9.2e-11 for pose 0, 3.7e-17 for pose 2, which says nothing about where another summation order
ends pose 2).  So the device's two runs must agree, for every pose, within 100 x the LARGEST of the references' distances (9.2e-9), floor
1e-12.  Measured on the MI355X: 5.0e-10, 1.6e-12, 9.5e-11, 9.4e-16, 1.4e-14, 3.7e-16."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import pose_localization_reference as L  # noqa: E402
import pose_refinement_reference as PR  # noqa: E402

from conftest import RK_HUBER  # noqa: E402
from cuba_amd.capi import POSELOC_STATUS_NAMES, CubaHipError, HipSolver  # noqa: E402

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -24
EXACT = ("status", "winner", "inliers", "edge_inlier")


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def lost_handle(fp, select=None, **opts):
    """a handle on fp whose selected poses hold NaN"""
    h = HipSolver(fp, RK_HUBER, **opts)
    q, t = L.nan_poses(fp, select)
    h.set_state(q, t, fp.Xw)
    return h


def check(got, case, what, f32=False):
    """statuses, counts, winner, inliers and edge_inlier exactly (under the margin condition, asserted here), cost to 1e-9, every OK pose
    within max(8 D, floor) of the reference's"""
    fp, ref, margins, D = case
    a, b = min((m[0] for m in margins.values()), default=np.inf), min((m[1] for m in margins.values()), default=np.inf)
    print(f"\n[pose localisation] {what}: margins (a) {a:.2e} (b) {b:.2e}, counts {ref['counts']}")
    assert a > L.MARGIN and b > L.MARGIN, margins
    for k in EXACT:
        assert np.array_equal(got[k], ref[k]), (k, np.flatnonzero(got[k] != ref[k]))
    assert [got[k] for k in POSELOC_STATUS_NAMES] == [ref["counts"][k] for k in POSELOC_STATUS_NAMES] and sum(ref["counts"].values()) == fp.Pt
    assert np.allclose(got["cost"], ref["cost"], rtol=1e-9, atol=0)
    ok = np.flatnonzero(ref["status"] == L.OK)
    dist = {p: PR.pose_distance(got["q"][p], got["t"][p], ref["q"][p], ref["t"][p]) for p in ok}
    bound = {p: max(8 * D[p], 2 * F32_EPS if f32 else 0.0) for p in ok}
    worst = max(ok, key=lambda p: dist[p] / max(bound[p], 1e-300)) if len(ok) else None
    if worst is not None:
        print(f"[pose localisation] {what}: largest pose distance device - reference {max(dist.values()):.2e}, D {min(D.values()):.2e} ... {max(D.values()):.2e}; "
              f"closest to its bound: pose {worst}, {dist[worst]:.2e} against {bound[worst]:.2e}")
        ratio = np.array([dist[p] / max(D[p], 1e-300) for p in ok])
        print(f"[pose localisation] {what}: device distance / D over {len(ok)} poses: median {np.median(ratio):.2f}, largest {ratio.max():.2f}")
    assert all(dist[p] <= bound[p] for p in ok), {p: (dist[p], bound[p]) for p in ok if dist[p] > bound[p]}
    rest = ref["status"] != L.OK                  # (the unchanged pose of every other: NaN for a lost one)
    q0, t0 = L.nan_poses(PR.float_rounded(fp)[0] if f32 else fp)
    assert np.array_equal(got["q"][rest], q0[rest], equal_nan=True) and np.array_equal(got["t"][rest], t0[rest], equal_nan=True)
    return dist


# ---- 1, 2. against the reference, over the hypothesis counts -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("hypotheses", L.HYPOTHESES)
def test_against_the_reference(name, hypotheses):
    case = L.gpu_case(name, hypotheses)
    fp, ref = case[0], case[1]
    h = lost_handle(fp)
    got = h.localize_poses(hypotheses=hypotheses, seed=L.SEED[name])
    check(got, case, f"{name}, {hypotheses} hypotheses")
    q, t, X = h.state()
    ok = ref["status"] == L.OK
    assert bits_equal(q[ok], got["q"][ok]) and bits_equal(t[ok], got["t"][ok]) and bits_equal(X, fp.Xw)
    free_rest = ~ok & (np.arange(fp.Pt) < fp.Pf)
    assert np.isnan(q[free_rest]).all() and np.isnan(got["q"][free_rest]).all()          # a pose that is not OK keeps its value, NaN or not
    if name == "wide":
        n, ns = np.bincount(fp.eP, minlength=fp.Pt), np.bincount(fp.eP[np.asarray(fp.eDim) == 3], minlength=fp.Pt)
        assert list(n) == [129, 150, 200, 257, 300] and ns[0] == ns[1] == 0 and (ns[2:] > 0).all() and (ns[2:] < n[2:]).all()


# ---- 3. the same result over the options -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_same_result_over_the_options(name):
    case = L.gpu_case(name, 256)
    fp = case[0]
    runs = []
    for opts in (dict(), dict(landmark_reorder=0, pose_reorder=0), dict(device_setup=0)):
        h = lost_handle(fp, **opts)
        runs.append(h.localize_poses(hypotheses=256, seed=L.SEED[name]))
        runs[-1]["state"] = h.state()
    check(runs[0], case, f"{name}, default options")
    for other in runs[1:]:
        for k in EXACT:
            assert np.array_equal(other[k], runs[0][k]), k
        # the pose is a function of three points taken in key order, and the sample is defined in the caller's numbering: bit for bit
        assert bits_equal(other["q"], runs[0]["q"]) and bits_equal(other["t"], runs[0]["t"])
        assert all(bits_equal(x, y) for x, y in zip(other["state"], runs[0]["state"]))
        assert np.allclose(other["cost"], runs[0]["cost"], rtol=1e-9, atol=0)


# ---- 4. the basin ---------------------------------------------------------------------------------------------------------------------------
LONG = dict(rounds=4, iterations=10, robust_rounds=2, min_inliers=10)
BASIN_POSES = 6


def test_basin_localize_then_refine_reaches_what_refinement_from_the_true_poses_reaches():
    fp = L.gpu_input("small")
    select = np.arange(fp.Pt) < BASIN_POSES
    # the same pipeline in the numpy references: the distance between the two starts' results (the header gives the values)
    loc = L.localize(fp, select=select, hypotheses=256, seed=L.SEED["small"])
    ra = PR.refine(fp, state=(loc["q"], loc["t"], fp.Xw), select=select, rk=RK_HUBER, **LONG)
    rb = PR.refine(fp, state=(fp.q, fp.t, fp.Xw), select=select, rk=RK_HUBER, **LONG)
    assert np.array_equal(ra["status"], rb["status"]) and np.array_equal(ra["edge_inlier"], rb["edge_inlier"]) and ra["counts"]["ok"] == BASIN_POSES
    own = [PR.pose_distance(ra["q"][p], ra["t"][p], rb["q"][p], rb["t"][p]) for p in range(BASIN_POSES)]
    h = lost_handle(fp, select)
    assert h.localize_poses(select=select, hypotheses=256, seed=L.SEED["small"])["ok"] == BASIN_POSES
    a = h.refine_poses(select=select, **LONG)
    twin = HipSolver(fp, RK_HUBER)
    b = twin.refine_poses(select=select, **LONG)
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["status"], ra["status"]) and np.array_equal(a["edge_inlier"], b["edge_inlier"])
    dist = [PR.pose_distance(a["q"][p], a["t"][p], b["q"][p], b["t"][p]) for p in range(BASIN_POSES)]
    print("\n[pose localisation] basin: device, localised start - true start " + " ".join(f"{d:.2e}" for d in dist) + "; the references' " + " ".join(f"{d:.2e}" for d in own))
    bound = max(100 * max(own), 1e-12)
    assert all(d <= bound for d in dist), (dist, own)
    # refinement alone, from poses 40 degrees and half the scene depth off, does not get there: what localize_poses is for
    q, t = PR.perturbed_poses(fp, 31, rot_deg=40.0, trans=12.0)
    far = HipSolver(fp, RK_HUBER)
    far.set_state(q, t, fp.Xw)
    c = far.refine_poses(select=select, **LONG)
    lost = [p for p in range(BASIN_POSES) if c["status"][p] != PR.OK or PR.pose_distance(c["q"][p], c["t"][p], b["q"][p], b["t"][p]) > bound]
    print(f"[pose localisation] basin: refinement alone from 40 degrees / 12 m off misses the poses {lost}")
    assert len(lost) >= 1


# ---- 5. statuses ------------------------------------------------------------------------------------------------------------------------------
def test_statuses_on_the_tiny_graph():
    fp, idx, edges = L.tiny_problem()
    n = np.bincount(fp.eP, minlength=fp.Pt)
    assert [int(n[idx[k]]) for k in ("three", "four", "five")] == [3, 4, 5]
    mask = np.ones(fp.E, bool); mask[edges["gated"]] = False
    omega = np.where(mask, fp.omega, 0.0)
    select = np.ones(fp.Pt, bool); select[idx["four"]] = False
    h = lost_handle(fp)
    h.set_edge_active(mask)
    want = dict(three=L.FEW_OBSERVATIONS, four=L.NOT_SELECTED, five=L.OK, collinear=L.NO_SOLUTION, gated=L.FEW_OBSERVATIONS, fixed=L.FIXED)
    ref = L.localize(fp, hypotheses=8, seed=3, omega=omega, min_inliers=5, select=select)
    got = h.localize_poses(select=select, hypotheses=8, seed=3, min_inliers=5, dry_run=True)
    assert {k: int(got["status"][idx[k]]) for k in want} == want and np.array_equal(got["status"], ref["status"])
    assert np.array_equal(got["inliers"], ref["inliers"]) and np.array_equal(got["edge_inlier"], ref["edge_inlier"]) and not got["edge_inlier"][~mask].any()
    assert [got[k] for k in POSELOC_STATUS_NAMES] == [1, 1, 1, 2, 1, 0] and (got["winner"][got["status"] != L.OK] == -1).all()
    # FEW_INLIERS through min_inliers: five edges in, six asked for
    got = h.localize_poses(hypotheses=8, seed=3, min_inliers=6, dry_run=True)
    assert got["status"][idx["five"]] == L.FEW_INLIERS == got["status"][idx["four"]] and got["inliers"][idx["five"]] == 5 and got["winner"][idx["five"]] == -1
    assert got["cost"][idx["five"]] < 1e-12 and np.isnan(got["q"][idx["five"]]).all()
    # exact measurements: the winner is the true pose
    got = h.localize_poses(hypotheses=8, seed=3, min_inliers=0)
    for k in ("four", "five"):
        assert got["status"][idx[k]] == L.OK and PR.pose_distance(got["q"][idx[k]], got["t"][idx[k]], fp.q[idx[k]], fp.t[idx[k]]) < 1e-9
    assert np.array_equal(h.edge_active(), mask)


# ---- 6. seed matters and only seed ----------------------------------------------------------------------------------------------------------
def test_seed_and_subset():
    case = L.gpu_case("small", 256)
    fp = case[0]
    h = lost_handle(fp)
    full = h.localize_poses(hypotheses=256, seed=L.SEED["small"], dry_run=True)
    again = h.localize_poses(hypotheses=256, seed=L.SEED["small"], dry_run=True)
    for k in EXACT:
        assert np.array_equal(full[k], again[k])
    assert all(bits_equal(full[k], again[k]) for k in ("q", "t", "cost"))
    other_case = L.gpu_case("small", 256, seed=L.SEED["small"] + 100)
    other = h.localize_poses(hypotheses=256, seed=L.SEED["small"] + 100, dry_run=True)
    check(other, other_case, "small, another seed")
    assert (other["winner"] != full["winner"]).any()
    select = np.arange(fp.Pt) % 3 == 1
    part = h.localize_poses(select=select, hypotheses=256, seed=L.SEED["small"], dry_run=True)
    for k in ("status", "winner", "inliers"):
        assert np.array_equal(part[k][select], full[k][select])
    assert all(bits_equal(part[k][select], full[k][select]) for k in ("q", "t", "cost"))
    assert np.array_equal(part["edge_inlier"][select[fp.eP]], full["edge_inlier"][select[fp.eP]])
    assert (part["status"][~select] == L.NOT_SELECTED).all() and (part["inliers"][~select] == 0).all() and part["not_selected"] == (~select).sum()
    live = np.asarray(fp.omega) > 0
    assert np.array_equal(part["edge_inlier"][~select[fp.eP]], live[~select[fp.eP]])


# ---- 7. dry run, what stays, optimize afterwards ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_dry_run_changes_nothing(precision):
    fp = L.gpu_input("small")
    h = lost_handle(fp, precision=precision)
    before = h.state()
    dry = h.localize_poses(seed=L.SEED["small"], dry_run=True)
    assert all(bits_equal(a, b) for a, b in zip(h.state(), before))
    real = h.localize_poses(seed=L.SEED["small"])
    for k in EXACT:
        assert np.array_equal(dry[k], real[k])
    ok = real["status"] == L.OK
    assert all(bits_equal(dry[k][ok], real[k][ok]) for k in ("q", "t", "cost")) and dry["ok"] == real["ok"] == fp.Pf
    assert bits_equal(h.state()[0][ok], real["q"][ok]) and bits_equal(h.state()[1][ok], real["t"][ok]) and not np.isnan(h.state()[0]).any()


def test_what_stays():
    """landmarks, unselected / fixed / rejected poses, edge_active(), the snapshot slots and the counters: bit-equal to before"""
    fp = L.gpu_input("small")
    h = HipSolver(fp, RK_HUBER)
    h.optimize(1)
    mask = np.arange(fp.E) % 7 != 0
    mask[fp.eP == 3] = np.arange((fp.eP == 3).sum()) < 3           # pose 3 keeps 3 edges: FEW_OBSERVATIONS
    h.set_edge_active(mask)
    h.snapshot_state(0)
    select = np.arange(fp.Pt) % 4 != 2
    q0, t0, X0 = h.state()
    counters = h.counters()
    got = h.localize_poses(select=select, seed=L.SEED["small"], min_inliers=10)
    q1, t1, X1 = h.state()
    ok = got["status"] == L.OK
    assert got["status"][3] == L.FEW_OBSERVATIONS and got["status"][fp.Pt - 1] == L.FIXED
    assert (got["status"][~select] == L.NOT_SELECTED).all() and ok.sum() > 20
    assert bits_equal(X1, X0) and bits_equal(q1[~ok], q0[~ok]) and bits_equal(t1[~ok], t0[~ok])
    assert bits_equal(q1[ok], got["q"][ok]) and not np.array_equal(q1[ok], q0[ok])
    assert np.array_equal(h.edge_active(), mask) and h.counters() == counters
    assert not got["edge_inlier"][~mask].any()
    h.restore_state(0)
    assert all(bits_equal(a, b) for a, b in zip(h.state(), (q0, t0, X0)))


def test_covariance_is_dropped_after_a_change():
    fp = L.gpu_input("small")
    h = HipSolver(fp, RK_HUBER)
    h.optimize(3)
    h.covariance(landmarks=False)
    before = h.covariance_blocks()
    h.localize_poses(dry_run=True)
    assert bits_equal(h.covariance_blocks(), before)               # (a dry run keeps it)
    assert h.localize_poses()["ok"] > 0
    with pytest.raises(CubaHipError):
        h.covariance_blocks()


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_optimize_afterwards_equals_a_handle_set_to_that_state(precision):
    fp = L.gpu_input("small")
    h = lost_handle(fp, precision=precision)
    assert h.localize_poses(seed=L.SEED["small"])["ok"] == fp.Pf
    twin = HipSolver(fp, RK_HUBER, precision=precision)
    twin.set_state(*h.state())
    assert all(bits_equal(a, b) for a, b in zip(h.state(), twin.state()))
    assert bits_equal(h.chi_squares(), twin.chi_squares())
    a, b = h.optimize(5)["chi2"], twin.optimize(5)["chi2"]
    assert len(a) == len(b) > 0 and bits_equal(a, b) and all(bits_equal(x, y) for x, y in zip(h.state(), twin.state()))


# ---- 8. the fp32 library ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "wide"])
def test_fp32_library(name):
    case = L.gpu_case(name, 256, f32=True)
    fp = case[0]
    h = lost_handle(fp, precision="f32")
    got = h.localize_poses(hypotheses=256, seed=L.SEED[name])
    check(got, case, f"{name}, fp32 library", f32=True)
    assert bits_equal(h.state()[0], got["q"]) and bits_equal(h.state()[1], got["t"])


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------------------
def status_of(call):
    with pytest.raises(CubaHipError) as e:
        call()
    return int(re.match(r"status (\d+)", str(e.value)).group(1))


def test_errors_and_the_handle_afterwards(small_fp):
    fp = small_fp
    STATE, ARG = 3, 1
    assert status_of(HipSolver(None, RK_HUBER).localize_poses) == STATE
    for part in (lambda s: s.set_partition(0, fp.Lt // 2), lambda s: s.set_graph(fp, landmark_range=(0, fp.Lt // 2))):
        p = HipSolver(fp, RK_HUBER)
        part(p)
        assert status_of(p.localize_poses) == STATE
    h = HipSolver(fp, RK_HUBER)
    before = h.state()
    for bad in (dict(hypotheses=0), dict(hypotheses=4097), dict(min_inliers=-1), dict(chi2_max=(np.nan, 7.815)), dict(chi2_max=(5.991, np.nan)),
                dict(chi2_max=(np.inf, 7.815)), dict(chi2_max=(5.991, np.inf)), dict(chi2_max=(0.0, 7.815)), dict(chi2_max=(5.991, 0.0)), dict(chi2_max=(-1.0, 7.815))):
        assert status_of(lambda: h.localize_poses(**bad)) == ARG
    assert h.lib.cuba_hip_localize_poses(h.h, None, 256, 0, None, 10, 0, None, None, None, None, None, None, None, None) == ARG        # chi2_max NULL
    with pytest.raises(ValueError):
        h.localize_poses(select=np.ones(fp.Pt + 1, bool))
    assert all(bits_equal(a, b) for a, b in zip(h.state(), before))
    # every output is optional, 4096 hypotheses are allowed, and the handle goes on
    assert h.lib.cuba_hip_localize_poses(h.h, None, 4096, 2 ** 64 - 1, (2 * C.c_double)(5.991, 7.815), 0, 1, None, None, None, None, None, None, None, None) == 0
    got = h.localize_poses(hypotheses=64, chi2_max=(1e6, 1e6), min_inliers=0, dry_run=True)
    assert got["ok"] > fp.Pf // 2 and sum(got[k] for k in POSELOC_STATUS_NAMES) == fp.Pt and all(bits_equal(a, b) for a, b in zip(h.state(), before))
    chi2 = h.optimize(5)["chi2"]
    assert len(chi2) > 1 and chi2[-1] < chi2[0]


# ---- 10. a handle that never calls it ------------------------------------------------------------------------------------------------------------
NAMED = ("graph_uploads", "structure_builds", "edge_sorts", "pcg_graph_instantiations", "host_looks", "value_bytes_uploaded")


def run_of(h):
    res = h.optimize(5)
    return dict(chi2=res["chi2"], state=h.state(), counters=h.counters(), pcg=h.pcg_history()[0], named=[h.counter(k) for k in NAMED])


def test_a_handle_that_never_calls_it_runs_as_one_that_did(small_fp):
    """optimize() on a plain handle and on a twin that made a (dry) localisation call before: the same iterates, counters, PCG history,
    uploads, structure builds, sorts and graph instantiations -- the feature hangs nothing onto the solve path"""
    plain = run_of(HipSolver(small_fp, RK_HUBER))
    twin = HipSolver(small_fp, RK_HUBER)
    assert twin.localize_poses(chi2_max=(1e6, 1e6), min_inliers=0, dry_run=True)["ok"] > 0
    called = run_of(twin)
    assert bits_equal(plain["chi2"], called["chi2"]) and all(bits_equal(a, b) for a, b in zip(plain["state"], called["state"]))
    assert plain["counters"] == called["counters"] and np.array_equal(plain["pcg"], called["pcg"]) and plain["named"] == called["named"]

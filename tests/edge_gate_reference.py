"""Reference for edge gating (cuba_hip_gate_edges and friends), numpy + fp64 on a FlatProblem and a state.

An edge stays active iff its chi2 = omega |r|^2 (uploaded omega) is at most the threshold of its kind and -- where asked for -- its point
lies in front of the camera (depth Xc[2] > 0); a NaN fails both tests.  A depth failure counts as "gated by depth" whatever its chi2, a
chi2 failure in front of the camera as "gated by chi2".  Modes: "reclassify" judges every edge afresh, "only_remove" never re-admits an
edge that `prev` has switched off, "dry_run" reports like "reclassify" and leaves `prev` in force.  Projection and rotation are the
oracle's (oracle.project / oracle.rotate), so chi2 equals OracleSolver.chi_squares() to rounding."""
import copy
import ctypes as C

import numpy as np

from oracle import oracle

CHI2_MONO, CHI2_STEREO = 5.991, 7.815
COUNT_NAMES = ("active_mono", "active_stereo", "gated_chi2_mono", "gated_chi2_stereo", "gated_depth", "changed")


def edge_chi2_depth(fp, state=None):
    """(chi2[E], depth[E]) at state = (q, t, Xw), default the FlatProblem's own estimates; caller's edge order"""
    q, t, Xw = (np.ascontiguousarray(a, dtype=np.float64) for a in ((fp.q, fp.t, fp.Xw) if state is None else state))
    cam = np.ascontiguousarray(fp.cam, dtype=np.float64)
    Xc, proj = np.zeros((fp.E, 3)), np.zeros((fp.E, 3))
    # oracle.project edge by edge -- its C function on rows of the arrays (the wrapper's four array conversions per call cost 1 ms per edge)
    orc_project = oracle.lib().orc_project
    at = lambda a, row: C.c_void_p(a.ctypes.data + a.strides[0] * int(row))      # noqa: E731
    for e in range(fp.E):
        p, l = fp.eP[e], fp.eL[e]
        orc_project(at(q, p), at(t, p), at(cam, p), at(Xw, l), C.c_int(int(fp.eDim[e])), at(Xc, e), at(proj, e))
    r = np.where(np.arange(3)[None, :] < fp.eDim[:, None], fp.meas - proj, 0.0)
    return fp.omega * (r * r).sum(1), Xc[:, 2].copy()


def thresholds(fp, chi2_max=(CHI2_MONO, CHI2_STEREO)):
    return np.where(fp.eDim == 3, chi2_max[1], chi2_max[0])


def threshold_margin(fp, chi, chi2_max=(CHI2_MONO, CHI2_STEREO)):
    """|chi2 - threshold| / threshold per edge: how far every decision is from flipping (inf where no rounding can flip it: no chi2 test, a NaN)"""
    thr = thresholds(fp, chi2_max)
    with np.errstate(invalid="ignore"):
        m = np.abs(chi - thr) / thr
    return np.where(np.isfinite(thr) & np.isfinite(chi), m, np.inf)


def classify(fp, state=None, chi2_max=(CHI2_MONO, CHI2_STEREO), positive_depth=True, mode="reclassify", prev=None, chi_depth=None):
    """dict: mask (the gate in force after the call), judged (what "reclassify" would leave), counts (COUNT_NAMES), chi2, depth,
    chi_ok, depth_ok, per_landmark (active edges per landmark under `mask`)"""
    assert mode in ("reclassify", "only_remove", "dry_run")
    chi, depth = edge_chi2_depth(fp, state) if chi_depth is None else chi_depth
    prev = np.ones(fp.E, bool) if prev is None else np.asarray(prev, bool)
    with np.errstate(invalid="ignore"):
        chi_ok = chi <= thresholds(fp, chi2_max)                 # (NaN: False)
        depth_ok = depth > 0 if positive_depth else np.ones(fp.E, bool)
    judged = chi_ok & depth_ok
    now = judged & prev if mode == "only_remove" else judged
    stereo = fp.eDim == 3
    counts = dict(active_mono=int((now & ~stereo).sum()), active_stereo=int((now & stereo).sum()),
                  gated_chi2_mono=int((depth_ok & ~chi_ok & ~stereo).sum()), gated_chi2_stereo=int((depth_ok & ~chi_ok & stereo).sum()),
                  gated_depth=int((~depth_ok).sum()), changed=int((now != prev).sum()))
    mask = prev if mode == "dry_run" else now
    return dict(mask=mask, judged=judged, counts=counts, chi2=chi, depth=depth, chi_ok=chi_ok, depth_ok=depth_ok,
                per_landmark=landmark_counts(fp, mask))


def landmark_counts(fp, mask):
    """active edges of every landmark, caller's landmark order"""
    return np.bincount(fp.eL[np.asarray(mask, bool)], minlength=fp.Lt).astype(np.int32)


def zero_information(fp, mask, omega_scale=1.0):
    """the FlatProblem with the gated edges' information set to 0: what a gated handle optimises"""
    out = copy.copy(fp)
    out.omega = np.where(np.asarray(mask, bool), fp.omega * omega_scale, 0.0)
    return out


def without_edges(fp, mask):
    """the FlatProblem with the gated edges taken out (vertices and their order kept: every vertex must keep an edge)"""
    keep = np.nonzero(np.asarray(mask, bool))[0]
    assert len(np.unique(fp.eL[keep])) == fp.Lt and len(np.unique(fp.eP[keep])) == fp.Pt
    out = copy.copy(fp)
    out.eP, out.eL, out.eDim = fp.eP[keep].copy(), fp.eL[keep].copy(), fp.eDim[keep].copy()
    out.meas, out.omega, out.edge_src = fp.meas[keep].copy(), fp.omega[keep].copy(), fp.edge_src[keep].copy()
    return out


def with_state(fp, state):
    out = copy.copy(fp)
    out.q, out.t, out.Xw = (np.array(a, dtype=np.float64) for a in state)
    return out


def mask_keeping_two_per_landmark(fp, rng, fraction=0.15):
    """a random mask that switches off about `fraction` of the edges and leaves every landmark at least two and every pose at least one"""
    mask = np.ones(fp.E, bool)
    per_lm, per_pose = np.bincount(fp.eL, minlength=fp.Lt), np.bincount(fp.eP, minlength=fp.Pt)
    for e in rng.permutation(fp.E)[: int(fraction * fp.E)]:
        if per_lm[fp.eL[e]] > 2 and per_pose[fp.eP[e]] > 1:
            mask[e] = False; per_lm[fp.eL[e]] -= 1; per_pose[fp.eP[e]] -= 1
    return mask

"""wall time of one cuba_hip_localize_poses call (256 hypotheses, warm handle; the call ends in a stream synchronise) on ONE selected pose,
on 16 and on all poses, with and without every output copied back, at KITTI-07 and KITTI-00 size, against
  1. get_solution + set_solution on the same handle, the floor of any host-side RANSAC
  2. refine_poses(4, 10) on the same selection, the step it precedes
Every timed localisation starts from NaN in the selected poses (set_state outside the timed region), every timed refinement from the
localised poses.  Medians of 30 calls after 4 warm-up calls of the same shape."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (the repository: this file lies in scripts/)
sys.path.insert(0, ROOT)
from cuba_amd.capi import HipSolver, _d  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_named  # noqa: E402

RK = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))


def med(fn, prepare=None, n=30, warm=4):
    ts = []
    for i in range(warm + n):
        if prepare:
            prepare()
        t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
        if i >= warm:
            ts.append(dt)
    ts = np.array(ts) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


for name in ("kitti07", "kitti00"):
    fp = flatten(synth_named(name, perturb=False))
    per_pose = np.bincount(fp.eP, minlength=fp.Pt)
    for precision in ("f64", "f32"):
        h = HipSolver(fp, RK, precision=precision)
        h.optimize(1)
        h.set_state(fp.q, fp.t, fp.Xw)
        thr = (2 * C.c_double)(5.991, 7.815)
        counts = (C.c_int64 * 6)()
        ip, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        status, inl, win = np.zeros(fp.Pt, np.int32), np.zeros(fp.Pt, np.int32), np.zeros(fp.Pt, np.int32)
        cost, q, t, edge = np.zeros(fp.Pt), np.zeros((fp.Pt, 4)), np.zeros((fp.Pt, 3)), np.zeros(fp.E, np.uint8)
        qs, ts_, X = h.state()

        def trip():
            h.lib.cuba_hip_get_solution(h.h, _d(qs), _d(ts_), _d(X))
            h.lib.cuba_hip_set_solution(h.h, _d(qs), _d(ts_), None)
        print(f"{name} {precision}: Pt {fp.Pt} E {fp.E}, edges per pose median {int(np.median(per_pose))} max {int(per_pose.max())}", flush=True)
        print(f"{name} {precision}: get_solution + set_solution(q, t)               median %.3f ms (min %.3f max %.3f)" % med(trip), flush=True)
        mid = fp.Pf // 2
        for what, chosen in (("1 pose", [mid]), ("16 poses", list(range(mid, min(mid + 16, fp.Pf)))), ("all poses", None)):
            sel = None
            if chosen is not None:
                sel = np.zeros(fp.Pt, np.uint8); sel[chosen] = 1
            selp = sel.ctypes.data_as(u8) if sel is not None else None
            lost = (np.arange(fp.Pt) < fp.Pf) if sel is None else sel.astype(bool)
            q0, t0 = fp.q.copy(), fp.t.copy()
            q0[lost] = np.nan; t0[lost] = np.nan
            reset = lambda: h.set_state(q0, t0, fp.Xw)      # noqa: E731
            bare = lambda: h.lib.cuba_hip_localize_poses(h.h, selp, 256, 0, thr, 10, 0, None, counts, None, None, None, None, None, None)      # noqa: E731
            full = lambda: h.lib.cuba_hip_localize_poses(h.h, selp, 256, 0, thr, 10, 0, status.ctypes.data_as(ip), counts, inl.ctypes.data_as(ip),      # noqa: E731
                                                         _d(cost), win.ctypes.data_as(ip), _d(q), _d(t), edge.ctypes.data_as(u8))
            reset()
            assert bare() == 0
            found = list(counts)
            print(f"{name} {precision}: {what}: counts {found}", flush=True)
            print(f"{name} {precision}: localize_poses 256, {what:9s} (counts only)    median %.3f ms (min %.3f max %.3f)" % med(bare, reset), flush=True)
            print(f"{name} {precision}: localize_poses 256, {what:9s} (+ every output) median %.3f ms (min %.3f max %.3f)" % med(full, reset), flush=True)
            reset(); bare()
            q1, t1, _ = h.state()
            start = lambda: h.set_state(q1, t1, fp.Xw)      # noqa: E731
            refine = lambda: h.lib.cuba_hip_refine_poses(h.h, selp, 4, 10, 2, thr, 10, 0, None, counts, None, None, None, None, None)      # noqa: E731
            if not np.isnan(q1).any():
                print(f"{name} {precision}: refine_poses 4 x 10,  {what:9s} (counts only)    median %.3f ms (min %.3f max %.3f)" % med(refine, start), flush=True)
        h.close()

"""wall time of one cuba_hip_refine_poses call (all poses, 4 rounds of 10 trials, warm handle; the call ends in a stream synchronise), with
and without the outputs copied back, at KITTI-07 and KITTI-00 size, against what a caller had before:
  1. a twin handle of the same graph with every landmark fixed -- upload and structure build timed apart -- and optimize(40) on it
  2. get_solution + set_solution on the same handle, the floor of any host-side refinement
Every timed call starts from the same perturbed poses (set_state outside the timed region)."""
import copy
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


def all_landmarks_fixed(fp):
    """the same graph as a FlatProblem whose landmarks are all fixed (Lf = 0): the pose-only problem through the general solver"""
    out = copy.copy(fp)
    keep = fp.eP < fp.Pf                 # (an edge between a fixed pose and a fixed landmark is no part of a graph)
    out.Lf = 0
    out.eP, out.eL, out.eDim, out.meas, out.omega, out.edge_src = fp.eP[keep], fp.eL[keep], fp.eDim[keep], fp.meas[keep], fp.omega[keep], fp.edge_src[keep]
    return out


for name in ("kitti07", "kitti00"):
    g = synth_named(name, perturb=False)
    fp = flatten(g)
    rng = np.random.default_rng(3)
    # the start: every pose about 1 degree and 0.1 m off
    from scipy.spatial.transform import Rotation
    dq = Rotation.from_rotvec(np.deg2rad(1.0) * rng.uniform(-1, 1, (fp.Pt, 3)))
    q0 = (dq * Rotation.from_quat(fp.q)).as_quat()
    q0[q0[:, 3] < 0] *= -1
    t0 = dq.apply(fp.t) + 0.1 * rng.uniform(-1, 1, (fp.Pt, 3))
    q0[fp.Pf:], t0[fp.Pf:] = fp.q[fp.Pf:], fp.t[fp.Pf:]
    for precision in ("f64", "f32"):
        h = HipSolver(fp, RK, precision=precision)
        h.optimize(1)
        reset = lambda: h.set_state(q0, t0, fp.Xw)      # noqa: E731
        thr = (2 * C.c_double)(5.991, 7.815)
        counts = (C.c_int64 * 6)()
        ip = C.POINTER(C.c_int32)
        status, inl = np.zeros(fp.Pt, np.int32), np.zeros(fp.Pt, np.int32)
        chi2, q, t, edge = np.zeros(fp.Pt), np.zeros((fp.Pt, 4)), np.zeros((fp.Pt, 3)), np.zeros(fp.E, np.uint8)
        bare = lambda: h.lib.cuba_hip_refine_poses(h.h, None, 4, 10, 2, thr, 10, 0, None, counts, None, None, None, None, None)      # noqa: E731
        full = lambda: h.lib.cuba_hip_refine_poses(h.h, None, 4, 10, 2, thr, 10, 0, status.ctypes.data_as(ip), counts, inl.ctypes.data_as(ip),      # noqa: E731
                                                   _d(chi2), _d(q), _d(t), edge.ctypes.data_as(C.POINTER(C.c_uint8)))
        qs, ts_, X = h.state()

        def trip():
            h.lib.cuba_hip_get_solution(h.h, _d(qs), _d(ts_), _d(X))
            h.lib.cuba_hip_set_solution(h.h, _d(qs), _d(ts_), None)
        reset()
        assert bare() == 0
        print(f"{name} {precision}: Pt {fp.Pt} E {fp.E} counts {list(counts)}", flush=True)
        print(f"{name} {precision}: refine_poses 4 x 10 (counts only)      median %.3f ms (min %.3f max %.3f)" % med(bare, reset), flush=True)
        print(f"{name} {precision}: refine_poses 4 x 10 (+ every output)   median %.3f ms (min %.3f max %.3f)" % med(full, reset), flush=True)
        print(f"{name} {precision}: get_solution + set_solution(q, t)      median %.3f ms (min %.3f max %.3f)" % med(trip), flush=True)
        h.close()
        # the twin with every landmark fixed
        fixed = all_landmarks_fixed(fp)
        t_up = []
        twin = None
        for _ in range(3):
            if twin is not None:
                twin.close()
            a = time.perf_counter()
            twin = HipSolver(fixed, RK, precision=precision)
            twin.build_structure()
            t_up.append((time.perf_counter() - a) * 1e3)
        print(f"{name} {precision}: twin (all landmarks fixed): create + upload + structure %.3f ms (best of 3)" % min(t_up), flush=True)
        resets = lambda: twin.set_state(q0, t0, fp.Xw)      # noqa: E731
        print(f"{name} {precision}: twin optimize(40)                      median %.3f ms (min %.3f max %.3f)" % med(lambda: twin.optimize(40), resets, n=10, warm=2), flush=True)
        twin.close()

"""wall time of one cuba_hip_triangulate_landmarks call (all landmarks, 5 iterations, warm handle; the call ends in a stream synchronise)
against get_solution + set_solution on the same handle, at KITTI-07 and KITTI-00 size"""
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


def med(fn, n=40, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e3
    return float(np.median(ts)), float(ts.min()), float(ts.max())


for name in ("kitti07", "kitti00"):
    fp = flatten(synth_named(name))
    for precision in ("f64", "f32"):
        h = HipSolver(fp, RK, precision=precision)
        h.optimize(2)
        thr = (2 * C.c_double)(5.991, 7.815)
        counts = (C.c_int64 * 8)()
        status = np.zeros(fp.Lt, np.int32); xyz = np.zeros((fp.Lt, 3))
        bare = lambda: h.lib.cuba_hip_triangulate_landmarks(h.h, None, 5, 1.0, thr, 0, None, counts, None)      # noqa: E731
        full = lambda: h.lib.cuba_hip_triangulate_landmarks(h.h, None, 5, 1.0, thr, 0, status.ctypes.data_as(C.POINTER(C.c_int32)), counts, _d(xyz))  # noqa: E731
        q, t, X = h.state()

        def trip():
            h.lib.cuba_hip_get_solution(h.h, _d(q), _d(t), _d(X))
            h.lib.cuba_hip_set_solution(h.h, None, None, _d(X))
        assert bare() == 0
        print(f"{name} {precision}: Lt {fp.Lt} E {fp.E} counts {list(counts)}", flush=True)
        print(f"{name} {precision}: triangulate (counts only)        median %.3f ms (min %.3f max %.3f)" % med(bare), flush=True)
        print(f"{name} {precision}: triangulate (+ status and xyz)  median %.3f ms (min %.3f max %.3f)" % med(full), flush=True)
        print(f"{name} {precision}: get_solution + set_solution(Xw) median %.3f ms (min %.3f max %.3f)" % med(trip), flush=True)
        h.close()

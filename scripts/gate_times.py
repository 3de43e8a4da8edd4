"""Outlier handling between two LM runs: edge gating against the route without it.

    python scripts/gate_times.py [--shape kitti00] [--route a|b] [--reps 20] [--out file.json]

From the state after optimize(5), restored before every repetition (one warm-up, then --reps timed ones), with HIP events on the
handle's stream and a host clock:

  a  the gated route: gate_edges() + optimize(10) on the handle as it stands.  Timed twice: from an ungated handle (the first gating
     call of a graph allocates the live information and the mask) and from a handle that holds a gate already.  Also the gate_edges()
     call alone (dry run: classification, counts, their read-back).
  b  the route of a library without gating: chi_squares() -> mask on the host -> the edge arrays without the outliers -> set_graph ->
     build_structure -> optimize(10).  Uses nothing of the gating API, so it also runs on a build that has none.

Both routes print the final chi2 of their optimize(10): the same objective on the same edges, to the solver's tolerance."""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_named  # noqa: E402

RK_HUBER = ((1, float(np.sqrt(5.991))), (1, float(np.sqrt(7.815))))
CHI2_MAX = (5.991, 7.815)


class Timer:
    """host clock and HIP events around a block, on the handle's stream"""
    def __init__(self, h):
        p = C.c_void_p()
        h._ck(h.lib.cuba_hip_get_stream(h.h, C.byref(p)))
        self.stream = torch.cuda.ExternalStream(p.value) if p.value else torch.cuda.default_stream()
        self.host, self.device = [], []

    def __enter__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        self.e0.record(self.stream)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.e1.record(self.stream)
        self.e1.synchronize()
        self.host.append(1e3 * (time.perf_counter() - self.t0))
        self.device.append(self.e0.elapsed_time(self.e1))

    def report(self):
        h, d = np.array(self.host[1:]), np.array(self.device[1:])            # (repetition 0 is the warm-up)
        return dict(host_ms_median=float(np.median(h)), host_ms_min=float(h.min()), event_ms_median=float(np.median(d)), event_ms_min=float(d.min()))


def with_state(fp, state):
    out = copy.copy(fp)
    out.q, out.t, out.Xw = state
    return out


def without_edges(fp, keep):
    out = copy.copy(fp)
    out.eP, out.eL, out.eDim, out.meas, out.omega = fp.eP[keep], fp.eL[keep], fp.eDim[keep], fp.meas[keep], fp.omega[keep]
    out.edge_src = fp.edge_src[keep]
    return out


def route_a(fp, reps):
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    h.snapshot_state()
    out = {}
    for name in ("from_an_ungated_handle", "from_a_gated_handle"):
        t = Timer(h)
        for _ in range(reps + 1):
            h.restore_state()
            h.set_edge_active(None if name == "from_an_ungated_handle" else np.ones(fp.E, bool))
            with t:
                counts = h.gate_edges(CHI2_MAX)
                chi2 = h.optimize(10)["chi2"]
        out[name] = dict(t.report(), final_chi2=float(chi2[-1]), iterations=len(chi2), gated=fp.E - counts["active_mono"] - counts["active_stereo"])
    t = Timer(h)
    h.restore_state(); h.set_edge_active(None)
    for _ in range(reps + 1):
        with t:
            h.gate_edges(CHI2_MAX, mode="dry_run")
    out["gate_edges_alone"] = t.report()
    out["landmarks_with_fewer_than_two_active_edges"] = int((h.landmark_active_edges() < 2).sum())
    h.close()
    return out


def route_b(fp, reps):
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    at5 = with_state(fp, h.state())
    thr = np.where(fp.eDim == 3, CHI2_MAX[1], CHI2_MAX[0])
    t = Timer(h)
    for _ in range(reps + 1):
        h.set_graph(at5); h.build_structure(); h.compute_errors()          # the full graph at the state after optimize(5), untimed
        with t:
            keep = h.chi_squares() <= thr
            pruned = without_edges(at5, keep)
            h.set_graph(pruned)
            h.build_structure()
            chi2 = h.optimize(10)["chi2"]
    out = dict(t.report(), final_chi2=float(chi2[-1]), iterations=len(chi2), gated=int((~keep).sum()))
    h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="kitti00")
    ap.add_argument("--route", default="a", choices=["a", "b"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    fp = flatten(synth_named(a.shape))
    out = dict(shape=a.shape, poses=fp.Pf, landmarks=fp.Lf, edges=fp.E, reps=a.reps, route=a.route)
    out.update((route_a if a.route == "a" else route_b)(fp, a.reps))
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

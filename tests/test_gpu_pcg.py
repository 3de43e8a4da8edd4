"""The reduced solve's block PCG (csrc/ba_pcg.hip) iterate by iterate against a plain fp64 two-level PCG of the same operator
(tests/pcg_emulator.py), on the handle's own reduced matrix: every kernel path the configuration rules can select, each case asserting
from HipSolver.pcg_config() that it ran the path it names.

a. Iterates.  A fresh handle per K (pcg_max_iter = K, the best iterate accepted, no exact-solver fallback, a tolerance that never
   fires; the coarse inverse is then the one inverted in line from this very matrix) stops with xp = x_K, the K-th iterate -- checked
   against x_{K-1} too.  K = 1 pins z_0 = M^-1 b, K = 2 A z_0; 4 / 5, 8 / 9, 16 / 17 straddle the batches of four iterations and the
   chunks of the hipGraph path.  Two dampings: 1e-5 and 1e-2 x max_diagonal.
b. Stop test.  The device's iteration count equals the first k with r_k.z_k <= tol^2 r_0.z_0 of the fp64 recursion.
c. True residual.  At the four BASELINE shapes, after a converged solve, sqrt(r.M^-1 r / r_0.z_0) with r = bsc - A xp in fp64: the
   device's recursive residual must not have drifted from the true one."""
import functools
import gc
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from pcg_emulator import TwoLevelPCG, stop_iteration  # noqa: E402
from test_gpu_configs import hub_graph, shuffled_pose_ids  # noqa: E402

from conftest import RK_HUBER, with_fixed  # noqa: E402
from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba, synth_named  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9, 16, 17)
DAMPINGS = (1e-5, 1e-2)
NEVER = 1e-30               # pcg_tol of the iterate tests (the recursive r.z can fall below 1e-60 r0.z0 within 12 iterations at the larger damping)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "small":          # 39 free poses
        return flatten(synth_ba(40, 600, 2400, seed=1))
    if name == "mid":            # 299 free poses: odd, so pcg_aggregate 2 leaves a lone last pose, 4 and 8 a short last aggregate
        return flatten(synth_ba(300, 3000, 12000, seed=11))
    if name == "rows":           # 699 free poses: aggregates of 168 / 336 / 600 poses are 5 / 3 / 2 aggregates
        return flatten(synth_ba(700, 4000, 16000, seed=13))
    if name == "big":            # 1599 free poses: more than 1536, so four block rows per SpMV workgroup
        return flatten(synth_ba(1600, 8000, 32000, seed=12))
    if name == "fixed":          # Pf < Pt: fixed poses inside the trajectory
        return flatten(with_fixed(synth_ba(120, 1500, 6000, seed=14), fixed_pose_rows=(7, 30, 31, 64, 119)))
    if name == "hub":            # a pose co-visible with more than 60 others
        return flatten(hub_graph())
    if name == "shuffled":       # shuffled pose ids: the library renumbers the free poses internally
        return flatten(shuffled_pose_ids(synth_named("kitti07"), seed=5))
    return flatten(synth_named(name))


def nc_class(cfg):
    Nc = 6 * cfg["cl"] * cfg["nc"]
    if not cfg["coarse_fp32"]:
        return "f64:" + ("<=768" if Nc <= 768 else ">768")
    return "f32:" + ("<=768" if Nc <= 768 else "<=1536" if Nc <= 1536 else ">1536")


# name: (graph, options, precision, what pcg_config() must show)
CASES = {
    "two_launch": ("small", {}, "f64", dict(spmv_rows=2, upper=0, cl=2, coarse_fp32=1)),
    "two_launch_fp64_coarse": ("small", dict(precond_fp32=0), "f64", dict(spmv_rows=2, upper=0, coarse_fp32=0)),
    "block_jacobi_rows2": ("mid", dict(pcg_aggregate=0), "f64", dict(spmv_rows=2, agg=0)),
    "block_jacobi_rows4": ("big", dict(pcg_aggregate=0), "f64", dict(spmv_rows=4, agg=0, upper=0)),
    "row_kernel_rows4": ("big", dict(spmv_upper=0), "f64", dict(spmv_rows=4, upper=0)),
    "upper_automatic": ("big", {}, "f64", dict(spmv_rows=4, upper=1)),
    "upper_forced_small": ("mid", dict(spmv_upper=1), "f64", dict(spmv_rows=2, upper=1)),
    "coarse_constant": ("mid", dict(coarse_linear=0), "f64", dict(cl=1)),
    "coarse_constant_upper": ("mid", dict(coarse_linear=0, spmv_upper=1, precond_fp32=0), "f64", dict(cl=1, upper=1)),
    "lone_last_f32_nc_gt1536": ("mid", dict(pcg_aggregate=2), "f64", dict(agg=2, cl=2, nc=150, coarse_fp32=1)),
    "lone_last_f64_nc_gt768": ("mid", dict(pcg_aggregate=2, precond_fp32=0), "f64", dict(agg=2, nc=150, coarse_fp32=0)),
    "lone_last_upper": ("mid", dict(pcg_aggregate=2, spmv_upper=1), "f64", dict(agg=2, upper=1)),
    "short_last_f32_nc_le1536": ("mid", dict(pcg_aggregate=4), "f64", dict(agg=4, nc=75, coarse_fp32=1)),
    "short_last_f64_nc_gt768": ("mid", dict(pcg_aggregate=4, precond_fp32=0), "f64", dict(agg=4, nc=75, coarse_fp32=0)),
    "short_last_f32_nc_le768": ("mid", dict(pcg_aggregate=8), "f64", dict(agg=8, nc=38, coarse_fp32=1)),
    "short_last_f64_nc_le768": ("mid", dict(pcg_aggregate=8, precond_fp32=0), "f64", dict(agg=8, nc=38, coarse_fp32=0)),
    "rows_ept2": ("rows", dict(spmv_upper=1, pcg_aggregate=168), "f64", dict(agg=168, upper=1, rows_ept=2)),
    "rows_ept4": ("rows", dict(spmv_upper=1, pcg_aggregate=336), "f64", dict(agg=336, upper=1, rows_ept=4)),
    "rows_ept8": ("rows", dict(spmv_upper=1, pcg_aggregate=600, precond_fp32=0), "f64", dict(agg=600, upper=1, rows_ept=8)),
    "big_nc_gt1536_rows4": ("big", dict(pcg_aggregate=8, spmv_upper=0), "f64", dict(agg=8, nc=200, spmv_rows=4, upper=0)),
    "fixed_poses": ("fixed", {}, "f64", dict(spmv_rows=2)),
    "ell_over": ("hub", {}, "f64", dict(ell_over=1)),
    "ell_over_upper": ("hub", dict(spmv_upper=1), "f64", dict(ell_over=1, upper=1)),
    "shuffled_reorder": ("shuffled", {}, "f64", dict(spmv_rows=2)),
    "f32_library": ("mid", {}, "f32", dict(coarse_fp32=0)),
    "f32_library_upper": ("mid", dict(spmv_upper=1), "f32", dict(coarse_fp32=0, upper=1)),
}
GRAPH_CASES = ("two_launch", "upper_forced_small", "block_jacobi_rows2")   # the same, replayed as hipGraphs

# max-norm relative agreement with the emulator's x_K, over both dampings and every K: a few times the worst value measured (fp64 storage
# of the coarse inverse 6.9e-13, fp32 storage 8.8e-10 -- an Ac^-1 entry whose fp32 rounding flips between LAPACK's inverse and the device's
# Gauss-Jordan sweep --, fp32 library 4.1e-6)
BAR = {"f64": 3e-12, "f32coarse": 3e-9, "f32": 1.5e-5}


def bar_for(precision, cfg):
    return BAR["f32"] if precision == "f32" else BAR["f32coarse"] if cfg["coarse_fp32"] else BAR["f64"]


def prepare(fp, precision, rel_lam, **opts):
    """a fresh handle, linearised, damped and reduced; returns (handle, lam, (rp, ci, v), bsc, config)"""
    h = HipSolver(fp, RK_HUBER, precision=precision, **opts)
    h.compute_errors(); h.build_system()
    lam = rel_lam * h.max_diagonal()
    h.set_lambda(lam); h.schur()
    return h, lam, h.hsc(), h.array("bsc"), h.pcg_config()


def emulator(hsc, lam, cfg):
    rp, ci, v = hsc
    return TwoLevelPCG(rp, ci, v, lam, cfg["agg"], cfg["cl"], order=cfg["pose_order"], coarse_fp32=bool(cfg["coarse_fp32"]))


def check_config(cfg, want, name):
    got = {k: cfg[k] for k in want}
    assert got == want, f"{name}: ran {got}, meant {want}"


def relerr(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_iterates_follow_the_fp64_recursion(name):
    gname, opts, precision, want = CASES[name]
    fp = graph(gname)
    worst, cfg0 = 0.0, None
    for rel_lam in DAMPINGS:
        ref = None
        for K in KS:
            h, lam, hsc, bsc, cfg = prepare(fp, precision, rel_lam, pcg_max_iter=K, pcg_accept_unconverged=1, direct_fallback=0,
                                            pcg_tol=NEVER, **opts)
            check_config(cfg, want, name)
            if gname == "shuffled":
                assert not np.array_equal(cfg["pose_order"], np.arange(fp.Pf)), "the internal renumbering is not active"
            if ref is None:
                em = emulator(hsc, lam, cfg)
                ref = em.run(bsc, max(KS), keep=range(max(KS) + 1))
                cfg0 = cfg
            h.solve_reduced()
            x = h.array("xp")
            hist, _ = h.pcg_history()
            h.close()
            # the stop test fires only where the recursive r.z has fallen below NEVER^2 r0.z0 (far below rounding: the iterates no
            # longer move); the iteration count is K before that
            kdone, ks = abs(int(hist[-1])), stop_iteration(ref["rz"], NEVER)
            assert kdone == K if ks is None or K < ks - 1 else ks - 1 <= kdone <= K, (name, K, hist, ks)
            e = relerr(x, ref["x"][kdone])
            if K <= 3:          # xp after a stop at max_iter is x_K, not x_{K-1}
                assert e < 1e-2 * relerr(ref["x"][K - 1], ref["x"][K]), (name, K, e)
            worst = max(worst, e)
            assert e <= bar_for(precision, cfg), f"{name}: K = {K}, damping {rel_lam:g} x max diagonal: relative error {e:.2e}"
    c = {k: v for k, v in cfg0.items() if k != "pose_order"}
    print(f"\n[pcg iterates] {name}: {c} class {nc_class(cfg0) if cfg0['agg'] else '-'} Pf {fp.Pf} worst rel err {worst:.2e}")


@pytest.mark.parametrize("name", GRAPH_CASES)
def test_iterates_on_the_hipgraph_path(name):
    """pcg_graph = 1: the first solve of a handle runs plain launches while its graphs are built; the second, on the same matrix, replays
    them (its coarse inverse is the overlapped inversion of the same matrix)"""
    gc.collect()                           # (hipGraphs only while one handle is alive)
    gname, opts, precision, want = CASES[name]
    fp = graph(gname)
    worst = 0.0
    for K in KS:
        h, lam, hsc, bsc, cfg = prepare(fp, precision, DAMPINGS[0], pcg_max_iter=K, pcg_accept_unconverged=1, direct_fallback=0,
                                        pcg_tol=NEVER, pcg_graph=1, **opts)
        check_config(cfg, want, name)
        h.solve_reduced()
        time.sleep(0.2)                    # (the helper thread finishes the graphs)
        plain = h.counter("pcg_iterations_plain_launches")
        h.compute_errors(); h.build_system(); h.set_lambda(lam); h.schur()
        again = emulator(h.hsc(), lam, cfg).A      # (the solve left full diagonal blocks: compare the matrices, not the storage)
        assert (again != emulator(hsc, lam, cfg).A).nnz == 0 and np.array_equal(h.array("bsc"), bsc)
        h.solve_reduced()
        x = h.array("xp")
        assert h.counter("pcg_graph_instantiations") > 0 and h.counter("pcg_iterations_plain_launches") == plain, "no graph replayed"
        h.close()
        ref = emulator(hsc, lam, cfg).run(bsc, K, keep=(K,))
        e = relerr(x, ref["x"][K])
        worst = max(worst, e)
        assert e <= bar_for(precision, cfg), f"{name} (hipGraphs): K = {K}: relative error {e:.2e}"
    print(f"\n[pcg iterates, hipGraphs] {name}: worst rel err {worst:.2e}")


STOP_CASES = [n for n in sorted(CASES) if CASES[n][2] == "f64"]


@pytest.mark.parametrize("tol", [1e-7, 1e-10])
@pytest.mark.parametrize("name", STOP_CASES)
def test_stop_iteration_matches_the_recursion(name, tol):
    gname, opts, precision, want = CASES[name]
    fp = graph(gname)
    h, lam, hsc, bsc, cfg = prepare(fp, precision, DAMPINGS[0], pcg_tol=tol, pcg_max_iter=5000, direct_fallback=0, **opts)
    assert h.solve_reduced()
    hist, bad = h.pcg_history()
    h.close()
    assert bad == 0 and hist[-1] > 0, (name, hist)
    got = int(hist[-1])
    ref = emulator(hsc, lam, cfg).run(bsc, got + 8)
    k = stop_iteration(ref["rz"], tol)
    ratio = ref["rz"] / (tol * tol * ref["rz"][0])
    near = np.abs(ratio[max(0, min(got, k or got) - 1):max(got, k or got) + 1] - 1) < 1e-6
    print(f"\n[pcg stop] {name} tol {tol:g}: device {got}, fp64 recursion {k}")
    if k != got and near.any():
        print(f"exempt: r.z within 1e-6 relative of tol^2 r0.z0 at the stop (device {got}, recursion {k})")
        return
    assert got == k, f"{name}: device stopped after {got} iterations, the fp64 recursion after {k} (r.z / tol^2 r0.z0 there: {ratio[got]:.3e})"


# (shape, options): the four BASELINE shapes at default options, and kitti00 / s2m with the upper-triangle iteration forced each way
RESIDUAL_CASES = [("kitti07", {}), ("kitti00", {}), ("s2m", {}), ("g4m", {}), ("kitti00", dict(spmv_upper=1)), ("kitti00", dict(spmv_upper=0)),
                  ("s2m", dict(spmv_upper=1)), ("s2m", dict(spmv_upper=0))]
RESIDUAL_FACTOR = 1.5         # measured: 0.42 ... 0.58


@pytest.mark.parametrize("shape,opts", RESIDUAL_CASES, ids=[f"{s}-{'-'.join(f'{k}{v}' for k, v in o.items()) or 'default'}" for s, o in RESIDUAL_CASES])
def test_true_residual_at_convergence(shape, opts):
    """sqrt(r.M^-1 r / r_0.z_0) of the TRUE residual r = bsc - A xp stays within a small factor of pcg_tol: the recursive residual the
    device's stop test reads has not drifted"""
    fp = graph(shape)
    h, lam, hsc, bsc, cfg = prepare(fp, "f64", DAMPINGS[0], direct_fallback=0, **opts)
    if "spmv_upper" in opts:
        assert cfg["upper"] == opts["spmv_upper"]
    tol = 1e-7
    assert h.solve_reduced()
    hist, bad = h.pcg_history()
    x = h.array("xp")
    h.close()
    assert bad == 0 and hist[-1] > 0
    em = emulator(hsc, lam, cfg)
    r = bsc - em.matvec(x)
    ratio = np.sqrt(float(r @ em.minv(r)) / float(bsc @ em.minv(bsc)))
    c = {k: v for k, v in cfg.items() if k != "pose_order"}
    print(f"\n[pcg true residual] {shape} {opts}: {c}, {int(hist[-1])} iterations, true M^-1-norm residual / tol = {ratio / tol:.3f}")
    assert ratio <= RESIDUAL_FACTOR * tol, f"{shape}: true relative residual {ratio:.3e} against pcg_tol {tol:g}"

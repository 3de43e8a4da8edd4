"""cuba_hip_optimize_batch class by class: every kernel class the batched launch chain can select, against solo runs bit for bit.

The batched wrappers (csrc: lm_pass_batch_kernel, schur_pass_batch_kernel, pcg_setup_expand_batch_kernel, pcg2_fused_batch_kernel,
pcg_spmv_batch_kernel, pcg_advance_batch_kernel, trial_tail_batch_kernel, reduce_report_batch_kernel, restore_if_rejected_batch_kernel,
dense_gj_*_batch_kernel) take blockIdx.y as the graph number and read their arguments from a device table; launch sizes are maxima over
the graphs, the kernel instantiation comes from the first graph in the PCG.  The contract: per graph the kernels, their arguments and
their order are the solo run's, so every result is bit-identical to cuba_hip_optimize on the handle alone.

Reference of every handle of every batch: a fresh solo handle with the same graph, robust kernels, options and start, driven by the same
sequence of calls.  Compared with np.array_equal: chi2 per iteration, state(), the "lm_trials" counter, pcg_history()[0] (and the
increment array("xp") in the iterate cases).  Bit-identity to solo is correctness because tests/test_gpu_pcg.py holds the SOLO wrapper of
each class to the fp64 emulator iterate by iterate; so each case asserts from pcg_config() which class it ran, and from the lead's
"batch_full_trials" / "batch_iteration_trials" counters which of the batch driver's two modes ran.  Wherever a case runs the fp64 library at the
default tolerance the batched chi2 per iteration is also held to OracleSolver within CHI2_TOL of tests/test_gpu_configs.py.

Cases: 1 every (storage, Nc bucket, cl) class with the smallest and with the largest graph as hs[0]; 2 both SpMV instantiations (the
768-workgroup rule of launch_pcg_batch_iteration); 3 iterates with per-graph pcg_max_iter 1 / 4 / 5 / 17; 4 mixed precision (all
handles: full path; one of two: iterations-only path); 5 a run that ends inside the batch (table index != handle index); 6 failing
reduced solves inside a batch; 7 the limits of the call (64, 65, 1 handle, two tolerances, one stream, one handle twice); 8 a second call
on the same handles, bitwise; 9 fixed vertices and internal renumbering; 10 a handle that leaves its class in the middle of the call
(fp32-stored coarse inverse dropped after a PCG breakdown), on the full and on the iterations-only path.  DESIGN.md section 5."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_gpu_configs import CHI2_TOL  # noqa: E402
from test_gpu_pcg import graph as pcg_graph  # noqa: E402

from conftest import RK_HUBER, RK_NONE  # noqa: E402
from cuba_amd.capi import CubaHipError, HipSolver, optimize_batch  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

pytestmark = pytest.mark.gpu

NEVER = 1e-30
_graphs, _solo, _oracle, _starts = {}, {}, {}, {}


def graph(name):
    """the small graphs of tests/test_gpu_pcg.py, and a few of other sizes that fall into the same Nc buckets"""
    if name not in _graphs:
        if name[0] == "g" and name[1:].isdigit():                 # g450: 449 free poses, g515: 514, g600: 599
            P = int(name[1:])
            _graphs[name] = flatten(synth_ba(P, 10 * P, 40 * P, seed=P))
        elif name == "clean":       # 39 free poses, no outliers, ground-truth start: LM converges to rounding level within 30 iterations
            _graphs[name] = flatten(synth_ba(40, 600, 2400, seed=1, outlier_frac=0.0, perturb=False))
        elif name == "gaugefree":   # the graph of test_fp32_coarse_inverse_falls_back_when_the_pcg_breaks_down (tests/test_gpu_parity.py)
            _graphs[name] = flatten(synth_ba(96, 3000, 12000, seed=21, stereo_frac=0.0, fix_first=False))
        else:
            _graphs[name] = pcg_graph(name)
    return _graphs[name]


def spec(gname, start=None, precision="f64", **opts):
    """one handle of a batch: (graph, start, library, options) -- hashable, so that solo and oracle references are computed once"""
    return (gname, start, precision, tuple(sorted(opts.items())))


def start_state(sp):
    """start None: the graph's own estimates; an int: landmarks and free-pose translations moved by seeded noise; "converged": the end
    state of a 60-iteration OracleSolver run"""
    gname, start = sp[0], sp[1]
    fp = graph(gname)
    if start is None:
        return fp.q, fp.t, fp.Xw
    if (gname, start) not in _starts:
        if start == "converged":
            from oracle.oracle import OracleSolver
            o = OracleSolver(fp, RK_HUBER)
            o.optimize(60)
            _starts[(gname, start)] = o.state()
        else:
            rng = np.random.default_rng(1000 + start)
            t = fp.t.copy()
            t[:fp.Pf] += rng.normal(0, 0.02, (fp.Pf, 3))
            _starts[(gname, start)] = (fp.q, t, fp.Xw + rng.normal(0, 0.05, fp.Xw.shape))
    return _starts[(gname, start)]


def make(sp):
    gname, start, precision, opts = sp
    opts = dict(opts)
    rk = RK_NONE if opts.pop("robust_none", 0) else RK_HUBER         # ("robust_none" is this file's, not an option of the library)
    h = HipSolver(graph(gname), rk, precision=precision, **opts)
    if start is not None:
        h.set_state(*start_state(sp))
    return h


def record(h, chi2, xp):
    r = dict(chi2=chi2, state=h.state(), trials=h.counters()["lm_trials"], hist=h.pcg_history()[0].copy(), bad=h.pcg_history()[1],
             fallbacks=h.counter("precond_fp32_fallbacks"), coarse_fp32=h.pcg_config()["coarse_fp32"])
    if xp:
        r["xp"] = h.array("xp")
    return r


def solo(sp, plan, xp=False):
    """the reference: a fresh handle alone, driven by the same calls (an int n = optimize(n), "reset" = set_state to the start)"""
    key = (sp, plan, xp)
    if key not in _solo:
        h = make(sp)
        chi2 = []
        for step in plan:
            if step == "reset":
                h.set_state(*start_state(sp))
            else:
                chi2.append(h.optimize(step)["chi2"])
        _solo[key] = record(h, chi2, xp)
        h.close()
    return _solo[key]


def oracle_chi2(sp, n):
    key = (sp[0], sp[1], n)
    if key not in _oracle:
        from oracle.oracle import OracleSolver
        o = OracleSolver(graph(sp[0]), RK_HUBER)
        if sp[1] is not None:
            o.set_state(*start_state(sp))
        _oracle[key] = o.optimize(n)["chi2"]
    return _oracle[key]


def kernel_class(cfg, Pf, scalar_size):
    """batch_kernel_class() of csrc/ba_pcg.hip: -1 = not batchable; else ((storage and Nc bucket) * 2 + (cl == 2)) * 2 + occupancy,
    with Nc = 6 cl nc, buckets 0 / 1 / 2 = fp32 storage of the coarse inverse with Nc <= 768 / <= 1536 / beyond, 3 / 4 = fp64 storage
    (always, in the fp32 library: the inverse is stored in the library's Scalar) with Nc <= 768 / beyond, and occupancy =
    spmv_wants_occupancy(): 2 Pf > 3 * 1024"""
    if cfg["agg"] <= 0 or cfg["upper"] or cfg["spmv_rows"] != 2:
        return -1
    Nc = 6 * cfg["cl"] * cfg["nc"]
    if cfg["coarse_fp32"] and scalar_size == 8:
        bucket = 0 if Nc <= 768 else 1 if Nc <= 1536 else 2
    else:
        bucket = 3 if Nc <= 768 else 4
    return ((bucket * 2 + (1 if cfg["cl"] == 2 else 0)) * 2) + (1 if 2 * Pf > 3 * 1024 else 0)


BUCKETS = ("f32:<=768", "f32:<=1536", "f32:>1536", "f64:<=768", "f64:>768")


def class_name(k):
    return "not batchable" if k < 0 else f"{BUCKETS[k // 4]}:cl{1 + (k // 2) % 2}" + (":occupancy" if k % 2 else "")


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def run_batch(label, specs, plan, path, xp=False, oracle=True, want_class=None):
    """the batch against its solo references.  path: "full" (the batch driver's full mode: every launch of a trial batched),
    "iterations" (the PCG iterations only), "fallback" (one handle after the other, batched == 0).  Returns what it ran."""
    hs = [make(sp) for sp in specs]
    cfgs = [h.pcg_config() for h in hs]
    classes = [kernel_class(c, graph(sp[0]).Pf, h.scalar_size) for c, sp, h in zip(cfgs, specs, hs)]
    for c in cfgs:
        assert c["spmv_rows"] == 2 and c["upper"] == 0, (label, c)
    if want_class is not None:
        assert [class_name(k) for k in classes] == [want_class] * len(hs), (label, [class_name(k) for k in classes])
    if path != "fallback":
        assert len(set(classes)) == 1 and classes[0] >= 0, (label, classes)
    chi2, batched = [], []
    for step in plan:
        if step == "reset":
            for h, sp in zip(hs, specs):
                h.set_state(*start_state(sp))
        else:
            got, b = optimize_batch(hs, step)
            chi2.append(got); batched.append(b)
    full, its = hs[0].counter("batch_full_trials"), hs[0].counter("batch_iteration_trials")
    print(f"\n[batch] {label}: n {len(hs)}, class {class_name(classes[0])}, path {path} (full trials {full}, iteration-only trials {its}, "
          f"batched solves {batched})")
    if path == "full":
        assert all(b > 0 for b in batched) and full > 0 and its == 0, (label, batched, full, its)
    elif path == "iterations":
        assert all(b > 0 for b in batched) and full == 0 and its > 0, (label, batched, full, its)
    else:
        assert all(b == 0 for b in batched) and full == 0 and its == 0, (label, batched, full, its)
    out = []
    for i, (h, sp, c) in enumerate(zip(hs, specs, cfgs)):
        want = solo(sp, plan, xp)
        got = record(h, [per_call[i] for per_call in chi2], xp)
        print(f"   [{i}] {sp[0]} Pf {graph(sp[0]).Pf} agg {c['agg']} cl {c['cl']} nc {c['nc']} Nc {6 * c['cl'] * c['nc']} coarse_fp32 {c['coarse_fp32']}: "
              f"iterations {[len(x) for x in got['chi2']]}, trials {got['trials']}, PCG iterations per solve {got['hist'].tolist()}")
        assert same(got["chi2"], want["chi2"]), (label, i, got["chi2"], want["chi2"])
        assert same(got["state"], want["state"]), (label, i, "state")
        assert got["trials"] == want["trials"] and np.array_equal(got["hist"], want["hist"]), (label, i, got["trials"], want["trials"], got["hist"], want["hist"])
        assert got["bad"] == want["bad"] and got["fallbacks"] == want["fallbacks"] and got["coarse_fp32"] == want["coarse_fp32"], (label, i)
        if xp:
            assert np.array_equal(got["xp"], want["xp"]), (label, i, "xp")
        if oracle and sp[2] == "f64" and isinstance(plan[0], int) and "pcg_tol" not in dict(sp[3]):
            ref = oracle_chi2(sp, plan[0])
            assert len(got["chi2"][0]) == len(ref) and np.all(np.abs(got["chi2"][0] - ref) <= CHI2_TOL * ref), (label, i, got["chi2"][0], ref)
        out.append(got)
        h.close()
    return out, cfgs


# ---- 1. every class, both lead orders ------------------------------------------------------------------------------------------
# class: (options, graphs in ascending size).  nc = ceil(Pf / agg), Nc = 6 cl nc: small 39 free poses, mid 299, g450 449, g515 514, g600 599.
F64 = dict(precond_fp32=0)
CLASSES = {
    "f32:<=768:cl2": ("f64", dict(pcg_aggregate=8), ("small", "mid", "g450")),                      # Nc 60, 456, 684
    "f32:<=768:cl1": ("f64", dict(pcg_aggregate=4, coarse_linear=0), ("small", "mid", "g450")),     # Nc 60, 450, 678
    "f32:<=1536:cl2": ("f64", dict(pcg_aggregate=4), ("mid", "g450")),                              # Nc 900, 1356
    "f32:<=1536:cl1": ("f64", dict(pcg_aggregate=2, coarse_linear=0), ("mid", "g450")),             # Nc 900, 1350
    "f32:>1536:cl2": ("f64", dict(pcg_aggregate=2), ("mid", "g450")),                               # Nc 1800, 2700 (beyond the 2304 columns held in registers)
    "f32:>1536:cl1": ("f64", dict(pcg_aggregate=2, coarse_linear=0), ("g515", "g600")),             # Nc 1542, 1800: nc 257 is the smallest with Nc > 1536
    "f64:<=768:cl2": ("f64", dict(pcg_aggregate=8, **F64), ("small", "mid", "g450")),
    "f64:<=768:cl1": ("f64", dict(pcg_aggregate=4, coarse_linear=0, **F64), ("small", "mid", "g450")),
    "f64:>768:cl2": ("f64", dict(pcg_aggregate=4, **F64), ("mid", "g450")),
    "f64:>768:cl1": ("f64", dict(pcg_aggregate=2, coarse_linear=0, **F64), ("mid", "g450")),
    "f32lib:<=768:cl2": ("f32", dict(pcg_aggregate=8), ("small", "mid", "g450")),
    "f32lib:<=768:cl1": ("f32", dict(pcg_aggregate=4, coarse_linear=0), ("small", "mid", "g450")),
    "f32lib:>768:cl2": ("f32", dict(pcg_aggregate=4), ("mid", "g450")),
    "f32lib:>768:cl1": ("f32", dict(pcg_aggregate=2, coarse_linear=0), ("mid", "g450")),
}


@pytest.mark.parametrize("lead", ["smallest_first", "largest_first"])
@pytest.mark.parametrize("name", list(CLASSES))
def test_every_class_with_either_lead(name, lead):
    """each pcg2_fused_batch_kernel<CL, AC, AC2, W> instantiation of both libraries, on graphs of different nc, Pf, landmark count and
    LDS bytes.  Smallest first: every launch maximum (gridSpmvMax, ncMax, ldsMax, lmMax, schurMax, setupMax, tailMax, restoreMax, the
    sweep's nMax) comes from another graph than the one the kernel is chosen from, the lead's surplus workgroups return early and its LDS
    layout sits in a larger allocation"""
    precision, opts, graphs = CLASSES[name]
    specs = [spec(g, precision=precision, **opts) for g in graphs]
    if lead == "largest_first":
        specs = specs[::-1]
    want = name.replace("f32lib", "f64")          # (the fp32 library stores the inverse in its own Scalar: the W = 2 instantiations)
    got, cfgs = run_batch(f"{name} {lead}", specs, (4,), "full", want_class=want)
    assert len({c["nc"] for c in cfgs}) == len(cfgs)          # the graphs differ in their coarse dimension
    assert all(len(r["chi2"][0]) == 4 for r in got)


# ---- 2. the SpMV instantiation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 6])
def test_spmv_instantiation_by_batch_size(n):
    """launch_pcg_batch_iteration (csrc/ba_pcg.hip) takes pcg_spmv_batch_kernel<2, 4> -- an instantiation no solo run can select -- when
    2 * gridSpmvMax * n * 2 > 3 * 1024, i.e. gridSpmvMax * n > 768, and <2, 1> otherwise; same source, same bits.  "mid" has 150 SpMV
    workgroups: 5 handles stay below, 6 go beyond"""
    specs = [spec("mid", start=s) for s in range(n)]
    got, cfgs = run_batch(f"spmv instantiation, n = {n}", specs, (4,), "full", want_class="f32:<=768:cl2")
    grid = max((graph("mid").Pf + c["spmv_rows"] - 1) // c["spmv_rows"] for c in cfgs)
    assert grid == 150 and (grid * n > 768) == (n == 6), (grid, n)
    assert len({tuple(r["hist"]) for r in got}) > 1           # the starts differ: so do the solves


# ---- 3. iterates inside a batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(pcg_aggregate=2, precond_fp32=0)], ids=["default", "f64_gt768"])
def test_iterates_with_per_graph_iteration_limits(opts):
    """pcg_max_iter 1, 4, 5 and 17 side by side, the best iterate accepted, a tolerance that never fires: xp after one LM iteration is the
    K-th iterate of each graph's own solve.  K = 1 pins the batched first preconditioner application, 4 / 5 straddle a chunk, and the
    mixed limits pin that maxIter comes from the graph's own table entry (the batch enqueues 17 iterations for all four)"""
    specs = [spec("mid", start=i, pcg_max_iter=K, pcg_accept_unconverged=1, direct_fallback=0, pcg_tol=NEVER, **opts) for i, K in enumerate((1, 4, 5, 17))]
    got, _ = run_batch("iterates K = 1 / 4 / 5 / 17", specs, (1,), "full", xp=True, oracle=False)
    for r, K in zip(got, (1, 4, 5, 17)):
        # every solve stopped at ITS limit, and is reported as such (negative) although the batch enqueued 17 iterations for each graph
        assert np.all(r["hist"] == -K) and r["bad"] == len(r["hist"]), (K, r["hist"], r["bad"])
    assert not any(np.array_equal(got[0]["xp"], r["xp"]) for r in got[1:])


# ---- 4. mixed precision --------------------------------------------------------------------------------------------------------
def test_mixed_precision_handles_take_the_full_path():
    """lm_pass_batch_kernel<float> and schur_pass_batch_kernel<float>"""
    run_batch("mixed_precision = 1 everywhere", [spec(g, mixed_precision=1) for g in ("small", "g450", "mid")], (4,), "full")


@pytest.mark.parametrize("order", [0, 1])
def test_mixed_and_plain_handles_take_the_iterations_only_path(order):
    specs = [spec("mid", mixed_precision=1), spec("small")]
    run_batch("mixed_precision differs", specs[::-1] if order else specs, (4,), "iterations")


# ---- 5. a run that ends inside the batch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", [0, 1, 2])
def test_a_run_that_ends_early_leaves_the_batch(position):
    """one handle starts at the end state of a converged OracleSolver run on an outlier-free graph: its run ends at once (ten rejected
    trials, or rho <= 0) while the others go on, `act` shrinks, and entry a of the device table is handle act[a] != a.  First, in the
    middle, last: the indices part ways in three ways.  (The oracle comparison of that handle covers the iterations both runs have: at a
    minimum held to rounding level the sign of a chi2 difference, which ends the run, depends on the summation order.)"""
    n_it = 6
    early = spec("clean", start="converged")
    ref = oracle_chi2(early, n_it)
    assert len(ref) < n_it, ref                                  # the oracle alone: this run is shorter than the call asks for
    others = [spec("mid"), spec("g450")]
    specs = others[:position] + [early] + others[position:]
    got, _ = run_batch(f"early end at position {position}", specs, (n_it,), "full", oracle=False)
    for sp, r in zip(specs, got):
        if sp == early:
            assert len(r["chi2"][0]) < n_it, r["chi2"]
            m = min(len(ref), len(r["chi2"][0]))
            assert m > 0 and np.all(np.abs(r["chi2"][0][:m] - ref[:m]) <= CHI2_TOL * ref[:m])
        else:
            o = oracle_chi2(sp, n_it)
            assert len(r["chi2"][0]) == n_it == len(o) and np.all(np.abs(r["chi2"][0] - o) <= CHI2_TOL * o)


# ---- 6. failing reduced solves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("position", [0, 1])
def test_failing_reduced_solves_inside_a_batch(position):
    """a handle whose solves stop at pcg_max_iter = 1 without the exact fallback and without pcg_accept_unconverged: a failed solve is
    launch_lm_decide_failed followed by the batched tail with tailGrid = 0 and reportOn = 0; the trial is rejected, the damping raised,
    and after maxq = 10 rejections the run halts: one iteration, ten trials, nothing moved.  (The batch enqueues the iterations its other
    graphs need for this graph too: a solve that stopped at its limit must still be reported as failed.)  Beside plain handles, each as
    alone -- the failing handle's unchanged estimates and its trial count included"""
    failing = spec("mid", start=3, pcg_max_iter=1, direct_fallback=0)
    others = [spec("small"), spec("g450")]
    specs = others[:position] + [failing] + others[position:]
    got, _ = run_batch(f"failing solves at position {position}", specs, (3,), "full", oracle=False)
    for sp, r in zip(specs, got):
        if sp == failing:
            print(f"   failing handle: history {r['hist'].tolist()}, unconverged {r['bad']}, trials {r['trials']}, iterations {len(r['chi2'][0])}")
            assert np.array_equal(r["hist"], [-1] * 10) and r["bad"] == 10 == r["trials"] and len(r["chi2"][0]) == 1
            h = make(sp)
            assert same(r["state"], h.state())                                      # every solve failed: nothing moved
            h.close()
        else:
            o = oracle_chi2(sp, 3)
            assert len(r["chi2"][0]) == len(o) and np.all(np.abs(r["chi2"][0] - o) <= CHI2_TOL * o)


# ---- 7. the limits of the call -------------------------------------------------------------------------------------------------
def test_sixty_four_handles_batch():
    """CUBA_HIP_BATCH_MAX = 64 graphs in one call: three distinct starts, one solo run per start"""
    specs = [spec("small", start=i % 3) for i in range(64)]
    run_batch("64 handles", specs, (3,), "full")


def test_sixty_five_handles_are_refused():
    hs = [make(spec("small", start=i % 3)) for i in range(65)]
    with pytest.raises(CubaHipError, match="status 1"):         # CUBA_HIP_ERR_INVALID_ARGUMENT
        optimize_batch(hs, 3)
    for i in (0, 33, 64):                                        # ... and every handle is as it was
        want = solo(spec("small", start=i % 3), (3,))
        assert same([hs[i].optimize(3)["chi2"]], want["chi2"]) and same(hs[i].state(), want["state"])
    for h in hs:
        h.close()


def test_calls_that_fall_back_to_one_handle_after_the_other():
    run_batch("n = 1", [spec("small")], (3,), "fallback")
    run_batch("two pcg_tol", [spec("mid", pcg_tol=1e-8), spec("small", pcg_tol=1e-9)], (3,), "fallback")
    # one handle twice: the documented contract is `distinct` handles -- refused, handle intact
    h = make(spec("small"))
    with pytest.raises(CubaHipError, match="status 1"):
        optimize_batch([h, h], 3)
    want = solo(spec("small"), (3,))
    assert same([h.optimize(3)["chi2"]], want["chi2"]) and same(h.state(), want["state"])
    h.close()


# ---- 8. the second call --------------------------------------------------------------------------------------------------------
def test_second_call_on_the_same_handles_is_bitwise_the_solo_second_run():
    """optimize_batch, set_state, optimize_batch against optimize, set_state, optimize: the second run's first solve starts with the coarse
    inverse the first run's first trial left -- the same data on both sides"""
    run_batch("second call", [spec("small"), spec("mid"), spec("g450", start=1)], (4, "reset", 4), "full", oracle=False)


# ---- 9. fixed vertices, internal renumbering -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
def test_fixed_vertices_and_internal_renumbering(order):
    """fixed poses inside the trajectory (Pf < Pt) and shuffled pose ids (the library renumbers the free poses and the landmarks
    internally: default pose_reorder and landmark_reorder) in one batch"""
    specs = [spec("fixed"), spec("shuffled")]
    hs = make(specs[1])
    assert not np.array_equal(hs.pcg_config()["pose_order"], np.arange(graph("shuffled").Pf)), "the internal renumbering is not active"
    hs.close()
    assert graph("fixed").Pf < graph("fixed").Pt - 1
    run_batch("fixed + shuffled", specs[::-1] if order else specs, (4,), "full")


# ---- 10. a handle that leaves its class in the middle of the call --------------------------------------------------------------
# the gauge-free monocular graph of test_fp32_coarse_inverse_falls_back_when_the_pcg_breaks_down (tests/test_gpu_parity.py) without robust
# kernels: LM runs whose PCG breaks down with the fp32-stored coarse inverse around trial 31 (the solo path, which handles that, reports
# "precond_fp32_fallbacks").  kept: without the exact solver the repeat with fp64 storage converges and the handle keeps fp64 storage
# for the rest of its run -- some 27 further trials in another kernel class than its neighbours.  restored: with pcg_aggregate = 8 and
# the exact solver the repeat breaks down too, the handle takes its fp32 copy back and goes on with exact solves.
CLASS_CHANGE = {"kept": (dict(direct_fallback=0), {}), "restored": (dict(pcg_aggregate=8), dict(pcg_aggregate=8))}


@pytest.mark.parametrize("position", [0, 1, 2])
@pytest.mark.parametrize("variant", list(CLASS_CHANGE))
def test_a_handle_that_leaves_its_class_solves_alone(variant, position):
    """retryWithFp64Inverse (csrc/ba_lm.hip) sets sys.acinv32 = nullptr for the rest of the run: the handle is then of an fp64-storage
    class and must not sit in the others' W = 4 launches (nor they in its W = 2 ones).  The batch driver checks the class before every
    trial's solves, lets such a handle solve alone, and chooses the kernels from the first graph still in the PCG -- position 0 is the
    lead itself changing class"""
    n_it = 40
    opts, other_opts = CLASS_CHANGE[variant]
    fb = spec("gaugefree", robust_none=1, **opts)
    want = solo(fb, (n_it,))
    assert want["fallbacks"] >= 1 and want["coarse_fp32"] == (0 if variant == "kept" else 1), (want["fallbacks"], want["coarse_fp32"])
    if variant == "kept":
        assert np.all(want["hist"][-20:] > 0)                      # ... and it went on solving by PCG, in the fp64-storage class
    others = [spec("small", **other_opts), spec("mid", **other_opts)]
    specs = others[:position] + [fb] + others[position:]
    got, _ = run_batch(f"class change ({variant}), position {position}", specs, (n_it,), "full", oracle=False, want_class="f32:<=768:cl2")
    assert got[position]["fallbacks"] == want["fallbacks"]


def class_change_iterations_only(position):
    """the "kept" handle beside a plain and a mixed-precision one: the batch that keeps everything but the PCG iterations per stream"""
    fb = spec("gaugefree", robust_none=1, direct_fallback=0)
    others = [spec("small"), spec("mid", mixed_precision=1)]
    return fb, others[:position] + [fb] + others[position:]


@pytest.mark.parametrize("position", [0, 1])
def test_a_handle_that_leaves_its_class_solves_alone_on_the_iterations_only_path(position):
    """the same with the trial's other launches on the handles' own streams: the handle that left the class solves alone on ITS stream,
    is no entry of the compact table, and the join / fork events go round it"""
    n_it = 40
    fb, specs = class_change_iterations_only(position)
    want = solo(fb, (n_it,))
    assert want["fallbacks"] >= 1 and want["coarse_fp32"] == 0, (want["fallbacks"], want["coarse_fp32"])
    got, _ = run_batch(f"class change (kept), iterations only, position {position}", specs, (n_it,), "iterations", oracle=False, want_class="f32:<=768:cl2")
    assert got[position]["fallbacks"] == want["fallbacks"]

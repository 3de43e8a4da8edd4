"""The scripts of the handle-life tests: lists of steps (tests/handle_life_model.py) that one solver handle lives through -- TEST
INFRASTRUCTURE.  tests/test_handle_life_model.py runs them dry (rules, transition coverage, the fp64 reference of every checkpoint);
tests/test_gpu_handle_life.py runs them on a live handle and compares it with a fresh twin at every Check.

Every Check needs estimates the model knows, so a script names them (an upload, SetState, a restore) after every run.  Graphs come from
synth_ba at the smallest sizes that still switch the code path; factor graphs stay at 40 poses (the dense reference)."""
import copy
import functools

import numpy as np

import direction_factor_reference as dr
import edge_gate_reference as eg
import landmark_prior_reference as lr
import pose_range_factor_reference as pp
import position_factor_reference as pfr
import range_factor_reference as rr
import robust_pose_factor_reference as rb
from conftest import RK_HUBER, RK_TUKEY, with_fixed
from handle_life_model import (ERR_ARGUMENT, ERR_STATE, Check, Covariance, ExpectPoseOrder, Gate, Hint, Optimize, Refused, Restore, SetFactors,
                               SetMask, SetOption, SetPartition, SetPoseFactorKernels, SetRobustKernel, SetState, Snapshot, Stages, Upload, Push, Pop, Batch)  # noqa: F401

from cuba_amd.graph import flatten
from cuba_amd.synth import synth_ba

# the graph of the "orders" script: the smallest of the sizes 49, 50, 56, 64, 80, 100, 150, 200 (40 landmarks and 160 edges a pose) for
# which the library reports a non-identity internal pose order for shuffled pose ids -- up to 80 poses it keeps the caller's (the script
# asserts the fact from the hook at run time)
ORDER_GRAPH = dict(P=100, L=4000, E=16000, seed=13)


@functools.lru_cache(maxsize=None)
def graph(name):
    from test_gpu_configs import graph_with_duplicate_observations, shuffled_pose_ids
    if name == "w40": return synth_ba(40, 600, 2400, seed=1)
    if name == "w12": return synth_ba(12, 96, 400, seed=1)
    if name == "w150": return synth_ba(150, 2400, 9600, seed=7)
    if name == "ordered": return synth_ba(**ORDER_GRAPH)
    if name == "shuffled": return shuffled_pose_ids(graph("ordered"), seed=2)
    if name == "big":
        from test_gpu_parity import graph_with_big_landmarks
        return graph_with_big_landmarks()[0]
    if name == "duplicates": return graph_with_duplicate_observations()
    if name == "pose_only":
        g = graph("w40"); return with_fixed(g, (), range(len(g.lm_ids)))
    if name == "landmark_only":
        g = graph("w40"); return with_fixed(g, range(len(g.pose_ids)), ())
    if name == "mono": return synth_ba(40, 600, 2400, seed=5, stereo_frac=0.0)
    if name == "stereo": return synth_ba(40, 600, 2400, seed=6, stereo_frac=1.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def problem(name):
    fp = flatten(graph(name))
    fp.shuffled = name == "shuffled"
    return fp


def start(fp):
    """SetState with the uploaded estimates: the estimates are known again"""
    return SetState((fp.q, fp.t, fp.Xw))


def other_edges(fp, seed, n=6):
    """the same five counts, other index arrays: n edges observe the nearest landmark their pose does not see yet instead of their own
    (which keeps at least two edges); the measurement stays, so the edge becomes one more outlier of a graph that has 3 % of them"""
    rng = np.random.default_rng(seed)
    out = copy.copy(fp)
    out.eL = fp.eL.copy()
    seen = set(zip(fp.eP.tolist(), fp.eL.tolist()))
    per_lm = np.bincount(fp.eL, minlength=fp.Lt)
    done = 0
    for e in rng.permutation(fp.E):
        p, l = int(fp.eP[e]), int(fp.eL[e])
        if per_lm[l] <= 3 or l >= fp.Lf:
            continue
        for l2 in np.argsort(((fp.Xw[:fp.Lf] - fp.Xw[l]) ** 2).sum(1))[1:6]:
            if (p, int(l2)) not in seen:
                out.eL[e] = l2; seen.add((p, int(l2))); per_lm[l] -= 1; per_lm[l2] += 1; done += 1
                break
        if done == n:
            break
    assert done == n and not np.array_equal(out.eL, fp.eL)
    return out


def other_values(fp, seed):
    """the same index arrays, other measurements and landmark estimates"""
    rng = np.random.default_rng(seed)
    out = copy.copy(fp)
    out.Xw = fp.Xw + rng.normal(0, 0.02, fp.Xw.shape)
    out.meas = fp.meas + rng.normal(0, 0.3, fp.meas.shape) * (np.arange(3)[None, :] < fp.eDim[:, None])
    return out


def broken(fp, how):
    out = copy.copy(fp)
    if how == "counts":
        out.Pf = fp.Pt + 1
    elif how == "edge_index":                 # one edge fewer (so no promise covers the arrays) and one pose index out of range
        for name in ("eP", "eL", "eDim", "omega", "meas", "edge_src"):
            setattr(out, name, getattr(fp, name)[:-1].copy())
        out.eP[3] = fp.Pt + 5
    return out


# ---- windows ------------------------------------------------------------------------------------------------------------------------
def windows():
    A, B, C = problem("w40"), problem("w12"), problem("w150")
    A2 = other_edges(A, 1)
    A2v = other_values(A2, 2)
    return [
        Upload(A), Check(3),
        Upload(B, "two"), Check(2),                                            # shrinks
        Upload(C), Check(3),                                                   # grows past the first capacity
        Upload(A, "two"), Optimize(2),                                         # returns to the first size
        Upload(A), Check(3),                                                   # identical, found by comparison
        Upload(eg.with_state(A, (A.q, A.t, A.Xw + 0.01)), "two"), Check(2),    # ... but for the estimates
        Hint(True, False), Upload(A, "two"), Optimize(2),
        Hint(True, True), Upload(A), Check(3),
        Upload(A2), Check(3),                                                  # same counts, other edges
        Upload(A2v, "two"), Check(3),                                          # same edges, other values
        Hint(True, False), Upload(other_values(A2, 9)), Check(2),              # ... under a promise of the edges alone
        Upload(A, "begin"), Hint(True, True), Upload(A), Check(2),             # a begin without its end, then a promise of its values
    ]


def windows_refusals():
    """a promise followed by a refused upload followed by a valid upload of other edges with the same counts: the promise must be gone;
    a begin without its end followed by a refused upload: the begun graph stays in force, with the values that were on their way"""
    A = problem("w40")
    A2, A3 = other_edges(A, 1), other_edges(A, 3)
    return [
        Upload(A), Optimize(2), Snapshot(2),
        Hint(True, True), Refused(Upload(broken(A, "counts")), ERR_ARGUMENT), Restore(2), Upload(A2), Check(3),
        Hint(True, False), Refused(Upload(A, "ranged", (5, A.Lt + 3)), ERR_ARGUMENT), Upload(A3, "two"), Check(3),
        Hint(True, True), Refused(Upload(broken(A3, "edge_index")), ERR_ARGUMENT), Upload(A), Check(2),
        Refused(Upload(broken(A, "edge_index")), ERR_ARGUMENT), start(A), Check(2),          # no promise: the graph in force stays
        Upload(other_values(A, 11), "begin"), Refused(Upload(broken(A, "counts")), ERR_ARGUMENT), Check(2),          # ... a begun one too
    ]


# ---- orders -------------------------------------------------------------------------------------------------------------------------
def orders():
    O, S = problem("ordered"), problem("shuffled")
    return [
        Upload(O), Snapshot(0), Optimize(1), Restore(0), Check(2), ExpectPoseOrder(True),
        Snapshot(0), Upload(S), Refused(Restore(0), ERR_STATE), Check(2), ExpectPoseOrder(False),
        Snapshot(0), Upload(S), Refused(Restore(0), ERR_STATE), Check(2), ExpectPoseOrder(False),          # the order is kept
        # ("device_setup" on a handle that holds a graph: the analysis follows at once, the edge sort with the next upload -- the run between
        # the two is compared once the upload has brought the handle to what a fresh one does)
        start(S), Snapshot(1), SetOption("device_setup", 0), Optimize(1), Restore(1, may_be_dropped=True), Upload(S), Check(2),
        start(S), Snapshot(1), SetOption("device_setup", 1), Optimize(1), Restore(1, may_be_dropped=True), Upload(S, "two"), Check(2),
        Snapshot(0), Upload(O, "two"), Refused(Restore(0), ERR_STATE), Check(2), ExpectPoseOrder(True),
    ]


def reorder_options():
    """landmark_reorder "takes effect with the next cuba_hip_set_graph": 0 and 1, each followed by an identical upload and by another
    one; pose_reorder 0 and 1 on the shuffled graph"""
    O, S = problem("ordered"), problem("shuffled")
    O2, O3 = other_edges(O, 4), other_edges(O, 5)
    return [
        Upload(O), Optimize(1),
        SetOption("landmark_reorder", 0), Upload(O), Check(2),
        SetOption("landmark_reorder", 1), Upload(O, "two"), Check(2),
        SetOption("landmark_reorder", 0), Upload(O2), Check(2),
        SetOption("landmark_reorder", 1), Upload(O3), Check(2),
        Upload(S), Optimize(1), ExpectPoseOrder(False),
        # ("pose_reorder", like "device_setup" in the orders script: a run under the new value, then the upload with which it takes effect)
        SetOption("pose_reorder", 0), start(S), Optimize(1), Upload(S), Check(2), ExpectPoseOrder(True),
        Upload(S, "two"), Check(2), ExpectPoseOrder(True),
        SetOption("pose_reorder", 1), start(S), Optimize(1), Upload(S), Check(2), ExpectPoseOrder(False),
        Upload(S), Check(2), ExpectPoseOrder(False),
    ]


# ---- options ------------------------------------------------------------------------------------------------------------------------
def _there_and_back(fp, key, second, first, run=None):
    """the key to a second value, a run, back to the first one, a run"""
    return [SetOption(key, second), start(fp), run or Check(2), SetOption(key, first), start(fp), Check(2)]


def options_pcg(size, precision="f64"):
    fp = problem(size)
    s = [Upload(fp), Check(3)]
    tol = (1e-9, 1e-7) if precision == "f64" else (1e-5, 1e-4)          # (a tighter one, the library's default)
    for key, second, first in (("pcg_aggregate", 6, -1), ("coarse_linear", 0, 1), ("precond_fp32", 0, 1 if precision == "f64" else 0),
                               ("spmv_upper", 0, -1), ("spmv_upper", 1, -1), ("pcg_max_iter", 500, 0), ("reduction_chunks", 4, 0),
                               ("pcg_tol",) + tol):
        s += _there_and_back(fp, key, second, first)
    return s


def options_solver(size):
    fp = problem(size)
    s = [Upload(fp), Check(3)]
    s += _there_and_back(fp, "mixed_precision", 1, 0, Check(2, reference=False))
    s += _there_and_back(fp, "profile", 1, 0)                                   # host loop <-> device chain
    s += [SetOption("reduced_solver", 1), start(fp), Check(2),                  # two exact solves with another slack between them
          SetOption("direct_slack", 2), start(fp), Check(2),
          SetOption("direct_slack", -1), start(fp), Check(2),
          SetOption("direct_max_tiles", 1), start(fp), Optimize(2),             # the plan is refused: whatever the run does, the next is the twin's
          SetOption("direct_max_tiles", 1 << 20), start(fp), Check(2),
          SetOption("reduced_solver", 0), start(fp), Check(2)]
    s += _there_and_back(fp, "direct_fallback", 0, 1)
    return s


def options_graphs():
    """captured PCG graphs: kept by an identical upload, dropped when the buffers moved; robust kernels between runs"""
    A, C = problem("w40"), problem("w150")
    return [
        Upload(A), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]), Check(2),
        SetOption("pcg_graph", 1), start(A), Optimize(3), start(A), Check(3),
        Upload(A), Check(3),                                                   # identical upload: the graphs are kept
        Upload(C), Check(2), Upload(A), Check(3),                              # the buffers moved
        SetOption("pcg_graph", 0), start(A), Check(2),
        SetRobustKernel(0, *RK_TUKEY[0]), SetRobustKernel(1, *RK_TUKEY[1]), start(A), Check(2),
        SetRobustKernel(0, 0, 0.0), SetRobustKernel(1, 0, 0.0), start(A), Check(2),
    ]


# ---- factors ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def factor_sets(which):
    """two sets of other lengths per kind on the 40-pose graph, made with the kinds' own make_* helpers"""
    from test_gpu_pose_priors import make_priors as make_pose_priors
    from test_gpu_relative_pose import make_rel
    fp = problem("w40")
    a = dict(pose_priors=make_pose_priors(fp, [1, 5, 17], seed=1),
             relative_pose_edges=make_rel(fp, [(3, 20), (9, 3)], seed=2),
             landmark_priors=lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0),
             position_factors=pfr.make_factors(fp, [5, 8, 22], seed=4, kind=rb.HUBER, delta=2.0),
             direction_factors=dr.make_factors(fp, [5, 9, 30], seed=5, kind=rb.HUBER, delta=2.0),
             range_factors=rr.make_factors(fp, [5, 3, 12], seed=6, kind=rb.HUBER, delta=2.0),
             pose_range_factors=pp.make_factors(fp, [(2, 30), (7, 25), (11, 12)], seed=7, kind=rb.CAUCHY, delta=2.0))
    b = dict(pose_priors=make_pose_priors(fp, [2, 6, 18, 30, 31], seed=11),
             relative_pose_edges=make_rel(fp, [(4, 28), (10, 4), (15, 33)], seed=12),
             landmark_priors=lr.make_priors(fp, [7, 50], seed=13),
             position_factors=pfr.make_factors(fp, [1, 2, 3, 4, 30], seed=14),
             direction_factors=dr.make_factors(fp, [6, 10], seed=15),
             range_factors=rr.make_factors(fp, [8, 9, 13, 14, 20], seed=16),
             pose_range_factors=pp.make_factors(fp, [(2, 30), (6, 21)], seed=17))
    return dict(a=a, b=b)[which]


def _factor_cycle(kinds):
    fp = problem("w40")
    a, b = factor_sets("a"), factor_sets("b")
    s = [Upload(fp), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]), Optimize(1)]
    for k in kinds:
        s += [SetFactors(k, a[k]), start(fp), Check(2), SetFactors(k, b[k]), start(fp), Check(2), SetFactors(k, None)]
    return s + [start(fp), Check(2)]


def factors_unary():
    return _factor_cycle(("pose_priors", "landmark_priors", "position_factors", "direction_factors", "range_factors"))


def factors_binary():
    fp = problem("w40")
    a = factor_sets("a")
    n = len(a["relative_pose_edges"][0])
    return _factor_cycle(("relative_pose_edges", "pose_range_factors"))[:-2] + [
        SetFactors("pose_priors", a["pose_priors"]), SetFactors("relative_pose_edges", a["relative_pose_edges"]),
        SetPoseFactorKernels(0, np.full(3, rb.HUBER), np.full(3, 2.0)), SetPoseFactorKernels(1, np.full(n, rb.CAUCHY), np.full(n, 1.5)),
        start(fp), Check(2),
        SetPoseFactorKernels(1, None), start(fp), Check(2),
        SetFactors("pose_priors", factor_sets("b")["pose_priors"]), start(fp), Check(2),          # the replaced set is a new set: no kernels
    ]


def factors_all():
    """all seven at once, then an identical upload under a promise: the factors are gone, the mask remains"""
    fp = problem("w40")
    a = factor_sets("a")
    mask = eg.mask_keeping_two_per_landmark(fp, np.random.default_rng(3))
    s = [Upload(fp), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1])]
    s += [SetFactors(k, a[k]) for k in a]
    s += [Check(3), SetMask(mask), start(fp), Check(2),
          Hint(True, True), Upload(fp), Check(2),
          Refused(SetFactors("pose_priors", ([fp.Pt + 2],) + tuple(a["pose_priors"][1:][i][:1] for i in range(3))), ERR_ARGUMENT),
          SetFactors("pose_range_factors", a["pose_range_factors"]),
          Refused(Upload(broken(fp, "edge_index")), ERR_ARGUMENT), start(fp), Check(2)]          # a refused upload keeps factors and mask
    return s


def factors_pairs():
    """the binary kinds' union of pairs changes while a mask is set and after an exact solve and a covariance have built their plans"""
    fp, B = problem("w40"), problem("w12")
    a, b = factor_sets("a"), factor_sets("b")
    mask = eg.mask_keeping_two_per_landmark(fp, np.random.default_rng(4))
    pairs = (("pose", 3, "pose", 20), ("pose", 4, "landmark", 10))
    return [
        Upload(fp), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]),
        SetFactors("relative_pose_edges", a["relative_pose_edges"]), SetMask(mask), SetOption("reduced_solver", 1),
        Check(2, covariance_pairs=pairs), start(fp), Covariance(pairs),
        SetFactors("pose_range_factors", a["pose_range_factors"]), Check(2, covariance_pairs=pairs),          # the union grows
        SetFactors("relative_pose_edges", b["relative_pose_edges"]), start(fp), Check(2, covariance_pairs=pairs),          # ... changes
        SetFactors("relative_pose_edges", None), SetFactors("pose_range_factors", None), start(fp), Check(2),          # ... empties
        SetOption("reduced_solver", 0), Upload(B), Optimize(1), Upload(fp),
        SetFactors("pose_range_factors", b["pose_range_factors"]), SetFactors("range_factors", b["range_factors"]), Check(2),          # after a resize
    ]


# ---- gate ---------------------------------------------------------------------------------------------------------------------------
GATE = (400.0, 520.0)          # thresholds that switch the gross outliers of the 40-pose graph off and leave every landmark two edges


@functools.lru_cache(maxsize=None)
def settled():
    """the 40-pose graph's estimates after four iterations of the fp64 reference: where a caller gates (ORB-SLAM: optimize, gate, optimize)"""
    from oracle.oracle import OracleSolver
    o = OracleSolver(problem("w40"), RK_HUBER)
    o.optimize(4)
    return SetState(tuple(np.array(a) for a in o.state()))


def gate():
    A = problem("w40")
    Av, A2 = other_values(A, 6), other_edges(A, 7)
    return [
        Upload(A), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]),
        settled(), Gate(GATE), Check(3),
        Upload(A), Check(2),                                                   # identical: the mask stays
        Upload(Av, "two"), settled(), Gate(GATE, mode="dry_run"), Check(2),    # new values, same edges: it stays, rebuilt from the new information
        settled(), Gate(GATE, mode="only_remove"), Check(2),
        Upload(A2), Check(2),                                                  # other edges: gone
        settled(), Gate(GATE), Upload(A, "two"), Check(2),                     # ... and a mask set on them goes with them
    ]


def gate_big_landmark():
    """half of a landmark with more than 64 observations gated, then ungated"""
    fp = problem("big")
    per_lm = np.bincount(fp.eL, minlength=fp.Lt)
    l = int(np.argmax(per_lm))
    assert per_lm[l] > 64
    mask = np.ones(fp.E, bool)
    mask[np.nonzero(fp.eL == l)[0][::2]] = False
    return [Upload(fp), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]), Check(2),
            SetMask(mask), start(fp), Check(2), SetMask(None), start(fp), Check(2)]


# ---- classes ------------------------------------------------------------------------------------------------------------------------
def classes():
    s = [SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1])]
    for k, name in enumerate(("w40", "big", "duplicates", "pose_only", "landmark_only", "mono", "stereo", "w40")):
        s += [Upload(problem(name), "two" if k % 2 else "one"), Check(2)]
    return s


# ---- partition ----------------------------------------------------------------------------------------------------------------------
def partition():
    A = problem("w40")
    Av = other_values(A, 8)
    half = (0, A.Lt // 2)
    a = factor_sets("a")
    return [
        Upload(A), SetPartition(*half), Check(0),
        Refused(SetFactors("pose_priors", a["pose_priors"]), ERR_STATE),
        SetPartition(0, -1), start(A), Check(2),
        SetFactors("pose_priors", a["pose_priors"]), start(A), Check(2),
        Upload(A, "ranged", half), Check(0),
        Upload(A), Check(2),                                                   # whole again, no promise
        Upload(A, "ranged", half), Hint(True, True), Upload(A, "two"), Check(2),          # whole again under a promise: the device held half the values
        Hint(True, True), Upload(Av, "ranged", half), Check(0),                # a ranged upload ignores the (wrong) promise of values
        Upload(Av), Check(2),
        SetPartition(*half), Upload(Av), Check(2),                             # a whole upload lifts a partition that was set
    ]


# ---- failures -----------------------------------------------------------------------------------------------------------------------
def failures():
    A = problem("w40")
    return [
        Upload(A), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]), Check(2),
        SetOption("pcg_max_iter", 1), SetOption("direct_fallback", 0), start(A), Optimize(3),          # every solve fails
        SetOption("pcg_max_iter", 0), SetOption("direct_fallback", 1), start(A), Check(3),
        Refused(SetOption("reduced_solver", 2), ERR_ARGUMENT), Refused(SetOption("no_such_option", 1), ERR_ARGUMENT), start(A), Check(2),
        Refused(Restore(5), ERR_STATE), start(A), Check(2),
        start(A), Optimize(0), Check(2),
        start(A), Push(), Stages(), Pop(), Check(2),
    ]


# ---- covariance ---------------------------------------------------------------------------------------------------------------------
def covariance():
    A, C = problem("w40"), problem("w150")
    pa = (("pose", 3, "pose", 20), ("pose", 4, "landmark", 10), ("landmark", 5, "landmark", 300))
    pc = (("pose", 100, "pose", 2), ("landmark", 1500, "pose", 140))
    mask = eg.mask_keeping_two_per_landmark(A, np.random.default_rng(9))
    return [
        Upload(A), SetRobustKernel(0, *RK_HUBER[0]), SetRobustKernel(1, *RK_HUBER[1]),
        Covariance(pa), Check(2, covariance_pairs=pa),
        Upload(C), Covariance(pc), Check(2, covariance_pairs=pc),                          # a window of another size, then again
        Upload(A), Covariance(pa), SetOption("reduced_solver", 1), Covariance(pa), Check(2, covariance_pairs=pa),
        start(A), Covariance(pa), SetOption("direct_slack", 2), Covariance(pa), Check(2, covariance_pairs=pa),
        SetOption("reduced_solver", 0), SetOption("direct_slack", -1),
        start(A), Covariance(pa), SetMask(mask), Covariance(pa), Check(2, covariance_pairs=pa),          # a mask between two covariance calls
    ]


# ---- batch --------------------------------------------------------------------------------------------------------------------------
def batch_lives():
    """three handles that have each lived through the first half of windows, factors_all or gate enter cuba_hip_optimize_batch together,
    go on alone, and enter a second batch in another order: name -> (before the first batch, between the two)"""
    A, Av = problem("w40"), other_values(problem("w40"), 6)
    return {"windows": (windows()[:11], [Optimize(1), Hint(True, True), Upload(A)]),
            "factors_all": (factors_all()[:10], [Optimize(1), SetFactors("range_factors", None), start(A)]),
            "gate": (gate()[:5], [Optimize(1), Upload(Av, "two")])}


BATCH_ITERATIONS = (3, 2)


def batch_script(name):
    """one handle's part of the batch test as a script of its own (the dry runs)"""
    first, between = batch_lives()[name]
    return tuple(first + [Batch(BATCH_ITERATIONS[0])] + between + [Batch(BATCH_ITERATIONS[1])])


SCRIPTS = {
    "windows": windows, "windows_refusals": windows_refusals, "orders": orders, "reorder_options": reorder_options,
    "options_pcg_40": functools.partial(options_pcg, "w40"), "options_pcg_150": functools.partial(options_pcg, "w150"),
    "options_solver_40": functools.partial(options_solver, "w40"), "options_solver_150": functools.partial(options_solver, "w150"),
    "options_graphs": options_graphs,
    "factors_unary": factors_unary, "factors_binary": factors_binary, "factors_all": factors_all, "factors_pairs": factors_pairs,
    "gate": gate, "gate_big_landmark": gate_big_landmark, "classes": classes, "partition": partition, "failures": failures,
    "covariance": covariance,
}
# (the fp32 library refuses cuba_hip_compute_covariance[_pairs]: the scripts that call them run on the fp64 library only)
FP64_ONLY = ("covariance", "factors_pairs")


@functools.lru_cache(maxsize=None)
def script(name, precision="f64"):
    fn = SCRIPTS[name]
    return tuple(fn(precision=precision) if name.startswith("options_pcg") else fn())

"""A plain model of the C ABI's state rules (include/cuba_hip.h) -- TEST INFRASTRUCTURE, pure Python and numpy.

A solver handle carries cached facts from one call to the next (the sort, the structure, captured PCG graphs, the coarse inverse, the exact
solver's plan, the gate, the factor sets, snapshots, a pending promise).  This model tracks none of them.  It tracks a `Spec`: everything a
caller needs to build a FRESH handle in the same state -- so that "the reused handle" and "a fresh handle made from the Spec" (the twin of
tests/test_gpu_handle_life.py) must compute the same bits, whatever the reused one has lived through.

The Spec holds the problem in force, the estimates, the robust kernels, the option values, the seven factor sets with the pose-factor
kernels, the edge mask (caller's edge order), the partition and the snapshot slots.  The estimates are the model's own: a run moves them to
"unknown" (None), and only a call that names them -- an upload, set_state, a restore of a slot taken while they were known -- makes them
known again.  Nothing is ever read from a live handle.

The rules, each with the sentence of include/cuba_hip.h it restates (`Rules` holds one switch per rule; the wrong setting of each switch
is what tests/test_handle_life_model.py shows to change the predicted Spec):

  upload_clears_factors     "Valid any time after cuba_hip_set_graph, which clears the set." (every factor kind; the pose-factor kernels:
                            "cuba_hip_set_graph drop[s] them")
  upload_clears_snapshots   "Copies are dropped by cuba_hip_set_graph"
  mask_survives_same_edges  "The mask outlives a cuba_hip_set_graph whose edge arrays (pose, landmark, dimension, count) are those of the
                            previous call -- promised by cuba_hip_hint_unchanged or found by the library's own comparison --  ...  Any other
                            cuba_hip_set_graph drops the mask"
  promise_one_call          "A promise about the NEXT cuba_hip_set_graph call only"
  refusal_consumes_promise  "(it is consumed by that call, successful or not)"
  refusal_keeps_the_rest    "A cuba_hip_set_graph[_begin / _partition] that is refused ... leaves the handle as it was: the previous graph, its
                            factor sets, its mask and its snapshot slots stay in force; only a pending cuba_hip_hint_unchanged promise is
                            consumed."
  ranged_ignores_values     "[a ranged upload] ignores a "same values" promise (cuba_hip_hint_unchanged)"
  wrong promise             "A wrong promise is not detected: the solver then works on the previous call's edges / values."  (The scripts
                            make wrong promises exactly where a rule says the promise is gone: the model then predicts the NEW edges.)
  restore_or_state_error    "restoring an absent slot is CUBA_HIP_ERR_STATE, never a silent mix-up of pose rows"
  options_keep              options and cuba_hip_set_robust_kernel keep their last value across every other call
  landmark_reorder          "takes effect with the next cuba_hip_set_graph" -- invisible in the Spec (every host-pointer entry point keeps
                            the caller's numbering), so the rule is carried by the twin comparison alone.

`apply(step, spec, handle=None)` updates the Spec and, given a handle (cuba_amd.capi.HipSolver), makes the same call on it; without one it
is a dry run.  It appends the names of the transitions the step took (TRANSITIONS) to spec.trace."""
import copy
import dataclasses
import hashlib
from dataclasses import dataclass, field

import numpy as np

import edge_gate_reference as eg

OK, ERR_ARGUMENT, ERR_RUNTIME, ERR_STATE = 0, 1, 2, 3          # (CUBA_HIP_OK, _ERR_INVALID_ARGUMENT, _ERR_RUNTIME, _ERR_STATE)

KINDS = ("pose_priors", "relative_pose_edges", "landmark_priors", "position_factors", "direction_factors", "range_factors",
         "pose_range_factors")
# the keyword under which tests/pose_range_factor_reference.dense_lm takes each kind (pose_range_factors: its positional set)
DENSE_KEYWORD = dict(pose_priors="priors", relative_pose_edges="rel", landmark_priors="lmp", position_factors="pf", direction_factors="df",
                     range_factors="rs", pose_range_factors=None)
CHI2_GETTER = dict(pose_priors="prior_chi_squares", relative_pose_edges="relative_pose_chi_squares",
                   landmark_priors="landmark_prior_chi_squares", position_factors="position_factor_chi_squares",
                   direction_factors="direction_factor_chi_squares", range_factors="range_factor_chi_squares",
                   pose_range_factors="pose_range_factor_chi_squares")
BINARY_KINDS = ("relative_pose_edges", "pose_range_factors")

OPTION_DEFAULTS = dict(pcg_tol=None, pcg_max_iter=None, heuristics=1, precond_fp32=None, pose_reorder=1, device_setup=1, mixed_precision=None,
                       pcg_accept_unconverged=0, direct_fallback=1, direct_after=None, direct_max_tiles=None, direct_slack=None,
                       reduced_solver=0, pcg_aggregate=None, coarse_linear=None, covariance_workspace_mb=0, landmark_reorder=1,
                       reduction_chunks=0, spmv_upper=None, pcg_graph=0, profile=0)          # None: the library's own default, never set


@dataclass
class Rules:
    upload_clears_factors: bool = True
    upload_clears_snapshots: bool = True
    mask_survives_same_edges: bool = True
    promise_one_call: bool = True
    refusal_consumes_promise: bool = True
    refusal_keeps_the_rest: bool = True
    ranged_ignores_values: bool = True
    restore_or_state_error: bool = True
    options_keep: bool = True


RIGHT = Rules()


@dataclass
class Spec:
    fp: object = None                                  # the FlatProblem in force (its q / t / Xw are the UPLOADED estimates)
    est: object = None                                 # (q, t, Xw) now; None: moved by a run
    rk: tuple = ((0, 0.0), (0, 0.0))
    options: dict = field(default_factory=dict)
    precision: str = "f64"
    factors: dict = field(default_factory=dict)        # kind -> the setter's arguments
    kernels: dict = field(default_factory=dict)        # pose-factor type (0 priors, 1 relative-pose edges) -> (kind[n], delta[n])
    mask: object = None                                # bool[E], caller's edge order; None: no gate
    partition: object = None                           # (begin, end) or None
    ranged: bool = False                               # the upload in force was a ranged one
    snapshots: dict = field(default_factory=dict)      # slot -> (q, t, Xw), or None for a copy of unknown estimates
    pushed: object = None                              # push's copy: ("known", est) / ("moved",) / None
    promise: tuple = (False, False)                    # the pending cuba_hip_hint_unchanged
    begun: bool = False                                # a begin-only upload is the one in force
    trace: list = field(default_factory=list)
    checks: list = field(default_factory=list)         # (reference key, iterations) of every check step, in order
    rules: Rules = field(default_factory=Rules)

    # ---- what a fresh handle needs ---------------------------------------------------------------------------------------------------
    def problem(self):
        """the FlatProblem a twin uploads: the one in force with the model's estimates"""
        assert self.fp is not None and self.est is not None, "the estimates are unknown here: name them before a check"
        return eg.with_state(self.fp, self.est)

    def key(self):
        """a digest of everything a fresh handle would be built from (the trace and the pending promise are not part of it)"""
        h = hashlib.sha1()

        def put(x):
            if x is None:
                h.update(b"<none>")
            elif isinstance(x, np.ndarray):
                h.update(str(x.dtype).encode() + str(x.shape).encode() + np.ascontiguousarray(x).tobytes())
            elif isinstance(x, (tuple, list)):
                h.update(b"(%d" % len(x))
                for y in x:
                    put(y)
            elif isinstance(x, dict):
                for k in sorted(x, key=str):
                    put(str(k)); put(x[k])
            else:
                h.update(repr(x).encode())
        fp = self.fp
        if fp is not None:
            put([fp.Pt, fp.Pf, fp.Lt, fp.Lf, fp.cam, fp.eP, fp.eL, fp.eDim, fp.meas, fp.omega])
        put(self.est); put(self.rk); put({k: v for k, v in self.options.items() if v is not None}); put(self.precision)
        put(self.factors); put(self.kernels); put(self.mask); put(self.partition); put(self.ranged); put(self.snapshots)
        return h.hexdigest()

    def reference_key(self):
        """what the fp64 reference run depends on: the key without the options, the precision, the partition and the snapshots"""
        s = dataclasses.replace(self, options={}, precision="f64", partition=None, ranged=False, snapshots={})
        return s.key()


def copy_est(e):
    return None if e is None else tuple(np.array(a, dtype=np.float64) for a in e)


def same_index_arrays(a, b):
    return (a is not None and b is not None and (a.Pt, a.Pf, a.Lt, a.Lf, a.E) == (b.Pt, b.Pf, b.Lt, b.Lf, b.E)
            and np.array_equal(a.eP, b.eP) and np.array_equal(a.eL, b.eL) and np.array_equal(a.eDim, b.eDim))


def same_counts(a, b):
    return a is not None and b is not None and (a.Pt, a.Pf, a.Lt, a.Lf, a.E) == (b.Pt, b.Pf, b.Lt, b.Lf, b.E)


def upload_refusal(fp, landmark_range=None, edges_promised=False):
    """None, or the kind of refusal (CUBA_HIP_ERR_INVALID_ARGUMENT) cuba_hip_set_graph answers to these arguments.  edges_promised: "the
    library then skips its own comparison of the index arrays" -- and with it their validation: the arrays are not read at all"""
    if landmark_range is not None and not (0 <= landmark_range[0] <= landmark_range[1] <= fp.Lt):
        return "range"
    if min(fp.Pt, fp.Pf, fp.Lt, fp.Lf, len(fp.eP)) < 0 or fp.Pf > fp.Pt or fp.Lf > fp.Lt:
        return "counts"
    if edges_promised:
        return None
    eP, eL = np.asarray(fp.eP), np.asarray(fp.eL)
    if ((eP < 0) | (eP >= fp.Pt) | (eL < 0) | (eL >= fp.Lt)).any():
        return "edge_index"
    if (~np.isin(fp.eDim, (2, 3))).any():
        return "edge_dim"
    if ((eP >= fp.Pf) & (eL >= fp.Lf)).any():
        return "both_fixed"
    return None


# ---- the step vocabulary ------------------------------------------------------------------------------------------------------------
@dataclass
class Upload:
    """cuba_hip_set_graph (form "one"), _begin + build_structure + _end ("two"), _begin alone ("begin"), _partition ("ranged")"""
    fp: object
    form: str = "one"
    landmark_range: tuple = None


@dataclass
class Hint:
    same_edges: bool = True
    same_values: bool = False


@dataclass
class SetFactors:
    """the setter of one kind with these arguments; args None: the empty set (clears)"""
    kind: str
    args: tuple = None


@dataclass
class SetPoseFactorKernels:
    factor_type: int
    kind: object = None
    delta: object = None


@dataclass
class Gate:
    chi2_max: tuple = (eg.CHI2_MONO, eg.CHI2_STEREO)
    positive_depth: bool = True
    mode: str = "reclassify"


@dataclass
class SetMask:
    mask: object = None            # None: cuba_hip_set_edge_active(NULL)


@dataclass
class SetOption:
    key: str
    value: float


@dataclass
class SetRobustKernel:
    edge_type: int
    kind: int
    delta: float


@dataclass
class SetState:
    est: tuple


@dataclass
class Snapshot:
    slot: int = 0


@dataclass
class Restore:
    """may_be_dropped: the library may have dropped the slot with its internal pose order ("Copies are dropped ... whenever the library
    changes its internal pose order"); the call then answers CUBA_HIP_ERR_STATE and leaves the estimates alone.  Which of the two happens is
    the library's business, so a script names the estimates (SetState) after such a step, and the next check sees a mix-up of rows."""
    slot: int = 0
    may_be_dropped: bool = False


@dataclass
class Push:
    pass


@dataclass
class Pop:
    pass


@dataclass
class SetPartition:
    begin: int
    end: int


@dataclass
class Covariance:
    """cuba_hip_compute_covariance, then cuba_hip_compute_covariance_pairs on `pairs`; both are asked for again at the next check"""
    pairs: tuple = ()


@dataclass
class Optimize:
    niter: int


@dataclass
class Stages:
    """one hand-driven trial: errors, system, lambda, solve, update"""
    pass


@dataclass
class Batch:
    """cuba_hip_optimize_batch of this handle with `others` (live handles of the test; a dry run ignores them), this one at `position`.
    Like a Check it needs known estimates: every handle of the batch is compared with a twin that runs alone."""
    niter: int
    others: tuple = ()
    position: int = 0


@dataclass
class ExpectPoseOrder:
    """the internal pose order reported by the test hook (pcg_config) is the identity, or is not; a dry run takes the script's word"""
    identity: bool


@dataclass
class Refused:
    """a call that must be answered with `status` and change nothing but what the header says it consumes"""
    step: object
    status: int


@dataclass
class Check:
    """the twin comparison (tests/test_gpu_handle_life.py), then optimize(niter) on both"""
    niter: int = 3
    covariance_pairs: tuple = None       # not None: covariance blocks and these pairs are compared too
    reference: bool = True               # False only under an option with which the library itself does not promise the fp64 bar (mixed_precision)


# ---- transitions: (call, what the handle had lived through) ---------------------------------------------------------------------------
TRANSITIONS = {
    "upload.first": "the first upload of a handle",
    "upload.one_call": "cuba_hip_set_graph", "upload.two_step": "_begin, build_structure, _end", "upload.begin_only": "_begin without its _end",
    "upload.ranged": "cuba_hip_set_graph_partition",
    "upload.shrinks": "fewer poses than the upload in force", "upload.grows": "more poses than any upload before",
    "upload.returns": "a size the handle has held before, after another one",
    "upload.identical.compared": "same index arrays and values, no promise",
    "upload.identical.promised_edges": "same index arrays, (True, False)",
    "upload.identical.promised_values": "same index arrays, (True, True)",
    "upload.same_counts_other_edges": "all five counts equal, other index arrays",
    "upload.same_edges_other_values": "same index arrays, other measurements or information",
    "upload.same_edges_other_estimates": "same index arrays and values, other estimates",
    "upload.promised_after_begin_only": "a promise of values right after a begin-only upload",
    "upload.wrong_promise_after_refusal": "same counts, other edges, a promise made before a refused call",
    "upload.ranged_with_values_promise": "a ranged upload under a (True, True) promise",
    "upload.whole_after_ranged": "a whole upload after a ranged one",
    "upload.drops_factors": "factor sets were in force", "upload.drops_snapshots": "snapshot slots were in use",
    "upload.keeps_mask": "a mask was set, same edges", "upload.drops_mask": "a mask was set, other edges",
    "upload.with_graphs_captured": "pcg_graph = 1 and a run behind it",
    "upload.after_exact_solve": "reduced_solver = 1 and a run behind it",
    "upload.after_covariance": "a covariance behind it",
    "upload.order_changes": "shuffled pose ids after ordered ones, or back", "upload.order_kept": "the shuffled graph again",
    "upload.after_landmark_reorder.identical": "landmark_reorder changed, same index arrays",
    "upload.after_landmark_reorder.other": "landmark_reorder changed, other index arrays",
    "refused.upload.counts": "Pf > Pt", "refused.upload.range": "a bad landmark range", "refused.upload.edge_index": "an edge index out of range",
    "refused.upload.with_promise": "a promise was pending", "refused.upload.with_factors": "factor sets were in force",
    "refused.upload.with_mask": "a mask was set", "refused.upload.with_snapshot": "a slot was in use",
    "refused.upload.after_begin_only": "a begin-only upload was the one in force: it stays, with ITS values",
    "refused.factors": "a factor set the library refuses", "refused.factors.partitioned": "a factor set on a partitioned handle",
    "refused.option": "a value or key cuba_hip_set_option refuses", "refused.restore": "an empty slot",
    "hint": "cuba_hip_hint_unchanged",
    "factors.set": "a kind without a set", "factors.replace": "a set of another length", "factors.clear": "n = 0",
    "factors.all_seven": "the seventh kind joins six", "factors.pair_union_changes": "the binary kinds' union of pairs changes",
    "factors.pair_union_changes.with_mask": "... while a mask is set", "factors.pair_union_changes.after_exact_solve": "... after an exact solve",
    "factors.pair_union_changes.after_covariance": "... after a covariance", "factors.after_resize": "after a window of another size",
    "factors.kernels": "pose-factor kernels set, replaced or cleared",
    "gate.reclassify": "", "gate.only_remove": "", "gate.dry_run": "", "mask.set": "", "mask.clear": "", "mask.with_factors": "a mask beside factor sets",
    "mask.big_landmark": "half of a landmark with more than 64 observations",
    "option.live": "cuba_hip_set_option on a handle with a structure", "option.after_run": "... with a run behind it",
    "option.back": "a key returns to the value it had",
    "robust_kernel.live": "cuba_hip_set_robust_kernel between runs",
    "state.set": "", "snapshot": "", "restore": "", "restore.after_upload": "the slot was dropped by an upload", "push": "", "pop": "",
    "partition.set": "", "partition.lifted": "",
    "covariance": "", "covariance.with_mask": "", "covariance.after_resize": "", "covariance.option_between": "reduced_solver or direct_slack changed since the last one",
    "run": "cuba_hip_optimize", "run.zero_iterations": "niter = 0", "run.every_solve_fails": "pcg_max_iter = 1 without a fallback",
    "run.after_failed_run": "the run after it", "stages": "", "batch": "", "batch.again": "a second batch in another order",
    "class.big_landmarks": "", "class.duplicates": "", "class.pose_only": "", "class.landmark_only": "", "class.all_mono": "", "class.all_stereo": "",
    "class.plain_again": "",
    "check": "", "check.with_mask": "", "check.with_factors": "", "check.with_robust_kernels": "",
}

# the option keys the scripts must move on a live handle, each to a second value and back (section "options" of the issue)
LIVE_OPTION_KEYS = ("pcg_aggregate", "coarse_linear", "precond_fp32", "spmv_upper", "pcg_max_iter", "reduction_chunks", "mixed_precision",
                    "profile", "reduced_solver", "direct_slack", "direct_max_tiles", "direct_fallback", "pcg_tol", "pcg_graph",
                    "landmark_reorder", "pose_reorder", "device_setup")
for _k in LIVE_OPTION_KEYS:
    TRANSITIONS["option." + _k] = "the key on a live handle"
for _k in KINDS:
    TRANSITIONS["factors." + _k] = "the kind set at least once"


def graph_classes(fp):
    """the kernel classes a graph leaves the plain one for, read from its arrays"""
    out = []
    E = len(fp.eP)
    if E and np.bincount(fp.eL, minlength=fp.Lt).max() > 64: out.append("big_landmarks")
    if E and len(np.unique(fp.eP.astype(np.int64) * fp.Lt + fp.eL)) < E: out.append("duplicates")
    if fp.Lf == 0: out.append("pose_only")
    if fp.Pf == 0: out.append("landmark_only")
    if E and (fp.eDim == 2).all(): out.append("all_mono")
    if E and (fp.eDim == 3).all(): out.append("all_stereo")
    return out


def free_pairs(spec):
    """the binary kinds' union of distinct free-free pairs: part of the topology"""
    out = set()
    Pf = spec.fp.Pf if spec.fp is not None else 0
    for kind in BINARY_KINDS:
        if kind in spec.factors:
            for i, j in zip(spec.factors[kind][0], spec.factors[kind][1]):
                i, j = int(i), int(j)
                if i < Pf and j < Pf:
                    out.add((min(i, j), max(i, j)))
    return out


def factor_count(args):
    return 0 if args is None else int(np.asarray(args[0]).size)


class Life:
    """what the handle has lived through, for the predicates of TRANSITIONS only -- never for the Spec"""

    def __init__(self):
        self.sizes, self.max_poses = [], 0
        self.ran = self.ran_exact = self.ran_graphs = self.covariance = self.failed_run = False
        self.reorder_changed = self.cov_option_changed = False
        self.shuffled = None
        self.option_history = {}
        self.classes, self.refused_with_promise = set(), False


def _life(spec):
    if not hasattr(spec, "_life"):
        spec._life = Life()
    return spec._life


def _hit(spec, *names):
    for n in names:
        assert n in TRANSITIONS, n
        spec.trace.append(n)


def _call(handle, fn, *a, **kw):
    """the call on the live handle, when there is one"""
    if handle is not None:
        return getattr(handle, fn)(*a, **kw)
    return None


def _expect_status(handle, status, fn):
    if handle is None:
        return
    from cuba_amd.capi import CubaHipError
    try:
        fn()
    except CubaHipError as e:
        assert str(e).startswith("status %d:" % status), (str(e), status)
        return
    raise AssertionError("the call was accepted; expected status %d" % status)


def _upload(step, spec, handle, refused_status=None):
    rules, life = spec.rules, _life(spec)
    fp, prev = step.fp, spec.fp
    ranged = step.form == "ranged"
    promised_edges, promised_values = spec.promise
    refusal = upload_refusal(fp, step.landmark_range if ranged else None, promised_edges and same_counts(prev, fp) and not spec.ranged and not ranged)
    had_promise = promised_edges
    call = lambda: handle.set_graph(fp, two_step={"one": False, "two": True, "begin": "begin_only", "ranged": False}[step.form],          # noqa: E731
                                    landmark_range=step.landmark_range if ranged else None)
    if refusal is not None:
        assert refused_status == ERR_ARGUMENT, "the model refuses this upload (%s): wrap it in Refused(step, ERR_ARGUMENT)" % refusal
        _hit(spec, "refused.upload." + refusal)
        if had_promise:
            _hit(spec, "refused.upload.with_promise")
            life.refused_with_promise = True
        if spec.factors: _hit(spec, "refused.upload.with_factors")
        if spec.mask is not None: _hit(spec, "refused.upload.with_mask")
        if spec.snapshots: _hit(spec, "refused.upload.with_snapshot")
        if spec.begun: _hit(spec, "refused.upload.after_begin_only")
        _expect_status(handle, ERR_ARGUMENT, call)
        if rules.refusal_consumes_promise:
            spec.promise = (False, False)
        if not rules.refusal_keeps_the_rest:
            spec.factors, spec.kernels = {}, {}
        return
    assert refused_status is None, "the model accepts this upload"
    if handle is not None:
        call()
    counts_equal = same_counts(prev, fp) and not spec.ranged
    identical = counts_equal and same_index_arrays(prev, fp)
    # "A wrong promise is not detected: the solver then works on the previous call's edges / values"; a ranged upload reuses nothing
    honoured_edges = promised_edges and counts_equal and not ranged
    honoured_values = (promised_edges and promised_values and counts_equal and not spec.begun
                       and not (ranged and rules.ranged_ignores_values))
    same_edges = (identical or honoured_edges) and not ranged
    new = copy.copy(fp)
    if honoured_edges and not identical:
        new.eP, new.eL, new.eDim = prev.eP, prev.eL, prev.eDim
    if honoured_values:
        new.meas, new.omega = prev.meas, prev.omega
    # ---- transitions ----
    _hit(spec, {"one": "upload.one_call", "two": "upload.two_step", "begin": "upload.begin_only", "ranged": "upload.ranged"}[step.form])
    if prev is None: _hit(spec, "upload.first")
    else:
        if fp.Pt < prev.Pt: _hit(spec, "upload.shrinks")
        if fp.Pt > life.max_poses: _hit(spec, "upload.grows")
        if fp.Pt != prev.Pt and fp.Pt in life.sizes: _hit(spec, "upload.returns")
    if identical:
        same_vals = np.array_equal(prev.meas, fp.meas) and np.array_equal(prev.omega, fp.omega)
        if not same_vals: _hit(spec, "upload.same_edges_other_values")
        elif not promised_edges:
            _hit(spec, "upload.identical.compared")
            if not all(np.array_equal(a, b) for a, b in zip((prev.q, prev.t, prev.Xw), (fp.q, fp.t, fp.Xw))):
                _hit(spec, "upload.same_edges_other_estimates")
        elif promised_values: _hit(spec, "upload.identical.promised_values")
        else: _hit(spec, "upload.identical.promised_edges")
    elif counts_equal: _hit(spec, "upload.same_counts_other_edges")
    if spec.begun and promised_values: _hit(spec, "upload.promised_after_begin_only")
    if ranged and promised_values: _hit(spec, "upload.ranged_with_values_promise")
    if spec.ranged and not ranged: _hit(spec, "upload.whole_after_ranged")
    if spec.factors: _hit(spec, "upload.drops_factors")
    if spec.snapshots: _hit(spec, "upload.drops_snapshots")
    if spec.mask is not None: _hit(spec, "upload.keeps_mask" if same_edges else "upload.drops_mask")
    if life.ran_graphs: _hit(spec, "upload.with_graphs_captured")
    if life.ran_exact: _hit(spec, "upload.after_exact_solve")
    if life.covariance: _hit(spec, "upload.after_covariance")
    shuffled = getattr(fp, "shuffled", False)
    if life.shuffled is not None:
        if shuffled != life.shuffled: _hit(spec, "upload.order_changes")
        elif shuffled and identical: _hit(spec, "upload.order_kept")
    if life.reorder_changed: _hit(spec, "upload.after_landmark_reorder.identical" if identical else "upload.after_landmark_reorder.other")
    life.shuffled, life.reorder_changed = shuffled, False
    klass = graph_classes(fp)
    _hit(spec, *["class." + k for k in klass])
    if not klass and life.classes: _hit(spec, "class.plain_again")
    life.classes |= set(klass)
    if life.refused_with_promise and counts_equal and not identical: _hit(spec, "upload.wrong_promise_after_refusal")
    life.refused_with_promise = False
    life.sizes.append(fp.Pt); life.max_poses = max(life.max_poses, fp.Pt)
    life.ran = life.ran_exact = life.ran_graphs = life.covariance = False
    # ---- the Spec ----
    spec.fp, spec.est = new, copy_est((fp.q, fp.t, fp.Xw))
    if rules.upload_clears_factors:
        spec.factors, spec.kernels = {}, {}
    if rules.upload_clears_snapshots:
        spec.snapshots = {}
    spec.pushed = None
    if not (same_edges and rules.mask_survives_same_edges):
        spec.mask = None
    if rules.promise_one_call:
        spec.promise = (False, False)
    spec.begun = step.form == "begin"
    spec.ranged = ranged
    spec.partition = tuple(step.landmark_range) if ranged else None


def _set_factors(step, spec, handle, refused_status=None):
    life = _life(spec)
    setter = "set_" + step.kind
    n = factor_count(step.args)
    empty_args = {"pose_priors": ([], np.zeros((0, 4)), np.zeros((0, 3)), np.zeros((0, 6, 6))),
                  "relative_pose_edges": ([], [], np.zeros((0, 4)), np.zeros((0, 3)), np.zeros((0, 6, 6))),
                  "landmark_priors": ([], np.zeros((0, 3)), np.zeros((0, 3, 3))),
                  "position_factors": ([], np.zeros((0, 3)), np.zeros((0, 3, 3))),
                  "direction_factors": ([], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3, 3))),
                  "range_factors": ([], np.zeros((0, 3)), np.zeros(0), np.zeros(0)),
                  "pose_range_factors": ([], [], np.zeros(0), np.zeros(0))}[step.kind]
    args = step.args if n else empty_args
    if refused_status is not None:
        _hit(spec, "refused.factors.partitioned" if spec.partition is not None else "refused.factors")
        _expect_status(handle, refused_status, lambda: getattr(handle, setter)(*args))
        return
    assert spec.partition is None, "a landmark-partitioned handle refuses factor sets: wrap the step in Refused(step, ERR_STATE)"
    _call(handle, setter, *args)
    before = free_pairs(spec)
    had = step.kind in spec.factors
    if n:
        _hit(spec, "factors." + step.kind)
        if had and factor_count(spec.factors[step.kind]) != n: _hit(spec, "factors.replace")
        elif not had: _hit(spec, "factors.set")
        spec.factors[step.kind] = step.args
        if len(spec.factors) == len(KINDS) and not had: _hit(spec, "factors.all_seven")
    else:
        _hit(spec, "factors.clear")
        spec.factors.pop(step.kind, None)
    if step.kind in ("pose_priors", "relative_pose_edges"):          # "The kernels belong to the set ... (the replaced set is a new set)"
        spec.kernels.pop(0 if step.kind == "pose_priors" else 1, None)
    if free_pairs(spec) != before:
        _hit(spec, "factors.pair_union_changes")
        if spec.mask is not None: _hit(spec, "factors.pair_union_changes.with_mask")
        if life.ran_exact: _hit(spec, "factors.pair_union_changes.after_exact_solve")
        if life.covariance: _hit(spec, "factors.pair_union_changes.after_covariance")
    if len(set(life.sizes)) > 1: _hit(spec, "factors.after_resize")
    if spec.mask is not None: _hit(spec, "mask.with_factors")


def _set_option(step, spec, handle, refused_status=None):
    life = _life(spec)
    if refused_status is not None:
        _hit(spec, "refused.option")
        _expect_status(handle, refused_status, lambda: handle.set_option(step.key, step.value))
        return
    _call(handle, "set_option", step.key, step.value)
    if spec.fp is not None:
        _hit(spec, "option.live")
        if life.ran: _hit(spec, "option.after_run")
        if step.key in LIVE_OPTION_KEYS: _hit(spec, "option." + step.key)
        hist = life.option_history.setdefault(step.key, [spec.options.get(step.key, OPTION_DEFAULTS.get(step.key))])
        if step.value in hist[:-1] or (len(hist) > 1 and step.value == hist[0]): _hit(spec, "option.back")
        hist.append(step.value)
    if step.key == "landmark_reorder": life.reorder_changed = True
    if step.key in ("reduced_solver", "direct_slack") and life.covariance: life.cov_option_changed = True
    if spec.rules.options_keep:
        spec.options[step.key] = step.value


def _ran(spec, niter=1):
    life = _life(spec)
    if life.failed_run: _hit(spec, "run.after_failed_run")
    life.failed_run = spec.options.get("pcg_max_iter") == 1 and spec.options.get("direct_fallback") == 0 and niter > 0
    if life.failed_run: _hit(spec, "run.every_solve_fails")
    if niter > 0:
        life.ran = True
        life.ran_exact = life.ran_exact or spec.options.get("reduced_solver") == 1
        life.ran_graphs = life.ran_graphs or spec.options.get("pcg_graph") == 1
        spec.est = None
        spec.pushed = ("moved",)          # (the LM loop's own push / pop: "overwritten by every trial of cuba_hip_optimize")


def apply(step, spec, handle=None):
    """the step on the Spec, and on the handle when one is given; returns what the call returned (None in a dry run)"""
    life = _life(spec)
    if isinstance(step, Refused):
        inner = step.step
        if isinstance(inner, Upload): return _upload(inner, spec, handle, step.status)
        if isinstance(inner, SetFactors): return _set_factors(inner, spec, handle, step.status)
        if isinstance(inner, SetOption): return _set_option(inner, spec, handle, step.status)
        if isinstance(inner, Restore):
            assert inner.slot not in spec.snapshots and step.status == ERR_STATE
            _hit(spec, "refused.restore")
            if not spec.fp is None and life.sizes and not spec.snapshots: _hit(spec, "restore.after_upload")
            return _expect_status(handle, ERR_STATE, lambda: handle.restore_state(inner.slot))
        raise TypeError(inner)
    if isinstance(step, Upload): return _upload(step, spec, handle)
    if isinstance(step, Hint):
        _hit(spec, "hint")
        spec.promise = (bool(step.same_edges), bool(step.same_edges and step.same_values))
        return _call(handle, "hint_unchanged", step.same_edges, step.same_values)
    if isinstance(step, SetFactors): return _set_factors(step, spec, handle)
    if isinstance(step, SetPoseFactorKernels):
        _hit(spec, "factors.kernels")
        if step.kind is None: spec.kernels.pop(step.factor_type, None)
        else: spec.kernels[step.factor_type] = (np.asarray(step.kind, dtype=np.int32), np.asarray(step.delta, dtype=np.float64))
        return _call(handle, "set_pose_factor_robust_kernels", step.factor_type, [] if step.kind is None else step.kind,
                     [] if step.kind is None else step.delta)
    if isinstance(step, Gate):
        assert spec.est is not None, "gate_edges judges at the estimates: name them first"
        _hit(spec, "gate." + step.mode)
        c = eg.classify(spec.problem(), None, step.chi2_max, step.positive_depth, step.mode, spec.mask)
        assert eg.threshold_margin(spec.fp, c["chi2"], step.chi2_max).min() > 1e-3, "an edge sits on its threshold: fp32 rounding could flip it"
        got = _call(handle, "gate_edges", step.chi2_max, step.positive_depth, step.mode)
        if got is not None:
            assert got == c["counts"], (got, c["counts"])
        if step.mode != "dry_run":
            spec.mask = c["mask"].copy()
            if spec.factors: _hit(spec, "mask.with_factors")
        return got
    if isinstance(step, SetMask):
        _hit(spec, "mask.clear" if step.mask is None else "mask.set")
        spec.mask = None if step.mask is None else np.asarray(step.mask, bool).copy()
        if spec.mask is not None:
            if spec.factors: _hit(spec, "mask.with_factors")
            off = np.bincount(spec.fp.eL[~spec.mask], minlength=spec.fp.Lt)
            if ((np.bincount(spec.fp.eL, minlength=spec.fp.Lt) > 64) & (off > 0)).any(): _hit(spec, "mask.big_landmark")
        return _call(handle, "set_edge_active", step.mask)
    if isinstance(step, SetOption): return _set_option(step, spec, handle)
    if isinstance(step, SetRobustKernel):
        if spec.fp is not None: _hit(spec, "robust_kernel.live")
        if spec.rules.options_keep:
            rk = list(spec.rk); rk[step.edge_type] = (int(step.kind), float(step.delta)); spec.rk = tuple(rk)
        return _call(handle, "set_robust_kernel", step.edge_type, step.kind, step.delta)
    if isinstance(step, SetState):
        _hit(spec, "state.set")
        spec.est = copy_est(step.est)
        return _call(handle, "set_state", *step.est)
    if isinstance(step, Snapshot):
        _hit(spec, "snapshot")
        spec.snapshots[step.slot] = copy_est(spec.est)
        return _call(handle, "snapshot_state", step.slot)
    if isinstance(step, Restore):
        assert step.slot in spec.snapshots, "the model holds no such slot: wrap the step in Refused(step, ERR_STATE)"
        _hit(spec, "restore")
        if handle is not None and step.may_be_dropped:
            from cuba_amd.capi import CubaHipError
            try:
                handle.restore_state(step.slot)
            except CubaHipError as e:
                assert str(e).startswith("status %d:" % ERR_STATE), str(e)
                del spec.snapshots[step.slot]
                return ERR_STATE
        else:
            _call(handle, "restore_state", step.slot)
        if spec.rules.restore_or_state_error:
            spec.est = copy_est(spec.snapshots[step.slot])
        return OK
    if isinstance(step, ExpectPoseOrder):
        if handle is not None:
            order = handle.pcg_config()["pose_order"]
            assert len(order) == spec.fp.Pf and np.array_equal(order, np.arange(len(order))) == step.identity, order
        return None
    if isinstance(step, Push):
        _hit(spec, "push")
        spec.pushed = ("known", copy_est(spec.est)) if spec.est is not None else ("moved",)
        return _call(handle, "push")
    if isinstance(step, Pop):
        _hit(spec, "pop")
        assert spec.pushed is not None
        spec.est = copy_est(spec.pushed[1]) if spec.pushed[0] == "known" else None
        return _call(handle, "pop")
    if isinstance(step, SetPartition):
        lifted = step.end < 0
        _hit(spec, "partition.lifted" if lifted else "partition.set")
        spec.partition = None if lifted else (step.begin, step.end)
        return _call(handle, "set_partition", step.begin, step.end)
    if isinstance(step, Covariance):
        _hit(spec, "covariance")
        if spec.mask is not None: _hit(spec, "covariance.with_mask")
        if len(set(life.sizes)) > 1: _hit(spec, "covariance.after_resize")
        if life.cov_option_changed: _hit(spec, "covariance.option_between")
        life.covariance, life.cov_option_changed = True, False
        if handle is not None:
            return handle.covariance(), handle.covariance_pairs(list(step.pairs))
        return None
    if isinstance(step, Optimize):
        _hit(spec, "run")
        if step.niter == 0: _hit(spec, "run.zero_iterations")
        _ran(spec, step.niter)
        return _call(handle, "optimize", step.niter)
    if isinstance(step, Stages):
        _hit(spec, "stages")
        pushed = spec.pushed
        _ran(spec)
        spec.pushed = pushed          # (the stage calls leave push's copy alone)
        if handle is not None:
            handle.compute_errors(); handle.build_system(); handle.set_lambda(1e-5 * handle.max_diagonal())
            ok = handle.solve(); handle.update(); handle.restore_diagonal()
            return ok
        return None
    if isinstance(step, Batch):
        _hit(spec, "batch.again" if "batch" in spec.trace else "batch")
        assert spec.est is not None, "the estimates are unknown here: name them before a batch"
        spec.checks.append((spec.reference_key(), step.niter))
        if handle is not None:
            from cuba_amd.capi import optimize_batch
            hs = list(step.others); hs.insert(step.position, handle)
            return optimize_batch(hs, step.niter)
        return None          # (as with a check: the caller compares with the twins' solo runs, then calls ran())
    if isinstance(step, Check):
        _hit(spec, "check")
        if spec.mask is not None: _hit(spec, "check.with_mask")
        if spec.factors: _hit(spec, "check.with_factors")
        if any(k for k, _ in spec.rk): _hit(spec, "check.with_robust_kernels")
        assert spec.est is not None, "the estimates are unknown here: name them before a check"
        if spec.partition is None:          # (a partitioned handle evaluates its own landmarks only: its stages are compared, nothing is run)
            assert step.niter >= 2
            spec.checks.append((spec.reference_key(), step.niter))
        return None          # (the GPU module runs the comparison and then calls ran())
    raise TypeError(step)


def ran(spec, niter):
    """the bookkeeping of the optimize(niter) a check ends with"""
    _ran(spec, niter)


# ---- the fp64 reference of a checkpoint ------------------------------------------------------------------------------------------------
_references = {}


def reference(spec, niter):
    """chi2 per iteration of the plain fp64 LM on the Spec's problem: OracleSolver, or pose_range_factor_reference.dense_lm when factors
    are present (all seven kinds); a mask is applied by handing over the sub-graph of the active edges, as tests/edge_gate_reference.py
    does; the dense LM too where a pose observes a landmark twice.  Cached by the Spec's reference key."""
    key = (spec.reference_key(), niter)
    if key not in _references:
        import pose_range_factor_reference as pp
        from oracle.oracle import OracleSolver
        fp = spec.problem()
        if spec.mask is not None and not spec.mask.all():
            fp = eg.without_edges(fp, spec.mask)
        o = OracleSolver(fp, spec.rk)
        # (a pose that observes a landmark twice: the oracle restates the reference's diagonal block, T where the complete Schur complement
        # has T + T^T -- DESIGN section 5, tests/test_gpu_configs.py::test_duplicate_observations_of_one_pose --, so the dense LM on the
        # full normal equations is the reference there)
        if spec.factors or "duplicates" in graph_classes(fp):
            kw = {DENSE_KEYWORD[k]: v for k, v in spec.factors.items() if DENSE_KEYWORD[k]}
            if 0 in spec.kernels: kw["kp"] = spec.kernels[0]
            if 1 in spec.kernels: kw["kr"] = spec.kernels[1]
            chi2 = pp.dense_lm(o, fp, spec.factors.get("pose_range_factors"), niter, **kw)["chi2"]
        else:
            chi2 = o.optimize(niter)["chi2"]
        _references[key] = np.array(chi2)
    return _references[key]


def run_script(steps, spec=None, handle=None, on_check=None):
    """every step in order; on_check(spec, step) is called at each Check (the GPU module's comparison)"""
    spec = Spec() if spec is None else spec
    for step in steps:
        apply(step, spec, handle)
        if isinstance(step, (Check, Batch)):
            if on_check is not None:
                on_check(spec, step)
            if spec.partition is None:
                ran(spec, step.niter)
    return spec

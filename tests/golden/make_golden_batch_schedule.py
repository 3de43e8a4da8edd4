"""Generates tests/golden/batch_schedule.json: the host's schedule of cuba_hip_optimize_batch -- what a batch enqueues and when it looks --
which tests/test_gpu_batch.py cannot see: it holds every handle of a batch bit for bit to a solo run, and a batch that enqueued twice the
iterations or took twice the host looks would still pass it.  After every optimize_batch call of every case, per handle, the counters
lm_trials, pcg_iterations, pcg_iterations_enqueued, pcg_host_looks, host_looks, coarse_refreshes, coarse_inline_inversions,
exact_solve_fallbacks, pcg_unconverged_solves, precond_fp32_fallbacks and pcg_history()[0]; for the lead also batch_full_trials,
batch_iteration_trials and the call's count of batched reduced solves.  All of them follow from the call sequence and from what the device
reports at a look, never from timing: two recordings at the commit named in the fixture agreed in every leaf, so none is left out.

Cases, on the graphs of tests/test_gpu_batch.py (39 to 599 free poses, handles built by its spec / make): the full path with three graphs,
smallest and largest first; the iterations-only path (one mixed-precision handle of two), both orders; per-graph iteration limits
1 / 4 / 5 / 17 with a tolerance that never fires; a run that ends early and a handle whose solves fail, each at position 1; a second call
on the same handles; a handle that leaves its kernel class (kept and restored) at position 1 on the full path, and at positions 0 and 1 on
the iterations-only path.  The fp32 library records the full-path cases that do not depend on how the coarse inverse is stored (it has
neither mixed precision nor an fp32-stored inverse to drop, hence no iterations-only batch of these graphs and no class change).
tests/test_gpu_batch_schedule.py recomputes every entry through record() below and asserts equality: the fixture pins a change that must
leave the schedule alone (a refactor of the batch loops) to the commit it was recorded at.

Needs the GPU; re-record when the toolchain changes (the fixture names the hipcc it was built with and the git tree hash of
cuda-bundle-adjustment_amd/csrc that the recorded library was built from), never to make a source change pass.  Run from the repo root:
`python tests/golden/make_golden_batch_schedule.py OUT.json $(git rev-parse HEAD:cuda-bundle-adjustment_amd/csrc)`."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import test_gpu_batch as tb  # noqa: E402

from cuba_amd.capi import optimize_batch  # noqa: E402

PRECISIONS = ("f64", "f32")
PER_HANDLE = ("lm_trials", "pcg_iterations", "pcg_iterations_enqueued", "pcg_host_looks", "host_looks", "coarse_refreshes", "coarse_inline_inversions",
              "exact_solve_fallbacks", "pcg_unconverged_solves", "precond_fp32_fallbacks")
LEAD = ("batch_full_trials", "batch_iteration_trials")


def cases(precision):
    """name -> (specs, plan, path); the specs of the tests of tests/test_gpu_batch.py that the names recall"""
    def spec(*a, **k):
        return tb.spec(*a, precision=precision, **k)
    three = [spec("small"), spec("mid"), spec("g450")]
    iterates = [spec("mid", start=i, pcg_max_iter=K, pcg_accept_unconverged=1, direct_fallback=0, pcg_tol=tb.NEVER) for i, K in enumerate((1, 4, 5, 17))]
    out = {
        "full_smallest_first": (three, (4,), "full"),
        "full_largest_first": (three[::-1], (4,), "full"),
        "iteration_limits_1_4_5_17": (iterates, (1,), "full"),
        "early_end_at_1": ([spec("mid"), spec("clean", start="converged"), spec("g450")], (6,), "full"),
        "failing_at_1": ([spec("small"), spec("mid", start=3, pcg_max_iter=1, direct_fallback=0), spec("g450")], (3,), "full"),
        "second_call": ([spec("small"), spec("mid"), spec("g450", start=1)], (4, "reset", 4), "full"),
    }
    if precision == "f64":
        mixed = [spec("mid", mixed_precision=1), spec("small")]
        out["iterations_mixed_first"] = (mixed, (4,), "iterations")
        out["iterations_plain_first"] = (mixed[::-1], (4,), "iterations")
        for variant, (opts, other_opts) in tb.CLASS_CHANGE.items():
            out["class_change_%s_at_1" % variant] = ([spec("small", **other_opts), spec("gaugefree", robust_none=1, **opts), spec("mid", **other_opts)], (40,), "full")
        for position in (0, 1):
            out["class_change_iterations_at_%d" % position] = (tb.class_change_iterations_only(position)[1], (40,), "iterations")
    return out


def snapshot(hs, batched):
    out = []
    for i, h in enumerate(hs):
        d = {k: h.counter(k) for k in PER_HANDLE}
        d["pcg_history"] = [int(v) for v in h.pcg_history()[0]]
        if i == 0:
            d.update({k: h.counter(k) for k in LEAD})
            d["batched_solves"] = int(batched)
        out.append(d)
    return out


def record_case(specs, plan, path):
    hs = [tb.make(sp) for sp in specs]
    calls = []
    for step in plan:
        if step == "reset":
            for h, sp in zip(hs, specs):
                h.set_state(*tb.start_state(sp))
        else:
            _, batched = optimize_batch(hs, step)
            calls.append(snapshot(hs, batched))
    lead = calls[-1][0]
    assert (lead["batch_full_trials"] > 0, lead["batch_iteration_trials"] > 0) == (path == "full", path == "iterations"), (path, lead)
    for h in hs:
        h.close()
    return {"call%d" % c: {"handle%d" % i: d for i, d in enumerate(snap)} for c, snap in enumerate(calls)}


def record(precision):
    return {name: record_case(*case) for name, case in cases(precision).items()}


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit("usage: make_golden_batch_schedule.py OUT.json CSRC_TREE_HASH")
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_batch_schedule.py", "hipcc_version": hipcc, "csrc_tree": sys.argv[2]}
    for precision in PRECISIONS:
        out[precision] = record(precision)
        print(precision, sorted(out[precision]), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

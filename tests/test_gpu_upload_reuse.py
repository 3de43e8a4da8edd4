"""What every upload of the handle-life scripts reuses, pinned by three counters.

The twin tests (tests/test_gpu_handle_life.py) hold a reused handle to a fresh one bit for bit -- and cannot see a handle that has stopped
reusing anything: one that sorts, uploads and analyses afresh at every call still equals its twin.  What is lost then is the time of the
reuse paths (the samples' warm-up + timed protocol, repeated local BA on one window).  So every script of tests/handle_life_scripts.py is
walked here on one live handle, without a twin, in the f64 setting with heuristics = 0, and after every step the deltas of

  value_bytes_uploaded   0 at an upload that kept the sorted values of the previous one
  edge_sorts             0 at an upload that kept the previous sort
  structure_builds       0 at the need() after an upload that kept the structure.  Where the first analysis finds a better pose order
                         (tryReorder) the need() shows one build AND one edge sort -- and shows both AGAIN at a later upload of the
                         same graph if the kept pose order was lost

are compared with tests/golden/upload_reuse.json (tests/golden/make_golden_upload_reuse.py), recorded on the MI355X before
cuba_hip_solver::setGraph was split into a plan (csrc/ba_upload_plan.hpp) and steps.  A Check counts as a step: its run is the need() that builds the structure and ends an open two-step
upload.  A partitioned handle runs nothing at a Check; compute_errors() is its need()."""
import json
import os

import pytest

import handle_life_model as m
import handle_life_scripts as sc
from conftest import ROOT

from cuba_amd.capi import HipSolver

pytestmark = pytest.mark.gpu

COUNTERS = ("value_bytes_uploaded", "edge_sorts", "structure_builds")
GOLDEN = os.path.join(ROOT, "tests", "golden", "upload_reuse.json")


def label(step):
    if isinstance(step, m.Refused):
        return "Refused(%s)" % label(step.step)
    if isinstance(step, m.Upload):
        return "Upload:" + step.form
    if isinstance(step, m.SetOption):
        return "SetOption:" + step.key
    return type(step).__name__


def walk(name):
    """[[label, d value_bytes_uploaded, d edge_sorts, d structure_builds], ...], one row per step of the script"""
    spec = m.Spec(precision="f64", options=dict(heuristics=0))
    live = HipSolver(None, spec.rk, precision="f64", heuristics=0)
    rows = []
    try:
        was = [live.counter(k) for k in COUNTERS]
        for step in sc.script(name):
            m.apply(step, spec, live)
            if isinstance(step, m.Check):
                if spec.partition is not None:
                    live.compute_errors()
                else:
                    live.optimize(step.niter)
                    m.ran(spec, step.niter)
            now = [live.counter(k) for k in COUNTERS]
            rows.append([label(step)] + [int(b - a) for a, b in zip(was, now)])
            was = now
    finally:
        live.close()
    return rows


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_is_not_vacuous(golden):
    """each of the three deltas is zero at some upload and non-zero at some upload; structure_builds is read at the step that builds (the
    need() after the upload: a two-step upload's own build_structure, or the next Check)"""
    assert sorted(golden) == sorted(sc.SCRIPTS)
    uploads = [row for rows in golden.values() for row in rows if row[0].startswith("Upload:")]
    for k in (1, 2, 3):
        assert any(row[k] == 0 for row in uploads) and any(row[k] > 0 for row in uploads), COUNTERS[k - 1]
    # ... and the kept pose order: some step that is no upload both sorts and builds (the order was found), and some upload of the
    # shuffled graph is followed by neither up to its Check (the order was kept)
    assert any(not row[0].startswith("Upload:") and row[2] > 0 and row[3] > 0 for rows in golden.values() for row in rows)
    after, open_ = [], False          # edge sorts + structure builds from an upload of the "orders" script to its Check, both included
    for row in golden["orders"]:
        if row[0].startswith("Upload:"): after.append(0); open_ = True
        if open_: after[-1] += row[2] + row[3]
        if row[0] == "Check": open_ = False
    assert 0 in after and max(after) >= 2, after


@pytest.mark.parametrize("name", sorted(sc.SCRIPTS))
def test_every_upload_reuses_what_it_reused(name, golden):
    want, got = golden[name], walk(name)
    print(name, got)
    assert len(got) == len(want), "%s has %d steps, its golden entry %d: record the golden again on the code it was recorded on" % (name, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s step %d: %r, golden %r (label, %s)" % (name, k, a, b, ", ".join(COUNTERS))

"""The host's schedule of cuba_hip_optimize_batch (csrc/ba_lm.hip) against tests/golden/batch_schedule.json: per handle and per call the
trials, the PCG iterations done and ENQUEUED, the host looks, the coarse refreshes and in-line inversions, the exact and unconverged
solves, the fp32 fall-backs and the iteration history, and for the lead which of the two modes of the batch driver ran how many trial
rounds and how many reduced solves went out batched.  tests/test_gpu_batch.py holds the results of a batch to solo runs bit for bit; that
a batch still enqueues the same iterations and takes the same looks -- what its speed consists of -- is held here.  Every entry is
recomputed by the fixture's own generator (tests/golden/make_golden_batch_schedule.py: record()) and must be EQUAL to the recorded one.

The fixture names the hipcc it was recorded with and the git tree hash of cuda-bundle-adjustment_amd/csrc that the recorded library was
built from.  Iteration counts depend on the arithmetic of the kernels: re-record the fixture with the generator when the toolchain changes
(at a commit whose results are trusted), never to make a source change pass."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_batch_schedule", os.path.join(GOLDEN, "make_golden_batch_schedule.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _leaves(d, prefix=""):
    """nested dict -> {path: leaf}"""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_leaves(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_batch_schedule_is_the_recorded_one(precision):
    with open(os.path.join(GOLDEN, "batch_schedule.json")) as f:
        want = _leaves(json.load(f)[precision])
    got = _leaves(_generator().record(precision))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    for k in differ:
        print(k, "\n  recorded", want[k], "\n  computed", got[k])
    assert not differ

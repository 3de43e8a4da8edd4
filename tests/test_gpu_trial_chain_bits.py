"""The bits of whole device-decided LM runs (cuba_hip_optimize) against tests/golden/trial_chain_bits.json: chi2 series, final state, number
of LM trials and PCG iteration history of runs that take every path of a trial's decision / report / restore chain -- the single-launch
trial tail over 10 iterations and over 1 (a run whose only decision the host waits for), a Tukey start with rejected trials (the restore
between two trials), a landmark with more than 64 observations and pose factors (the tail in several launches), and two runs in a row on
one handle (whatever a run leaves behind on the device for the next) -- on the fp64 and the fp32 library.  Every entry is recomputed by
the fixture's own generator (tests/golden/make_golden_trial_chain.py: record()) and must be EQUAL to the recorded one; every run must end
with late_decision_records == 0 (asserted by the generator's run()).

The fixture was recorded at the commit before the run start moved onto the device, the decision's publish became conditional and the restore
moved into the landmark pass: changes to launches, copies, fences and host calls must leave it alone.  It names the hipcc it was recorded
with; re-record it with the generator when the toolchain changes (at a commit whose results are trusted), never to make a source change
pass."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_trial_chain", os.path.join(GOLDEN, "make_golden_trial_chain.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _leaves(d, prefix=""):
    """nested dict -> {path: leaf}; a {"sha256", "len"} record of an array is a leaf"""
    out = {}
    for k, v in d.items():
        if isinstance(v, dict) and "sha256" not in v:
            out.update(_leaves(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_lm_runs_are_bit_identical_to_the_recorded_ones(precision):
    with open(os.path.join(GOLDEN, "trial_chain_bits.json")) as f:
        golden = json.load(f)[precision]
    want = _leaves(golden["runs"])
    got = _leaves(_generator().record(precision, golden["rejected_end_niter"]))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    for k in differ:
        print(k, "\n  recorded", want[k], "\n  computed", got[k])
    assert not differ

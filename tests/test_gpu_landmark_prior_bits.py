"""The bits of the landmark-prior code (csrc/ba_factor.hip, the prior forms of the landmark passes in csrc/ba_linearize.hip) and of the
big-landmark pass without priors against tests/golden/landmark_priors_bits.json: the landmark systems of both passes, the Schur complement,
the objective, the per-prior chi2 (a set past the chi2 kernel's grid included), LM trajectories (device-decision and host loop, a run with
rejected trials, a graph with landmarks of more than 64 and of more than 256 observations with and without priors) and the final states,
on the fp64 library, the fp32 library and the fp64 library with mixed_precision=1.  Every entry is recomputed by the fixture's own
generator (tests/golden/make_golden_landmark_priors.py: record()) and must be EQUAL to the recorded one: the tests against the numpy model
hold at 1e-12 / 1e-6 and cannot show that a change meant to leave the results alone did so.

The fixture names the hipcc it was recorded with.  Another compiler may order the arithmetic of the kernels differently: re-record the
fixture with the generator when the toolchain changes (at a commit whose results are trusted), never to make a source change pass."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_golden_landmark_priors", os.path.join(GOLDEN, "make_golden_landmark_priors.py"))
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


@pytest.mark.parametrize("config", ["f64", "f32", "f64_mixed"])
def test_landmark_prior_results_are_bit_identical_to_the_recorded_ones(generator, config):
    with open(os.path.join(GOLDEN, "landmark_priors_bits.json")) as f:
        want = _leaves(json.load(f)[config])
    got = _leaves(generator.record(config))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    for k in differ:
        print(k, "\n  recorded", want[k], "\n  computed", got[k])
    assert not differ

"""The bits of the factor code (csrc/ba_factor.hip) against tests/golden/factor_kinds_bits.json, for what the fixtures of
tests/test_gpu_pose_factor_bits.py and tests/test_gpu_landmark_prior_bits.py leave out: position factors and direction factors (each kind
alone, without and with robust kernels), pose priors and relative-pose edges with robust kernels (the kernels' ROBUST = true
instantiations), all five kinds on one handle (the launch order, the sums across kinds into the same diagonal blocks), sets with several
chi2 workgroups per kind (every offset into the partials buffer is non-trivial; 16 385 direction factors send the chi2 kernel's
grid-stride loop on a second trip) and a graph whose pose ids are shuffled, on the fp64 and the fp32 library.  Every entry is recomputed by the
fixture's own generator (tests/golden/make_golden_factor_kinds.py: record()) and must be EQUAL to the recorded one: the tests against the
numpy models hold at 1e-12 / 1e-6 and cannot show that a change meant to leave the results alone did so.

The fixture names the hipcc it was recorded with.  Another compiler may order the arithmetic of the kernels differently: re-record the
fixture with the generator when the toolchain changes (at a commit whose results are trusted), never to make a source change pass."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_factor_kinds", os.path.join(GOLDEN, "make_golden_factor_kinds.py"))
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
def test_factor_kind_results_are_bit_identical_to_the_recorded_ones(precision):
    with open(os.path.join(GOLDEN, "factor_kinds_bits.json")) as f:
        want = _leaves(json.load(f)[precision])
    got = _leaves(_generator().record(precision))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    for k in differ:
        print(k, "\n  recorded", want[k], "\n  computed", got[k])
    assert not differ

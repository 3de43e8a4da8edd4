"""The bits of the two range kinds of the factor code (csrc/ba_factor.hip) against tests/golden/range_kinds_bits.json, which
tests/test_gpu_factor_kinds_bits.py (five kinds) leaves out: range factors on a pose and range factors between two poses, each alone
without and with robust kernels, the pose-range factors next to relative-pose edges on the same blocks (the binary kinds' store-or-add
rule, the edges set before and after), gathers of both binary kinds over several workgroups, all seven kinds on one handle (the launch
order), sets with several chi2 workgroups for the two kinds and a 200-pose graph that the library renumbers, on the fp64 and the fp32
library.  Every entry is recomputed by the fixture's own generator (tests/golden/make_golden_range_kinds.py: record()) and must be EQUAL
to the recorded one: the tests against the numpy models hold at 1e-12 / 1e-6 and cannot show that a change meant to leave the results
alone did so.

The fixture names the hipcc it was recorded with and the git tree hash of cuda-bundle-adjustment_amd/csrc that the recorded library was
built from.  Another compiler may order the arithmetic of the kernels differently: re-record the fixture with the generator when the
toolchain changes (at a commit whose results are trusted), never to make a source change pass."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_range_kinds", os.path.join(GOLDEN, "make_golden_range_kinds.py"))
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
def test_range_kind_results_are_bit_identical_to_the_recorded_ones(precision):
    with open(os.path.join(GOLDEN, "range_kinds_bits.json")) as f:
        want = _leaves(json.load(f)[precision])
    got = _leaves(_generator().record(precision))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    for k in differ:
        print(k, "\n  recorded", want[k], "\n  computed", got[k])
    assert not differ

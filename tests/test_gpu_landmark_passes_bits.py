"""The bits of the kernels that walk the reprojection edges landmark by landmark (csrc/ba_edge.hip: chi2, back substitution, trial tail;
csrc/ba_linearize.hip: the landmark pass), wave form and workgroup form, against tests/golden/landmark_passes_bits.json: the per-edge chi2,
the landmark systems of both modes, the reduced system, xp, the step API's xl and gain-ratio denominator, the updated state and its
objective, and a three-iteration cuba_hip_optimize (chi2 series, state, number of trials) -- on a graph with one free landmark of 65 to 256
edges, on one with free landmarks of more than 256 edges (the workgroup's strided loop makes more than one trip) and on that one with its
largest landmark fixed, on the fp64 library, the fp32 library and the fp64 library with mixed_precision=1.  Every entry is recomputed by
the fixture's own generator (tests/golden/make_golden_landmark_passes.py: record()) and must be EQUAL to the recorded one.

The fixture was recorded at the commit before the wave and workgroup kernels were folded onto shared device helpers.  It names the hipcc
it was recorded with; re-record it with the generator when the toolchain changes (at a commit whose results are trusted), never to make a
source change pass."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_golden_landmark_passes", os.path.join(GOLDEN, "make_golden_landmark_passes.py"))
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


@pytest.mark.parametrize("graph", ["g40_big", "big", "big_fixed"])
@pytest.mark.parametrize("config", ["f64", "f32", "f64_mixed"])
def test_landmark_passes_are_bit_identical_to_the_recorded_ones(generator, config, graph):
    with open(os.path.join(GOLDEN, "landmark_passes_bits.json")) as f:
        want = _leaves(json.load(f)[config][graph])
    got = _leaves(generator.record(config, graph))
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k] != want[k]]
    for k in differ:
        print(k, "\n  recorded", want[k], "\n  computed", got[k])
    assert not differ

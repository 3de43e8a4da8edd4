"""Generates tests/golden/range_kinds_bits.json: the exact bits of what the solver computes with the two range kinds, which
factor_kinds_bits.json (five kinds) leaves out -- range factors on a pose and range factors between two poses, each alone without and with
robust kernels, the pose-range factors next to relative-pose edges on the same blocks (the store-or-add rule of the binary kinds' gathers,
the edges set before and after the factors), sets whose gather spans several workgroups with the boundary between block numbers and pose
numbers inside a later one (pose-range factors, relative-pose edges, and both), all seven kinds on one handle, sets with several chi2
workgroups for the two new kinds, and a 200-pose graph that the library renumbers -- on the fp64 and the fp32 library.  For every case:
hsc / bp / bsc after build_system(); assemble() (mode 0) and after set_lambda(0); schur() (mode 1), compute_errors, the per-factor chi2 of
every kind present, optimize(10) with the final state, and the host loop (profile=1).  Doubles are stored as float.hex() strings, arrays as
the sha256 of their bytes plus their length.  tests/test_gpu_range_kinds_bits.py recomputes every entry through record() below and asserts
equality: the fixture pins a change that must leave the results alone (a refactor of the factor code) to the commit it was recorded at.

(pose_factors_bits.json was not sized for the gather's geometry: its edges sit on 4 blocks and 8 free poses -- 144 block numbers + 216 pose
numbers, so the boundary between the two index spaces lies inside the first workgroup and mode 0 fits one workgroup.  The
gather_two_workgroups cases here cover the edges' gather at 11 blocks and 14 poses.)

Needs the GPU; re-record when the toolchain changes (the fixture names the hipcc it was built with and the git tree hash of
cuda-bundle-adjustment_amd/csrc that the recorded library was built from), never to make a source change pass.  Run from the repo root:
`python tests/golden/make_golden_range_kinds.py OUT.json $(git rev-parse HEAD:cuda-bundle-adjustment_amd/csrc)`."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import direction_factor_reference as dr  # noqa: E402
import landmark_prior_reference as lr  # noqa: E402
import pose_range_factor_reference as pp  # noqa: E402
import position_factor_reference as pfr  # noqa: E402
import range_factor_reference as rr  # noqa: E402
import robust_pose_factor_reference as rb  # noqa: E402
from conftest import RK_HUBER  # noqa: E402
from test_gpu_configs import shuffled_pose_ids  # noqa: E402
from test_gpu_pose_priors import make_priors  # noqa: E402
from test_gpu_pose_range_factors import assembly_pairs  # noqa: E402
from test_gpu_relative_pose import covisible, internal_position, make_rel, split_pairs  # noqa: E402
from test_pose_range_factor_reference import main_set as pose_range_main_set, with_kernel  # noqa: E402
from test_range_factor_reference import DELTAS, main_set as range_main_set  # noqa: E402

from cuba_amd.capi import HipSolver  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402

PRECISIONS = ("f64", "f32")
# many_parts: factors of the two range kinds, each a different multiple of the chi2 workgroup (256) plus something
MANY = dict(rng=300, prng=600)
MANY_ITERATIONS = 3
CHI = {"priors": "prior", "rel": "relative_pose", "lmp": "landmark_prior", "pos": "position_factor", "dir": "direction_factor", "rng": "range_factor",
       "prng": "pose_range_factor"}


def arr(a):
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "len": int(a.size)}


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def cycling(s):
    """a set with the kernels none / Huber / Tukey / Cauchy in turn, the sibling tests' deltas (kind, delta: the last two entries)"""
    kind = (np.arange(len(s[0])) % 4).astype(np.int32)
    return s[:-2] + (kind, np.array([DELTAS[int(k)] for k in kind]))


@functools.lru_cache(maxsize=None)
def g40():
    return flatten(synth_ba(40, 600, 2400, seed=1))


@functools.lru_cache(maxsize=None)
def g40_two_fixed():
    """the 40-pose graph with a second fixed pose: a factor between two poses can have both ends fixed"""
    g = synth_ba(40, 600, 2400, seed=1)
    g.pose_fixed[:2] = True
    fp = flatten(g)
    assert fp.Pt - fp.Pf == 2
    return fp


@functools.lru_cache(maxsize=None)
def shuffled200():
    return flatten(shuffled_pose_ids(synth_ba(200, 3000, 12000, seed=2), seed=1))


def two_workgroup_pairs(fp):
    """a chain over 10 free poses in alternating orientation (9 blocks with Schur products or without, as the graph has it) and two
    blocks without products on four more poses: 11 blocks, 14 poses.  Mode 1: 396 block numbers, so the boundary to the 378 pose numbers
    lies inside the second workgroup of 256; mode 0: the pose numbers alone take two workgroups"""
    have = covisible(fp)
    chain = [(k, k + 1) if k % 2 else (k + 1, k) for k in range(10, 19)]
    extra = [[(a, b) for b in range(a + 1, fp.Pf) if (a, b) not in have and b >= 20 and b % 2 == a % 2][0] for a in (0, 1)]
    pairs = chain + [extra[0], (extra[1][1], extra[1][0])]
    blocks = {(min(a, b), max(a, b)) for a, b in pairs}
    poses = {p for pair in pairs for p in pair}
    assert len(extra) == 2 and all(p < fp.Pf for p in poses)
    assert len(blocks) >= 8 and len(poses) >= 10 and 36 * len(blocks) > 256 and (36 * len(blocks)) % 256 and 27 * len(poses) > 256
    return pairs


def all_seven(fp):
    """the sets of tests/test_gpu_pose_range_factors.py::test_all_seven_kinds_on_one_handle, set in its order"""
    return dict(rel_last=True, prng=pose_range_main_set(fp, rb.CAUCHY), priors=make_priors(fp, [1, 5, 17], seed=1), rel=make_rel(fp, [(3, 20), (9, 3)], seed=2),
                lmp=lr.make_priors(fp, [4, 100, 333, 333], seed=3, kind=rb.HUBER, delta=2.0),
                pos=pfr.make_factors(fp, [5, 8, 22], seed=4, kind=rb.HUBER, delta=2.0), dir=dr.make_factors(fp, [5, 9, 30], seed=5, kind=rb.HUBER, delta=2.0),
                rng=rr.make_factors(fp, [5, 3, 12], seed=6, kind=rb.HUBER, delta=2.0))


def names_twice_and_fixed(fp, poses):
    poses = np.asarray(poses).ravel()
    return len(poses) != len(set(poses.tolist())) and (poses >= fp.Pf).any()


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (graph, the sets of a handle: priors, rel, lmp, pos, dir, rng, prng; rel_last: the edges are set behind the factors)"""
    fp, fp2 = g40(), g40_two_fixed()
    out = {
        "range": (fp, dict(rng=range_main_set(fp))),
        "range_robust": (fp, dict(rng=cycling(range_main_set(fp)))),
    }
    for name in ("range", "range_robust"):
        assert names_twice_and_fixed(fp, out[name][1]["rng"][0])
    # the assembly_pairs set (tests/test_gpu_pose_range_factors.py) and one factor with both ends fixed
    near, far, pairs = assembly_pairs(fp2)
    pairs = pairs + [(fp2.Pt - 2, fp2.Pt - 1)]
    s = pp.make_factors(fp2, pairs, seed=6)
    out["pose_range"] = (fp2, dict(prng=s))
    out["pose_range_robust"] = (fp2, dict(prng=cycling(s)))
    pi, pj = s[0], s[1]
    both, one = (pi >= fp2.Pf) & (pj >= fp2.Pf), (pi >= fp2.Pf) ^ (pj >= fp2.Pf)
    assert both.sum() == 1 and (pi[one] >= fp2.Pf).any() and (pj[one] >= fp2.Pf).any()          # (a fixed end in either seat)
    assert set(pi[~both & ~one].tolist()) & set(pj[~both & ~one].tolist())                      # (a pose that is i in one factor and j in another)
    # the sets of test_assembled_system_next_to_relative_pose_edges: a block both gathers write, one of the edges alone, one of the ranges alone
    near, far, pairs = assembly_pairs(fp)
    edges = make_rel(fp, [far[0], near[1], (far[2][1], far[2][0])], seed=2)
    s = with_kernel(pp.make_factors(fp, pairs + [near[1]], seed=7), rb.CAUCHY)
    out["pose_range_next_to_edges_first"] = (fp, dict(rel=edges, prng=s))
    out["pose_range_next_to_edges_last"] = (fp, dict(rel=edges, prng=s, rel_last=True))
    # the gathers at more than one workgroup: the factors alone, relative-pose edges on the same pairs alone, and both (every block added to)
    pairs = two_workgroup_pairs(fp)
    s, edges = cycling(pp.make_factors(fp, pairs, seed=8)), make_rel(fp, pairs, seed=9)
    out["gather_two_workgroups"] = (fp, dict(prng=s))
    out["gather_two_workgroups_edges"] = (fp, dict(rel=edges))
    out["gather_two_workgroups_both"] = (fp, dict(rel=edges, prng=s))
    out["all_seven"] = (fp, all_seven(fp))
    for name in ("range_robust", "pose_range_robust", "gather_two_workgroups"):
        sets = out[name][1]
        assert sorted(set((sets["rng"] if "rng" in sets else sets["prng"])[-2].tolist())) == [0, 1, 2, 3]
    return out


@functools.lru_cache(maxsize=None)
def many_parts():
    """the two range kinds with more than one chi2 workgroup each (the poses and pairs of their main sets repeated, with fresh seeded values,
    kernels in turn) next to the other five kinds at their small sizes"""
    fp = g40()
    out = all_seven(fp)
    pairs = np.stack(pose_range_main_set(fp)[:2], axis=1)
    out["rng"] = cycling(rr.make_factors(fp, np.resize(range_main_set(fp)[0], MANY["rng"]), seed=26))
    out["prng"] = cycling(pp.make_factors(fp, pairs[np.arange(MANY["prng"]) % len(pairs)], seed=27))
    sizes = [len(out[k][0]) for k in ("rng", "prng")]
    assert sizes == [300, 600] and all(n > 256 and n % 256 for n in sizes)
    return out


def shuffled200_sets():
    """the pairs of tests/test_gpu_pose_range_factors.py::test_assembled_system_with_shuffled_pose_ids"""
    fp = shuffled200()
    near, far = split_pairs(fp, 3, 3)
    pairs = [near[0], far[0], (far[0][1], far[0][0]), (far[1][1], far[1][0]), far[2], (near[1][1], near[1][0]), (near[0][1], near[0][0]), (near[2][0], fp.Pt - 1)]
    return pairs, dict(rel=make_rel(fp, [far[2], near[0]], seed=4), prng=with_kernel(pp.make_factors(fp, pairs, seed=3), rb.HUBER))


def handle(fp, precision, sets, **opts):
    h = HipSolver(fp, RK_HUBER, precision=precision, **opts)
    last = sets.get("rel_last", False)
    if "rel" in sets and not last:
        h.set_relative_pose_edges(*sets["rel"])
    if "prng" in sets:
        h.set_pose_range_factors(*sets["prng"])
    if "priors" in sets:
        h.set_pose_priors(*sets["priors"])
    if "rel" in sets and last:
        h.set_relative_pose_edges(*sets["rel"])
    if "lmp" in sets:
        h.set_landmark_priors(*sets["lmp"])
    if "pos" in sets:
        h.set_position_factors(*sets["pos"])
    if "dir" in sets:
        h.set_direction_factors(*sets["dir"])
    if "rng" in sets:
        h.set_range_factors(*sets["rng"])
    return h


def chi_squares(h, sets):
    return {CHI[k] + "_chi_squares": getattr(h, CHI[k] + "_chi_squares")() for k in CHI if k in sets}


def record_case(fp, precision, sets):
    out = {}
    for mode in (0, 1):
        h = handle(fp, precision, sets)
        if mode == 0:
            h.build_system()
            h.assemble()
        else:
            h.set_lambda(0.0)
            h.schur()
        out["mode%d" % mode] = {"hsc": arr(h.hsc()[2]), "bp": arr(h.array("bp")), "bsc": arr(h.array("bsc"))}
    out["compute_errors"] = float(h.compute_errors()).hex()
    for name, chi in chi_squares(h, sets).items():
        out[name] = hexes(chi)
    h = handle(fp, precision, sets)
    out["optimize"] = hexes(h.optimize(10)["chi2"])
    q, t, X = h.state()
    out["q"], out["t"], out["Xw"] = arr(q), arr(t), arr(X)
    out["optimize_host_loop"] = hexes(handle(fp, precision, sets, profile=1).optimize(10)["chi2"])
    return out


def record_many_parts(precision):
    sets = many_parts()
    h = handle(g40(), precision, sets)
    out = {"compute_errors": float(h.compute_errors()).hex()}
    for name, chi in chi_squares(h, sets).items():
        out[name] = arr(chi)
    out["optimize"] = hexes(h.optimize(MANY_ITERATIONS)["chi2"])
    return out


def record_shuffled200(precision):
    fp = shuffled200()
    pairs, sets = shuffled200_sets()
    h = handle(fp, precision, sets)
    out = {"optimize": hexes(h.optimize(10)["chi2"])}
    pos = internal_position(h, fp.Pf)
    assert not np.array_equal(pos, np.arange(fp.Pf))                  # (the renumbering took place)
    flipped = [pos[i] > pos[j] for i, j in pairs[:-1]]
    assert any(flipped) and not all(flipped)
    return out


def record(precision):
    out = {name: record_case(fp, precision, sets) for name, (fp, sets) in cases().items()}
    out["many_parts"] = record_many_parts(precision)
    out["shuffled200"] = record_shuffled200(precision)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit("usage: make_golden_range_kinds.py OUT.json CSRC_TREE_HASH")
    hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()[:2]          # (HIP and clang versions)
    out = {"generator": "tests/golden/make_golden_range_kinds.py", "hipcc_version": hipcc, "csrc_tree": sys.argv[2], "iterations": 10,
           "many_parts_iterations": MANY_ITERATIONS}
    for precision in PRECISIONS:
        out[precision] = record(precision)
        print(precision, out[precision]["all_seven"]["optimize"][-1], out[precision]["many_parts"]["optimize"][-1],
              out[precision]["shuffled200"]["optimize"][-1], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

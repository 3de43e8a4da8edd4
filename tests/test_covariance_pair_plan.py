"""Symbolic phase of the covariance pairs (csrc/ba_covariance_pairs.hip: pair_pack + pair_plan -- right-hand-side blocks, the forward and
backward column sets of every block, per-level work lists and restricted gather lists), checked on the CPU against a Python model built
from the exact solver's plan (capi.sparse_plan): every set must be the union of the elimination tree's root-ward chains (parent = first
off-diagonal row of a column) of the segments the block's right-hand side touches / its pairs' left sides read, closed under the rows of
a column, and every gather list ascending and restricted to its set.  No GPU involved: the C-ABI hook runs on the host."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_sparse_plan import CASES, _malformed_patterns, band_pattern  # noqa: E402

from cuba_amd.capi import CubaHipError, pair_plan, sparse_plan  # noqa: E402

PATTERNS = dict(CASES, trajectory_1000=lambda: band_pattern(1000, 18, closures=[(0, 770, 230)]))


def _pairs(P, rng, n):
    """random pose pairs plus the ones that matter: a pose with itself, the first against the last, the first against every pose"""
    pr = [(int(a), int(b)) for a, b in rng.integers(0, P, size=(n, 2))]
    pr += [(0, 0), (0, P - 1), (P - 1, 0)] + [(0, j) for j in range(0, P, max(1, P // 20))]
    return pr


def _model(plan, pairs):
    T = plan["T"]
    colPtr, rowIdx, pos = plan["colPtr"], plan["rowIdx"], plan["posOfSeg"]
    parent = [int(rowIdx[colPtr[j] + 1]) if colPtr[j + 1] - colPtr[j] > 1 else -1 for j in range(T)]

    def chains(starts):
        out = set()
        for j in starts:
            while j >= 0 and j not in out:
                out.add(j)
                j = parent[j]
        return sorted(out)

    segs = sorted({j // 5 for _, j in pairs}, key=lambda s: pos[s])
    block_of_seg = {s: b for b, s in enumerate(segs)}
    left = [set() for _ in segs]
    for i, j in pairs:
        left[block_of_seg[j // 5]].add(int(pos[i // 5]))
    fwd = [chains([int(pos[s])]) for s in segs]
    bwd = [chains(sorted(lf)) for lf in left]
    return block_of_seg, fwd, bwd


def _check(plan, pp, pairs):
    T, L = plan["T"], plan["nLevels"]
    colPtr, rowIdx = plan["colPtr"], plan["rowIdx"]
    block_of_seg, fwd, bwd = _model(plan, pairs)
    nb = len(fwd)
    assert pp["blocks"] == nb
    # pairs: the block of the right pose's segment, the pose's own columns in it
    got = pp["pairs"].reshape(-1, 4)
    for k, (i, j) in enumerate(pairs):
        assert got[k, 0] == block_of_seg[j // 5] and got[k, 1] == 6 * (j % 5), (k, i, j, got[k])
    # the sets: exactly the model's chains
    for b in range(nb):
        f = pp["fwdCols"][pp["fwdPtr"][b]:pp["fwdPtr"][b + 1]].tolist()
        w = pp["bwdCols"][pp["bwdPtr"][b]:pp["bwdPtr"][b + 1]].tolist()
        assert f == fwd[b], (b, f, fwd[b])
        assert w == bwd[b], (b, w, bwd[b])
        for s in (f, w):               # closed under the rows of a column
            ss = set(s)
            for j in s:
                assert set(rowIdx[colPtr[j] + 1:colPtr[j + 1]].tolist()) <= ss, (b, j)
        assert pp["slotCols"][pp["slotPtr"][b]:pp["slotPtr"][b + 1]].tolist() == sorted(set(f) | set(w))
    assert pp["slots"] == len(pp["slotCols"]) == pp["slotPtr"][-1]
    slot_block = np.repeat(np.arange(nb), np.diff(pp["slotPtr"]))
    slot_col = pp["slotCols"]
    level = np.zeros(T, dtype=int)
    for lv in range(L):
        level[plan["lvlCols"][plan["lvlColPtr"][lv]:plan["lvlColPtr"][lv + 1]]] = lv
    tile_of = {}
    for k in range(T):
        for t in range(colPtr[k] + 1, colPtr[k + 1]):
            tile_of[(int(rowIdx[t]), k)] = t
    # forward work: one record per (block, forward column), on its level (ascending), gather = the tiles (j, k), k in the set, ascending
    fr, fg = pp["fRec"].reshape(-1, 4), pp["fGather"].reshape(-1, 2)
    assert len(pp["fLvlPtr"]) == L + 1 and pp["fLvlPtr"][-1] == len(fr) == pp["fRecords"]
    seen = set()
    for lv in range(L):
        recs = fr[pp["fLvlPtr"][lv]:pp["fLvlPtr"][lv + 1]]
        assert [(slot_block[r[0]], r[1]) for r in recs] == sorted((slot_block[r[0]], r[1]) for r in recs)
        for slot, j, g0, n in recs:
            b = slot_block[slot]
            assert slot_col[slot] == j and level[j] == lv and (b, j) not in seen
            seen.add((b, j))
            fs = set(fwd[b])
            want = [(tile_of[(j, k)], k) for k in range(j) if (j, k) in tile_of and k in fs]
            ent = fg[g0:g0 + n]
            assert [(int(t), int(slot_col[s])) for t, s in ent] == want, (b, j)
            assert all(slot_block[s] == b for _, s in ent)
    assert seen == {(b, j) for b in range(nb) for j in fwd[b]}
    # backward work: levels descending, gather = every row of column j (in the set by closure), ascending
    br, bg = pp["bRec"].reshape(-1, 4), pp["bGather"].reshape(-1, 2)
    assert len(pp["bLvlPtr"]) == L + 1 and pp["bLvlPtr"][-1] == len(br) == pp["bRecords"]
    seen = set()
    for s in range(L):
        lv = L - 1 - s
        for slot, j, g0, n in br[pp["bLvlPtr"][s]:pp["bLvlPtr"][s + 1]]:
            b = slot_block[slot]
            assert slot_col[slot] == j and level[j] == lv and (b, j) not in seen
            seen.add((b, j))
            ent = bg[g0:g0 + n]
            assert [int(t) for t, _ in ent] == list(range(colPtr[j] + 1, colPtr[j + 1]))
            assert [int(slot_col[x]) for _, x in ent] == rowIdx[colPtr[j] + 1:colPtr[j + 1]].tolist()
            assert all(slot_block[x] == b for _, x in ent)
    assert seen == {(b, j) for b in range(nb) for j in bwd[b]}


@pytest.mark.parametrize("slack", [-1, 0, 4, 8])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_pair_plan_matches_the_model(name, slack):
    rp, ci = PATTERNS[name]()
    P = len(rp) - 1
    rng = np.random.default_rng(P + slack)
    pairs = _pairs(P, rng, 40)
    plan = sparse_plan(rp, ci, slack=slack)
    pp = pair_plan(rp, ci, pairs, slack=slack)
    _check(plan, pp, pairs)
    again = pair_plan(rp, ci, pairs, slack=slack)
    assert all(np.array_equal(pp[k], again[k]) for k in pp if isinstance(pp[k], np.ndarray))


def test_pair_plan_walks_paths_not_the_tree():
    """The point of the restriction: on the 1000-pose lap a pair costs a root-ward path forward and one backward, far fewer columns than
    the tree; "pose 0 against every pose" walks the whole tree backward for pose 0's block only."""
    rp, ci = PATTERNS["trajectory_1000"]()
    plan = sparse_plan(rp, ci, slack=4)
    T = plan["T"]
    pp = pair_plan(rp, ci, [(0, 999)], slack=4)
    # (a chain holds one column per level at most)
    assert pp["blocks"] == 1 and pp["fRecords"] <= plan["nLevels"] and pp["bRecords"] <= plan["nLevels"] < T // 2, (pp["fRecords"], pp["bRecords"], T)
    pp = pair_plan(rp, ci, [(i, 0) for i in range(1000)], slack=4)
    assert pp["blocks"] == 1 and pp["bRecords"] == T


def test_pair_plan_refuses_malformed_input():
    rp, ci = CASES["band_loop_closure"]()
    P = len(rp) - 1
    for name, r, c in _malformed_patterns():
        with pytest.raises(CubaHipError, match="status 1"):
            pair_plan(r, c, [(0, 1)])
    for bad in ([(-1, 0)], [(0, -1)], [(P, 0)], [(0, P)], [(3, 1 << 20)]):
        with pytest.raises(CubaHipError, match="status 1"):
            pair_plan(rp, ci, bad)
    pp = pair_plan(rp, ci, [(0, P - 1)])
    _check(sparse_plan(rp, ci), pp, [(0, P - 1)])

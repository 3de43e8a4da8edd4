"""Symbolic phase of the selected inversion behind the marginal covariances (csrc/ba_direct.hip: selinv_plan -- gather lists of the
Takahashi recurrence on the exact solver's factor pattern, steps walking the elimination tree's levels from the top down), checked on
the CPU: a matrix is inverted THROUGH the plan by a numpy restatement of the numeric kernels (tests/selinv_emulator.py) and compared
with LAPACK on the factor's pattern.  No GPU involved: the C-ABI hook runs on the host."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from selinv_emulator import TP, TS, factor_tiles, permuted_dense, selected_inverse  # noqa: E402
from sparse_chol_emulator import random_spd_blocks  # noqa: E402
from test_sparse_plan import CASES  # noqa: E402

from cuba_amd.capi import selinv_plan, sparse_plan  # noqa: E402


@pytest.mark.parametrize("slack", [-1, 0, 4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_selected_inverse_through_the_plan(name, slack):
    row_ptr, col_ind = CASES[name]()
    plan = sparse_plan(row_ptr, col_ind, slack=slack)
    sel = selinv_plan(row_ptr, col_ind, slack=slack)
    P = len(row_ptr) - 1
    T, nT = plan["T"], plan["nTiles"]
    colPtr, rowIdx = plan["colPtr"], plan["rowIdx"]
    # shape of the plan: every off-diagonal tile once, every column once, steps = levels top-down
    assert sel["nLevels"] == plan["nLevels"] and len(sel["stepPtr"]) == plan["nLevels"] + 1
    rec = sel["offRec"].reshape(-1, 4)
    assert sel["nOff"] == nT - T and sorted(rec[:, 0].tolist()) == sorted(set(range(nT)) - set(colPtr[:-1].tolist()))
    assert sorted(sel["cols"].tolist()) == list(range(T))
    level = np.zeros(T, dtype=int)
    for lv in range(plan["nLevels"]):
        level[plan["lvlCols"][plan["lvlColPtr"][lv]:plan["lvlColPtr"][lv + 1]]] = lv
    for s in range(sel["nLevels"]):
        lv = sel["nLevels"] - 1 - s
        assert all(level[j] == lv for j in sel["cols"][sel["colStepPtr"][s]:sel["colStepPtr"][s + 1]])
        for t, j, g0, n in rec[sel["stepPtr"][s]:sel["stepPtr"][s + 1]]:
            assert level[j] == lv and colPtr[j] < t < colPtr[j + 1] and n == colPtr[j + 1] - colPtr[j] - 1
            # every needed tile exists, on a higher level, with the right orientation
            i = rowIdx[t]
            for ts, tu in sel["gather"].reshape(-1, 2)[g0:g0 + n]:
                tile, tr = ts & 0x3fffffff, ts >> 30
                k = rowIdx[tu]
                a, b = (k, i) if tr else (i, k)
                assert a >= b and rowIdx[tile] == a and colPtr[b] <= tile < colPtr[b + 1]
                assert tr == (i < k) and level[b] > level[j]
    assert sel["entries"] == sum(int(n) for n in rec[:, 3])
    # the numbers: Sigma on the pattern = inv(A) there
    rng = np.random.default_rng(len(col_ind) + 7)
    A = random_spd_blocks(row_ptr, col_ind, rng)
    Ap, idx = permuted_dense(plan, P, A)
    sigma = selected_inverse(plan, sel, factor_tiles(plan, Ap))
    ref = np.linalg.inv(Ap)
    scale = np.abs(ref).max()
    for j in range(T):
        for t in range(colPtr[j], colPtr[j + 1]):
            i = rowIdx[t]
            want = ref[TS * i:TS * i + TS, TS * j:TS * j + TS]
            assert np.abs(sigma[t] - want).max() <= 1e-10 * scale, (name, slack, t)
    # ... and in the caller's blocks (the map the device extraction uses: blkTile, bit 30 = transposed)
    Ainv = np.linalg.inv(A)
    for bi in range(P):
        for kk in range(row_ptr[bi], row_ptr[bi + 1]):
            bj = col_ind[kk]
            tt = int(plan["blkTile"][kk]); tile, tr = tt & 0x3fffffff, tt >> 30
            li, lj = 6 * (bi % TP), 6 * (bj % TP)
            blk = sigma[tile][li:li + 6, lj:lj + 6] if tr else sigma[tile][lj:lj + 6, li:li + 6].T
            assert np.abs(blk - Ainv[6 * bi:6 * bi + 6, 6 * bj:6 * bj + 6]).max() <= 1e-10 * np.abs(Ainv).max()
    # deterministic: a function of the pattern
    again = selinv_plan(row_ptr, col_ind, slack=slack)
    assert all(np.array_equal(sel[k], again[k]) for k in sel if isinstance(sel[k], np.ndarray))


def test_sparse_plan_arrays_unchanged_by_the_selinv_plan():
    """the covariance's plan is built on top of the exact solver's and leaves its arrays as they were"""
    row_ptr, col_ind = CASES["two_closures"]()
    before = sparse_plan(row_ptr, col_ind, slack=-1)
    selinv_plan(row_ptr, col_ind, slack=-1)
    after = sparse_plan(row_ptr, col_ind, slack=-1)
    assert before.keys() == after.keys()
    assert all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k] for k in before)

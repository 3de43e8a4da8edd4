"""The selected inversion behind the marginal covariances (csrc/ba_covariance.hip: selinv_diag_inverse_kernel, selinv_u_kernel,
selinv_off_level_kernel, selinv_diag_level_kernel, selinv_extract_kernel) run on given matrices through the test hook
cuba_hip_debug_selected_inverse (capi.selected_inverse), against numpy's fp64 inverse of the very matrix handed over: the patterns where
tile code breaks (no off-diagonal tile, one padded tile, deep elimination trees from loop closures, every multiple-elimination slack),
block magnitudes over six decades, dense matrices of condition 1e8, a non-positive pivot, and the hook against a solver handle's own
covariance.  tests/test_selinv_plan.py checks the symbolic plan on the CPU through a numpy restatement of these kernels."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from sparse_chol_emulator import random_spd_blocks  # noqa: E402
from test_gpu_covariance import _dense_from_upper, _record, small_fp  # noqa: E402
from test_sparse_plan import CASES, band_pattern  # noqa: E402

from conftest import RK_HUBER  # noqa: E402
from cuba_amd.capi import CubaHipError, HipSolver, selected_inverse  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = dict(CASES, trajectory_1000=lambda: band_pattern(1000, 18, closures=[(0, 770, 230)]))
CLOSURES = ("band_loop_closure", "two_closures", "trajectory_1000")


@functools.lru_cache(maxsize=None)
def _system(name):
    rp, ci = PATTERNS[name]()
    A = random_spd_blocks(rp, ci, np.random.default_rng(len(ci)))
    return rp, ci, A, np.linalg.inv(A)


def pattern_errors(sigma, Ainv, rp, ci):
    """(max over the pattern's blocks and their mirrors of |got - want|_max / |want|_max, mask of those blocks)"""
    P = len(rp) - 1
    on = np.zeros((P, P), bool)
    err = 0.0
    for i in range(P):
        for k in range(rp[i], rp[i + 1]):
            j = ci[k]
            on[i, j] = on[j, i] = True
            for a, b in ((i, j), (j, i)):
                want = Ainv[6 * a:6 * a + 6, 6 * b:6 * b + 6]
                err = max(err, np.abs(sigma[6 * a:6 * a + 6, 6 * b:6 * b + 6] - want).max() / np.abs(want).max())
    return err, np.kron(on, np.ones((6, 6), bool))


@pytest.mark.parametrize("slack", [-1, 0, 4, 8])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_selected_inverse_on_sparse_patterns(name, slack):
    """Every pattern block of A^-1 to the emulator's 1e-10, exact zeros off the pattern, an exactly symmetric result (the diagonal tiles'
    mirror and the extraction's transposed tiles are the kernels' own), bit-reproducible; the block-diagonal pattern has no off-diagonal
    tile at all (selinv_u_kernel and selinv_off_level_kernel never launch), the closures give trees of more than one level."""
    rp, ci, A, Ainv = _system(name)
    sigma, bad, st = selected_inverse(A, slack=slack, with_stats=True)
    assert not bad
    err, on = pattern_errors(sigma, Ainv, rp, ci)
    _record(f"selinv_{name}_slack{slack}", dict(error=err, **st))
    assert err <= 1e-10, (name, slack, err, st)
    assert not sigma[~on].any()
    assert np.array_equal(sigma, sigma.T)
    assert np.array_equal(selected_inverse(A, slack=slack)[0], sigma)
    if name == "block_diagonal":
        assert st["tiles"] == st["tile_columns"], st
    if name in CLOSURES:
        assert st["levels"] > 1, st


# D A D with D constant per pose and log-spaced over 1 .. 1e3: the blocks of A span six decades, those of A^-1 as well (poses far from the
# gauge).  The reference is D^-1 inv(A) D^-1, exact in the scaling: numpy's own inverse of D A D is per block no better than the kernels
# (measured 1.1e-9 off it on trajectory_1000, where the kernels are 9.6e-10 off numpy's inverse -- recorded as "vs_numpy").  Measured
# against the scaled reference: 4.4e-15 (band_loop_closure), 2.9e-15 (two_closures), 1.0e-14 (trajectory_1000); bar with ~5x room.
BAR_SCALED = 5e-14


@pytest.mark.parametrize("name", CLOSURES)
def test_selected_inverse_scaled(name):
    rp, ci, A0, Ainv0 = _system(name)
    P = len(rp) - 1
    d = np.repeat(np.logspace(0, 3, P), 6)
    A = d[:, None] * A0 * d[None, :]
    sigma, bad = selected_inverse(A)
    assert not bad
    err, on = pattern_errors(sigma, Ainv0 / (d[:, None] * d[None, :]), rp, ci)
    _record(f"selinv_scaled_{name}", dict(error=err, vs_numpy=pattern_errors(sigma, np.linalg.inv(A), rp, ci)[0]))
    assert err <= BAR_SCALED, (name, err)
    assert not sigma[~on].any() and np.array_equal(sigma, sigma.T)


# Dense SPD matrices of condition 1e8 (as test_exact_reduced_solve_kernels_against_lapack builds them): one padded tile, whole tiles,
# 4 tiles + 1 pose, 22 poses' worth of tiles.  The pattern is full, so sigma is the whole inverse: |sigma - inv| <= 1e-6 |inv| (cond x eps
# with room; measured 4.2e-10 .. 1.9e-9).  |A sigma - I|: a symmetric inverse is not a left inverse to working precision (forward error
# x |A|); measured 1.1e-9 .. 5.2e-9 over the sizes, bar with ~5x room.
BAR_DENSE_RESIDUAL = 2.5e-8


@pytest.mark.parametrize("n", [6, 30, 126, 132, 384])
def test_selected_inverse_dense_conditioning(n):
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.logspace(0, 8, n)) @ Q.T
    A = 0.5 * (A + A.T)
    ref = np.linalg.inv(A)
    sigma, bad = selected_inverse(A)
    assert not bad
    err = np.abs(sigma - ref).max() / np.abs(ref).max()
    res = np.abs(A @ sigma - np.eye(n)).max()
    _record(f"selinv_dense_{n}", dict(error=err, residual=res))
    assert err <= 1e-6, (n, err)
    assert res <= BAR_DENSE_RESIDUAL, (n, res)
    assert np.array_equal(sigma, sigma.T)


def test_selected_inverse_reports_a_non_positive_pivot():
    """the indefinite matrix of test_exact_reduced_solve_reports_a_non_positive_pivot: reported (status 0), sigma left at zero; a positive
    definite matrix in the same process afterwards is inverted as before"""
    rng = np.random.default_rng(5)
    n = 192
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.linspace(1.0, 50.0, n); ev[100] = -3.0
    A = (Q * ev) @ Q.T
    A = 0.5 * (A + A.T)
    sigma, bad = selected_inverse(A)
    assert bad and not sigma.any()
    rp, ci, B, Binv = _system("two_closures")
    sigma, bad = selected_inverse(B)
    assert not bad and pattern_errors(sigma, Binv, rp, ci)[0] <= 1e-10


@pytest.mark.parametrize("pose_reorder", [1, 0])
def test_selected_inverse_matches_the_handle(pose_reorder):
    """The hook runs the product's calls: on the 40-pose graph, the handle's own reduced matrix at lambda = 0 (what covariance() leaves in
    hsc) through the hook agrees with the handle's pose blocks and covariance_blocks() to 1e-12 per block.  With pose_reorder = 0 the
    handle factorises the caller's pattern itself -- the same plan as the hook's, the same calls --, so the two agree bit for bit.  With
    the default reordering they agree bit for bit too on this graph (the trajectory's own pose order is the one the reordering keeps);
    a graph whose poses the handle renumbers would factorise a permuted pattern, under a plan (and summation order) of its own."""
    fp = small_fp()
    h = HipSolver(fp, RK_HUBER, pose_reorder=pose_reorder)
    h.optimize(10)
    cov = h.covariance()
    assert not cov["not_positive_definite"]
    blocks = h.covariance_blocks()
    rp, ci, v = h.hsc()
    S = _dense_from_upper(rp, ci, v, fp.Pf)
    sigma, bad = selected_inverse(S, slack=-1)
    assert not bad
    # the hook's pattern (blocks not identically zero) is the handle's
    nz = [(i, j) for i in range(fp.Pf) for j in range(i, fp.Pf) if S[6 * i:6 * i + 6, 6 * j:6 * j + 6].any() or i == j]
    assert nz == [(i, int(ci[k])) for i in range(fp.Pf) for k in range(rp[i], rp[i + 1])]
    ep = max(np.abs(cov["pose"][p] - sigma[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max() / np.abs(sigma[6 * p:6 * p + 6, 6 * p:6 * p + 6]).max()
             for p in range(fp.Pf))
    ec = max(np.abs(blocks[k] - sigma[6 * i:6 * i + 6, 6 * ci[k]:6 * ci[k] + 6]).max()
             / np.abs(sigma[6 * i:6 * i + 6, 6 * ci[k]:6 * ci[k] + 6]).max() for i in range(fp.Pf) for k in range(rp[i], rp[i + 1]))
    same = all(np.array_equal(cov["pose"][p], sigma[6 * p:6 * p + 6, 6 * p:6 * p + 6]) for p in range(fp.Pf)) and \
        all(np.array_equal(blocks[k], sigma[6 * i:6 * i + 6, 6 * ci[k]:6 * ci[k] + 6]) for i in range(fp.Pf) for k in range(rp[i], rp[i + 1]))
    _record(f"selinv_vs_handle_reorder{pose_reorder}", dict(pose=ep, cross=ec, bit_identical=same))
    assert max(ep, ec) <= 1e-12, (ep, ec)
    assert same


def test_selected_inverse_refused_in_fp32_library():
    rp, ci, A, _ = _system("one_tile")
    with pytest.raises(CubaHipError, match="status 1"):
        selected_inverse(A, precision="f32")

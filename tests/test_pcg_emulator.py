"""The fp64 PCG reference of tests/pcg_emulator.py, checked on the CPU: its coarse space (partition of unity, the lone-last-pose and
short-last-aggregate rules), its block-Jacobi limit, and convergence to scipy's direct solve on reduced systems the oracle builds from
synth.py graphs.  No GPU involved."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.dirname(__file__))
from pcg_emulator import TwoLevelPCG, agg_weights, prolongation, reduced_matrix, stop_iteration  # noqa: E402

from conftest import RK_HUBER  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba  # noqa: E402
from oracle.oracle import OracleSolver  # noqa: E402

_systems = {}


def oracle_system(P, L, E, seed, lam_rel=1e-4):
    """(rp, ci, v, bsc) of the oracle's reduced system at lambda = lam_rel * max diagonal (its diagonal blocks hold lambda already)"""
    key = (P, L, E, seed, lam_rel)
    if key not in _systems:
        fp = flatten(synth_ba(P, L, E, seed=seed))
        o = OracleSolver(fp, RK_HUBER)
        o.compute_errors(); o.build_system()
        o.set_lambda(lam_rel * o.max_diagonal()); o.schur()
        rp, ci, v = o.hsc()
        _systems[key] = (rp, ci, v, o.array("bsc"))
    return _systems[key]


def banded_system(Pf, seed=0, width=3):
    """random SPD block-banded upper BSR (a keyframe chain's co-visibility) and a right-hand side"""
    rng = np.random.default_rng(seed)
    rp, ci, v = [0], [], []
    for i in range(Pf):
        for j in range(i, min(Pf, i + width + 1)):
            ci.append(j)
            B = rng.normal(size=(6, 6)) * (0.3 if j > i else 1.0)
            v.append(B @ B.T + 6 * (width + 1) * np.eye(6) if j == i else B)
        rp.append(len(ci))
    return np.array(rp), np.array(ci), np.array(v), rng.normal(size=6 * Pf)


@pytest.mark.parametrize("Pf,agg", [(40, 8), (41, 8), (37, 6), (5, 6)])
def test_constant_functions_are_a_partition_of_unity(Pf, agg):
    for cl in (1, 2):
        P, nc = prolongation(Pf, agg, cl)
        assert nc == (Pf + agg - 1) // agg
        Pd = P.toarray()
        const = np.concatenate([np.arange(6) + 6 * cl * J for J in range(nc)])
        np.testing.assert_array_equal(Pd[:, const].reshape(Pf, 6, nc, 6).sum(axis=2), np.tile(np.eye(6), (Pf, 1, 1)))
        assert set(np.unique(Pd[:, const])) <= {0.0, 1.0}
    w = agg_weights(Pf, agg)
    assert np.all(np.abs(w) < 1)
    full = (Pf // agg) * agg
    if full:       # whole aggregates: the linear function is odd about the aggregate's centre
        assert np.allclose(w[:full].reshape(-1, agg).sum(axis=1), 0)


@pytest.mark.parametrize("Pf,agg", [(41, 8), (25, 6), (13, 2), (38, 8), (39, 6)])
def test_coarse_matrix_is_spd_at_the_edges(Pf, agg):
    """a lone last pose (Pf % agg == 1: weight 0 and an identity block) and a short last aggregate both give an SPD Ac"""
    rp, ci, v, _ = banded_system(Pf, seed=Pf)
    for cl in (1, 2):
        m = TwoLevelPCG(rp, ci, v, 0.0, agg, cl)
        assert np.linalg.eigvalsh(m.Ac).min() > 0
    if Pf % agg == 1:
        assert agg_weights(Pf, agg)[-1] == 0
        with pytest.raises(np.linalg.LinAlgError):       # without the identity block the coarse matrix is singular
            TwoLevelPCG(rp, ci, v, 0.0, agg, 2, patch=False)


def test_block_jacobi_limit():
    """agg = 0: M^-1 is the block-diagonal inverse, and the iterates are those of a plain block-Jacobi PCG"""
    rp, ci, v, b = banded_system(30, seed=3)
    m = TwoLevelPCG(rp, ci, v, 0.5, 0, 1)
    A = reduced_matrix(rp, ci, v, 0.5)[0].toarray()
    Dinv = np.zeros_like(A)
    for i in range(30):
        Dinv[6 * i:6 * i + 6, 6 * i:6 * i + 6] = np.linalg.inv(A[6 * i:6 * i + 6, 6 * i:6 * i + 6])
    r = np.random.default_rng(1).normal(size=180)
    np.testing.assert_allclose(m.minv(r), Dinv @ r, rtol=1e-12, atol=1e-12 * np.abs(Dinv @ r).max())
    x, rr = np.zeros(180), b.copy()
    z = Dinv @ rr; p = z.copy(); rz = rr @ z
    out = m.run(b, 6, keep=range(7))
    for k in range(6):
        q = A @ p; al = rz / (p @ q); x = x + al * p; rr = rr - al * q; z = Dinv @ rr
        rzn = rr @ z; p = z + rzn / rz * p; rz = rzn
        np.testing.assert_allclose(out["x"][k + 1], x, rtol=0, atol=1e-12 * np.abs(x).max())
        assert out["rz"][k + 1] == pytest.approx(rz, rel=1e-10)


def test_pose_order_is_a_symmetric_permutation():
    """with an internal order the preconditioner is P^T M P of the permuted problem: still SPD, and the solution unchanged"""
    rp, ci, v, b = banded_system(24, seed=5)
    order = np.random.default_rng(2).permutation(24)
    m = TwoLevelPCG(rp, ci, v, 0.1, 6, 2, order=order)
    Mi = np.stack([m.minv(e) for e in np.eye(144)], axis=1)
    assert np.abs(Mi - Mi.T).max() <= 1e-12 * np.abs(Mi).max() and np.linalg.eigvalsh(Mi).min() > 0
    x = spla.spsolve(m.A.tocsc(), b)
    assert np.abs(m.run(b, 144)["x_last"] - x).max() <= 1e-8 * np.abs(x).max()


@pytest.mark.parametrize("agg,cl,fp32", [(0, 1, False), (6, 1, False), (6, 2, False), (8, 2, True), (39, 2, False)])
def test_converges_to_the_direct_solve_on_oracle_systems(agg, cl, fp32):
    """reduced systems of synth.py graphs as the oracle builds them (40 poses: 39 free; agg 8 and 6 leave short
    last aggregates); the stop iteration is where r.z first falls below tol^2 r0.z0"""
    rp, ci, v, bsc = oracle_system(40, 600, 2400, seed=1)
    m = TwoLevelPCG(rp, ci, v, 0.0, agg, cl, coarse_fp32=fp32)
    x = spla.spsolve(m.A.tocsc(), bsc)
    out = m.run(bsc, 150)
    assert np.abs(out["x_last"] - x).max() <= 1e-9 * np.abs(x).max()
    k = stop_iteration(out["rz"], 1e-7)
    assert k is not None and 0 < k < 150
    assert out["rz"][k] <= 1e-14 * out["rz"][0] < out["rz"][k - 1]
    r = bsc - m.matvec(x)
    assert np.abs(r).max() <= 1e-9 * np.abs(bsc).max()


def test_lone_last_pose_on_an_oracle_system():
    """Pf = 39, agg = 2: the last aggregate is one pose with a zero linear weight"""
    rp, ci, v, bsc = oracle_system(40, 600, 2400, seed=1)
    assert len(rp) - 1 == 39
    m = TwoLevelPCG(rp, ci, v, 0.0, 2, 2)
    x = spla.spsolve(m.A.tocsc(), bsc)
    assert np.abs(m.run(bsc, 150)["x_last"] - x).max() <= 1e-9 * np.abs(x).max()

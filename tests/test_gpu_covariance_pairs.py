"""Covariance blocks of arbitrary vertex pairs (cuba_hip_compute_covariance_pairs / HipSolver.covariance_pairs, csrc/ba_covariance_pairs.hip):
the kernels alone on given matrices (capi.inverse_blocks) against numpy's inverse, the handle against a dense inverse of the oracle's
undamped Hessian, consistency with covariance() / covariance_blocks(), chunking, reproducibility, refusals, and the proof that a call
leaves the LM path bit for bit as it was.  Errors are |got - want|_max / sqrt(max|Sigma_aa| max|Sigma_bb|): the Cauchy-Schwarz scale keeps
tiny far-apart cross blocks meaningful."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from sparse_chol_emulator import random_spd_blocks  # noqa: E402
from test_gpu_covariance import RK_TUKEY_WIDE, _dense_from_upper, _record, _sequence, _assert_identical, dense_covariance, small_fp  # noqa: E402
from test_sparse_plan import CASES, band_pattern  # noqa: E402

from conftest import RK_HUBER, RK_NONE, with_fixed  # noqa: E402
from test_gpu_configs import shuffled_pose_ids  # noqa: E402
from cuba_amd.capi import CubaHipError, HipSolver, inverse_blocks  # noqa: E402
from cuba_amd.graph import flatten  # noqa: E402
from cuba_amd.synth import synth_ba, synth_named  # noqa: E402
from oracle.oracle import OracleSolver  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERNS = dict(CASES, trajectory_1000=lambda: band_pattern(1000, 18, closures=[(0, 770, 230)]))
CLOSURES = ("band_loop_closure", "two_closures", "trajectory_1000")


@functools.lru_cache(maxsize=None)
def _system(name):
    rp, ci = PATTERNS[name]()
    A = random_spd_blocks(rp, ci, np.random.default_rng(len(ci)))
    return rp, ci, A, np.linalg.inv(A)


def _block_pairs(rp, ci, rng, n=60):
    """random pairs (mostly off the pattern), pattern blocks in both orientations, a pose with itself, first against last and every pose"""
    P = len(rp) - 1
    pr = [(int(a), int(b)) for a, b in rng.integers(0, P, size=(n, 2))]
    ks = rng.choice(len(ci), size=min(len(ci), 20), replace=False)
    rows = np.repeat(np.arange(P), np.diff(rp))
    pr += [(int(rows[k]), int(ci[k])) for k in ks] + [(int(ci[k]), int(rows[k])) for k in ks]
    pr += [(0, 0), (P - 1, P - 1), (0, P - 1), (P - 1, 0)] + [(0, j) for j in range(0, P, max(1, P // 25))]
    return pr


def _scaled_error(blocks, pairs, Ainv, dim=6):
    err = 0.0
    for (a, b), got in zip(pairs, blocks):
        sa, sb = slice(dim * a, dim * a + dim), slice(dim * b, dim * b + dim)
        scale = np.sqrt(np.abs(Ainv[sa, sa]).max() * np.abs(Ainv[sb, sb]).max())
        err = max(err, np.abs(got - Ainv[sa, sb]).max() / scale)
    return err


@pytest.mark.parametrize("slack", [-1, 0, 4, 8])
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_kernels_on_sparse_patterns(name, slack):
    rp, ci, A, Ainv = _system(name)
    pairs = _block_pairs(rp, ci, np.random.default_rng(slack + 17))
    blocks, bad, st = inverse_blocks(A, pairs, slack=slack, with_stats=True)
    assert not bad
    err = _scaled_error(blocks, pairs, Ainv)
    _record(f"pairs_{name}_slack{slack}", dict(error=err, **st))
    assert err <= 1e-10, (name, slack, err, st)
    assert np.array_equal(inverse_blocks(A, pairs, slack=slack)[0], blocks)          # bit-reproducible


# D A D with D log-spaced over 1 .. 1e3 per pose, against D^-1 inv(A) D^-1 (exact in the scaling; see test_gpu_selinv.py)
@pytest.mark.parametrize("name", CLOSURES)
def test_kernels_scaled(name):
    rp, ci, A0, Ainv0 = _system(name)
    P = len(rp) - 1
    d = np.repeat(np.logspace(0, 3, P), 6)
    A = d[:, None] * A0 * d[None, :]
    pairs = _block_pairs(rp, ci, np.random.default_rng(3))
    blocks, bad = inverse_blocks(A, pairs)
    assert not bad
    err = _scaled_error(blocks, pairs, Ainv0 / (d[:, None] * d[None, :]))
    _record(f"pairs_scaled_{name}", dict(error=err))
    assert err <= 5e-14, (name, err)


@pytest.mark.parametrize("n", [6, 30, 126, 132, 384])
def test_kernels_dense_conditioning(n):
    rng = np.random.default_rng(n)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.logspace(0, 8, n)) @ Q.T
    A = 0.5 * (A + A.T)
    ref = np.linalg.inv(A)
    P = n // 6
    pairs = [(i, j) for i in range(P) for j in range(P)]
    blocks, bad = inverse_blocks(A, pairs)
    assert not bad
    got = np.zeros_like(ref)
    for (i, j), B in zip(pairs, blocks):
        got[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
    err = np.abs(got - ref).max() / np.abs(ref).max()
    _record(f"pairs_dense_{n}", dict(error=err))
    assert err <= 1e-6, (n, err)


def test_kernels_report_a_non_positive_pivot():
    rng = np.random.default_rng(5)
    n = 192
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.linspace(1.0, 50.0, n); ev[100] = -3.0
    A = (Q * ev) @ Q.T
    blocks, bad = inverse_blocks(0.5 * (A + A.T), [(0, 31), (5, 5)])
    assert bad and not blocks.any()


# ---- the handle ------------------------------------------------------------------------------------------------------------------------

def _slice(fp, kind, i):
    if kind == "pose":
        return slice(6 * i, 6 * i + 6) if i < fp.Pf else None
    return slice(6 * fp.Pf + 3 * i, 6 * fp.Pf + 3 * i + 3) if i < fp.Lf else None


def handle_pairs(fp, rng, n=25):
    """all four kinds (fixed vertices included), every vertex kind with itself, both orientations of each pair, repeated pairs"""
    def pick(kind):
        return int(rng.integers(0, fp.Pt if kind == "pose" else fp.Lt))
    out = []
    for ka in ("pose", "landmark"):
        for kb in ("pose", "landmark"):
            if (ka == "pose" and fp.Pt == 0) or (kb == "pose" and fp.Pt == 0) or (ka == "landmark" and fp.Lt == 0) or (kb == "landmark" and fp.Lt == 0):
                continue
            out += [(ka, pick(ka), kb, pick(kb)) for _ in range(n)]
    if fp.Pt:
        out += [("pose", 0, "pose", 0), ("pose", 0, "pose", fp.Pt - 1)]
    if fp.Lt:
        out += [("landmark", 0, "landmark", 0), ("landmark", fp.Lt - 1, "landmark", fp.Lt - 1)]
    out += [(kb, b, ka, a) for ka, a, kb, b in out]
    return out + out[:10]


def pair_errors(blocks, pairs, Hi, fp):
    err = 0.0
    for (ka, a, kb, b), got in zip(pairs, blocks):
        assert got.shape == (6 if ka == "pose" else 3, 6 if kb == "pose" else 3)
        sa, sb = _slice(fp, ka, a), _slice(fp, kb, b)
        if sa is None or sb is None:
            assert not got.any(), (ka, a, kb, b)
            continue
        scale = np.sqrt(np.abs(Hi[sa, sa]).max() * np.abs(Hi[sb, sb]).max())
        err = max(err, np.abs(got - Hi[sa, sb]).max() / scale)
    return err


def consistency_errors(h, blocks, pairs, fp, cov, Hi):
    """(diagonal pairs against covariance(), co-visible pose pairs against covariance_blocks(), Sigma_ab against Sigma_ba^T), with the
    Cauchy-Schwarz scale of the dense inverse Hi"""
    got = dict(zip(pairs, blocks))
    ed = {"pose": 0.0, "landmark": 0.0}
    es = 0.0
    for (ka, a, kb, b), B in got.items():
        sa, sb = _slice(fp, ka, a), _slice(fp, kb, b)
        if sa is None or sb is None:
            continue
        scale = np.sqrt(np.abs(Hi[sa, sa]).max() * np.abs(Hi[sb, sb]).max())
        if ka == kb and a == b:
            want = cov["pose"][a] if ka == "pose" else cov["landmark"][a]
            ed[ka] = max(ed[ka], np.abs(B - want).max() / scale)
        es = max(es, np.abs(B - got[(kb, b, ka, a)].T).max() / scale)
    ec = 0.0
    if fp.Pf:
        rp, ci = h.hsc_structure()
        cb = h.covariance_blocks()
        sel = np.random.default_rng(0).choice(len(ci), size=min(len(ci), 60), replace=False)
        rows = np.repeat(np.arange(fp.Pf), np.diff(rp))
        cpairs = [("pose", int(rows[k]), "pose", int(ci[k])) for k in sel]
        cbl, bad = h.covariance_pairs(cpairs)
        assert not bad
        for k, B in zip(sel, cbl):
            ec = max(ec, np.abs(B - cb[k]).max() / np.abs(cb[k]).max())
    return ed, ec, es


BAR = 1e-9
# The pairs and covariance() / covariance_blocks() share the factor but not the algorithm (triangular solves against the Takahashi
# recurrence).  Pose blocks -- co-visible pairs against covariance_blocks() (measured 2.6e-15) and diagonal pose pairs against covariance()
# -- keep the 1e-12 bar.  The landmark diagonals and Sigma_ab against Sigma_ba^T go through Hll^-1 and W on two different paths (the
# landmark pass of covariance() sums Sigma_pq W_q over pose pairs, the pairs sum W^T X over edges): measured up to 2.3e-11 and 2.7e-11 on
# the 40-pose graph, where each path is ~5e-11 off the dense inverse; bar with ~4x room.
BAR_CONSISTENT = 1e-12
BAR_CONSISTENT_LANDMARKS = 1e-10


def _check_handle(fp, rk, label, bar=BAR, **opts):
    h = HipSolver(fp, rk, **opts)
    h.optimize(10)
    pairs = handle_pairs(fp, np.random.default_rng(fp.E))
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    Hi = dense_covariance(h, fp, rk)
    err = pair_errors(blocks, pairs, Hi, fp)
    cov = h.covariance(landmarks=True)
    ed, ec, es = consistency_errors(h, blocks, pairs, fp, cov, Hi)
    # one vertex against all the others: solved with the single vertex on the right and transposed back
    one = [pairs[0][:2] + p[2:] for p in pairs]
    b_one, bad = h.covariance_pairs(one)
    assert not bad
    e_one = pair_errors(b_one, one, Hi, fp)
    _record("pairs_" + label, dict(error=err, one_vs_many=e_one, vs_covariance_pose=ed["pose"], vs_covariance_landmark=ed["landmark"],
                                   vs_covariance_blocks=ec, symmetry=es))
    assert max(err, e_one) <= bar, (label, err, e_one)
    assert max(ed["pose"], ec) <= BAR_CONSISTENT, (label, ed, ec)
    assert max(ed["landmark"], es) <= BAR_CONSISTENT_LANDMARKS, (label, ed, es)
    again, _ = h.covariance_pairs(pairs)
    assert all(np.array_equal(a, b) for a, b in zip(again, blocks))
    return h, pairs, blocks


@pytest.mark.parametrize("rk,label", [(RK_HUBER, "huber"), (RK_NONE, "none"), (RK_TUKEY_WIDE, "tukey_outlier")])
def test_handle_against_dense_inverse(rk, label):
    _check_handle(small_fp(with_outlier=rk is not RK_HUBER), rk, label)


def test_handle_fixed_vertices_shuffled_ids_landmark_order_mixed_precision():
    g = synth_ba(40, 600, 2400, seed=1)
    _check_handle(flatten(with_fixed(g, fixed_pose_rows=[3, 4, 20], fixed_lm_rows=list(range(0, 300, 7)))), RK_HUBER, "fixed")
    _check_handle(flatten(shuffled_pose_ids(g, seed=3)), RK_HUBER, "shuffled")
    for lo in (0, 1):
        _check_handle(small_fp(), RK_HUBER, f"landmark_reorder_{lo}", landmark_reorder=lo)
    _check_handle(small_fp(), RK_HUBER, "mixed_precision", mixed_precision=1)


@pytest.mark.parametrize("pf", [1, 4, 5, 6])
def test_few_free_poses(pf):
    g = synth_ba(12, 300, 1200, seed=4)
    fp = flatten(with_fixed(g, fixed_pose_rows=range(1 + pf, 12)))
    assert fp.Pf == pf
    _check_handle(fp, RK_HUBER, f"free_poses_{pf}")


def test_every_pose_fixed():
    """landmark-landmark = delta Hll^-1 (the landmark pass's, bit for bit), every cross block zero"""
    g = synth_ba(40, 600, 2400, seed=1)
    fp = flatten(with_fixed(g, fixed_pose_rows=range(g.nposes)))
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    pairs = handle_pairs(fp, np.random.default_rng(2))
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    lm_sys = h.array("lm_sys").reshape(fp.Lf, 9)
    idx = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    for (ka, a, kb, b), B in zip(pairs, blocks):
        if ka == kb == "landmark" and a == b and a < fp.Lf:
            assert np.array_equal(B, lm_sys[a][idx])
        else:
            assert not B.any(), (ka, a, kb, b)


def test_every_landmark_fixed():
    g = synth_ba(40, 600, 2400, seed=1)
    _check_handle(flatten(with_fixed(g, fixed_lm_rows=range(g.nlandmarks))), RK_HUBER, "every_landmark_fixed")


def test_landmarks_seen_only_by_fixed_poses():
    g = synth_ba(40, 600, 2400, seed=1)
    fp = flatten(with_fixed(g, fixed_pose_rows=range(12, 26)))
    h, pairs, blocks = _check_handle(fp, RK_HUBER, "landmarks_seen_only_by_fixed_poses")
    free_obs = np.bincount(fp.eL[fp.eP < fp.Pf], minlength=fp.Lt)[:fp.Lf]
    lonely = [int(l) for l in np.flatnonzero(free_obs == 0)[:5]]
    assert lonely
    q = [("landmark", l, "landmark", l) for l in lonely] + [("pose", 0, "landmark", l) for l in lonely]
    bl, _ = h.covariance_pairs(q)
    lm_sys = h.array("lm_sys").reshape(fp.Lf, 9)
    idx = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
    for (ka, a, kb, b), B in zip(q, bl):
        if ka == "landmark":
            assert np.array_equal(B, lm_sys[a][idx])
        else:
            assert not B.any()


def test_landmarks_with_more_than_64_observations():
    from test_gpu_parity import graph_with_big_landmarks
    g, n_big = graph_with_big_landmarks()
    fp = flatten(g)
    counts = np.bincount(fp.eL[fp.eP < fp.Pf], minlength=fp.Lt)[:fp.Lf]
    big = [int(l) for l in np.flatnonzero(counts > 64)]
    assert len(big) >= n_big
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    pairs = [("landmark", a, "landmark", b) for a in big for b in big] + [("pose", p, "landmark", l) for p in (0, fp.Pf - 1) for l in big]
    pairs += [(kb, b, ka, a) for ka, a, kb, b in pairs]
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    err = pair_errors(blocks, pairs, dense_covariance(h, fp, RK_HUBER), fp)
    _record("pairs_big_landmarks", dict(error=err, max_observations=int(counts.max())))
    assert err <= BAR, err


def test_chunks_agree_with_one_chunk():
    """a workspace cap of 0.07 MiB (8 tiles: the 40-pose graph's whole tree) forces one chunk per few blocks; a cap below one block's
    tiles is refused with the handle left usable"""
    fp = small_fp()
    pairs = handle_pairs(fp, np.random.default_rng(9), n=40)
    res = {}
    for mb in (0, 0.07):
        h = HipSolver(fp, RK_HUBER, covariance_workspace_mb=mb)
        h.optimize(10)
        res[mb], bad = h.covariance_pairs(pairs)
        assert not bad
        res[(mb, "chunks")] = h.counter("covariance_pairs_chunks")
        if mb:
            h.set_option("covariance_workspace_mb", 0.01)
            with pytest.raises(CubaHipError, match="status 2"):
                h.covariance_pairs(pairs)
            h.set_option("covariance_workspace_mb", mb)
            assert all(np.array_equal(a, b) for a, b in zip(h.covariance_pairs(pairs)[0], res[mb]))
    assert res[(0, "chunks")] == 1 and res[(0.07, "chunks")] >= 3, res
    err = max(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300) for a, b in zip(res[0], res[0.07]) if a.any())
    _record("pairs_chunks", dict(error=err, chunks=res[(0.07, "chunks")]))
    assert err <= 1e-13, err


def test_kitti00_size():
    fp = flatten(synth_named("kitti00"))
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    rng = np.random.default_rng(7)
    first = [("pose", 0, "pose", j) for j in range(fp.Pf)]
    rnd = []
    for ka in ("pose", "landmark"):
        for kb in ("pose", "landmark"):
            rnd += [(ka, int(rng.integers(0, fp.Pf if ka == "pose" else fp.Lf)), kb, int(rng.integers(0, fp.Pf if kb == "pose" else fp.Lf)))
                    for _ in range(200)]
    b_first, bad = h.covariance_pairs(first)
    assert not bad
    t_first = h.counter("covariance_pairs_ns")
    b_rnd, bad = h.covariance_pairs(rnd)
    assert not bad
    hrp, hci, hv = h.hsc()
    Si = np.linalg.inv(_dense_from_upper(hrp, hci, hv, fp.Pf))
    o = OracleSolver(fp, RK_HUBER)
    o.set_state(*h.state())
    o.compute_errors(); o.build_system()
    Hll = o.array("Hll").reshape(fp.Lf, 3, 3).transpose(0, 2, 1)
    Hpl = o.array("Hpl").reshape(fp.E, 3, 6).transpose(0, 2, 1)
    order = np.argsort(fp.eL, kind="stable")
    starts = np.searchsorted(fp.eL[order], np.arange(fp.Lf + 1))

    @functools.lru_cache(maxsize=None)
    def K(l):                       # (Hpl column block of landmark l as a 6 Pf x 3 matrix, Hll_l^-1, Si times that block)
        M = np.zeros((6 * fp.Pf, 3))
        for e in order[starts[l]:starts[l + 1]]:
            if fp.eP[e] < fp.Pf:
                M[6 * fp.eP[e]:6 * fp.eP[e] + 6] += Hpl[e]
        return M, np.linalg.inv(Hll[l]), Si @ M

    def want(ka, a, kb, b):
        if ka == "pose" and kb == "pose":
            return Si[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        if ka == "pose":
            _, Hm, SM = K(b)
            return -SM[6 * a:6 * a + 6] @ Hm
        if kb == "pose":
            _, Hl, SM = K(a)
            return -Hl @ SM[6 * b:6 * b + 6].T
        Ml, Hl, _ = K(a); _, Hm, SMm = K(b)
        return (Hl if a == b else 0) + Hl @ (Ml.T @ SMm) @ Hm

    def err(pairs, blocks):
        e = 0.0
        for (ka, a, kb, b), B in zip(pairs, blocks):
            scale = np.sqrt(np.abs(want(ka, a, ka, a)).max() * np.abs(want(kb, b, kb, b)).max())
            e = max(e, np.abs(B - want(ka, a, kb, b)).max() / scale)
        return e
    e1, e2 = err(first, b_first), err(rnd, b_rnd)
    _record("pairs_kitti00", dict(first_vs_all=e1, random=e2, first_vs_all_ns=t_first))
    assert max(e1, e2) <= 1e-8, (e1, e2)


@pytest.mark.parametrize("opts", [dict(), dict(reduced_solver=1)])
def test_later_optimize_is_unaffected(opts):
    fp = flatten(synth_named("kitti07"))
    pairs = [("pose", 0, "pose", 50), ("landmark", 3, "pose", 7), ("landmark", 10, "landmark", 900), ("pose", 2, "landmark", 5)]
    a = _sequence(fp, lambda h: h.covariance_pairs(pairs), **opts)
    b = _sequence(fp, lambda h: None, **opts)
    _assert_identical(a, b)


def test_refusals_leave_the_handle_usable():
    fp = small_fp()
    pairs = [("pose", 0, "pose", 30), ("landmark", 1, "pose", 2)]
    h32 = HipSolver(fp, RK_HUBER, precision="f32")
    with pytest.raises(CubaHipError, match="status 1"):
        h32.covariance_pairs(pairs)
    assert len(h32.optimize(3)["chi2"]) == 3
    h0 = HipSolver(None, RK_HUBER)
    z = np.zeros(1, dtype=np.int32)
    out = np.zeros(36)
    bad = C.c_int()
    ip = C.POINTER(C.c_int32)
    assert h0.lib.cuba_hip_compute_covariance_pairs(h0.h, 1, *(z.ctypes.data_as(ip) for _ in range(4)), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                    C.byref(bad)) == 3
    hp = HipSolver(None, RK_HUBER)
    hp.set_graph(fp, landmark_range=(0, fp.Lt // 2))
    with pytest.raises(CubaHipError, match="status 3"):
        hp.covariance_pairs(pairs)
    h = HipSolver(fp, RK_HUBER)
    h.optimize(5)
    good, _ = h.covariance_pairs(pairs)
    for badp in ([("pose", fp.Pt, "pose", 0)], [("landmark", 0, "landmark", fp.Lt)], [("pose", -1, "pose", 0)], [("vertex", 0, "pose", 0)],
                 [(2, 0, "pose", 0)]):
        with pytest.raises(CubaHipError, match="status 1"):
            h.covariance_pairs(pairs + badp)
    assert all(np.array_equal(a, b) for a, b in zip(h.covariance_pairs(pairs)[0], good))
    # a factor beyond direct_max_tiles: refused with status 2
    hh = HipSolver(fp, RK_HUBER, direct_max_tiles=1)
    with pytest.raises(CubaHipError, match="status 2"):
        hh.covariance_pairs(pairs)
    assert len(hh.optimize(3)["chi2"]) == 3


def test_non_positive_definite_leaves_out_untouched():
    """RK_TUKEY zeroes every edge of some landmarks after the run: reported, the caller's buffer untouched"""
    from conftest import RK_TUKEY
    fp = small_fp()
    h = HipSolver(fp, RK_TUKEY)
    h.optimize(10)
    ka = np.zeros(2, dtype=np.int32); ia = np.array([0, 3], dtype=np.int32); ib = np.array([3, 0], dtype=np.int32)
    out = np.full(72, 7.0)
    bad = C.c_int()
    ip = C.POINTER(C.c_int32)
    rc = h.lib.cuba_hip_compute_covariance_pairs(h.h, 2, ka.ctypes.data_as(ip), ia.ctypes.data_as(ip), ka.ctypes.data_as(ip), ib.ctypes.data_as(ip),
                                                 out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(bad))
    assert rc == 0 and bad.value == 1 and np.all(out == 7.0)


def test_cpp_drift_sample_matches_python(tmp_path):
    """host/samples/drift_uncertainty (cuba::computeCrossCovariances) against the same first-order drift model computed from
    HipSolver.covariance_pairs on the same graph: Cov(c_k - c_0) = A_k S_kk A_k^T + A_0 S_00 A_0^T - A_k S_k0 A_0^T - A_0 S_0k A_k^T"""
    import re
    import subprocess
    from conftest import ROOT
    from oracle.oracle import quat_to_rot
    g = with_fixed(synth_ba(60, 1500, 6000, seed=3), fixed_pose_rows=[0, 1])
    path = str(tmp_path / "graph.json")
    g.to_json(path)
    exe = os.path.join(ROOT, "cuda-bundle-adjustment_amd", "host", "samples", "drift_uncertainty")
    out = subprocess.run([exe, path, "10", "1", "3"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {int(m[0]): np.array([float(m[1]), float(m[2]), float(m[3])]) for m in re.findall(r"pose (\d+) drift (\S+) (\S+) (\S+)", out.stdout)}
    fp = flatten(g)
    h = HipSolver(fp, RK_HUBER)
    h.optimize(10)
    q = h.state()[0]
    ids = np.array([int(g.pose_ids[fp.pose_src[p]]) for p in range(fp.Pf)])
    free = [int(p) for p in np.argsort(ids)]
    report = free[::3]
    p0 = free[0]
    pairs = []
    for k in report:
        pairs += [("pose", k, "pose", k), ("pose", k, "pose", p0)]
    blocks, bad = h.covariance_pairs(pairs)
    assert not bad
    assert sorted(got) == sorted(int(ids[k]) for k in report)
    A0 = quat_to_rot(q[p0]).T
    S00 = blocks[0][3:, 3:]
    for r, k in enumerate(report):
        if k == p0:                 # (c_0 - c_0: zero up to rounding, checked below)
            continue
        Ak = quat_to_rot(q[k]).T
        Skk, Sk0 = blocks[2 * r][3:, 3:], blocks[2 * r + 1][3:, 3:]
        C = Ak @ Skk @ Ak.T + A0 @ S00 @ A0.T - Ak @ Sk0 @ A0.T - A0 @ Sk0.T @ Ak.T
        want = np.sqrt(np.maximum(np.diag(C), 0.0))
        assert np.allclose(got[int(ids[k])], want, rtol=1e-6, atol=1e-12 * want.max()), (k, got[int(ids[k])], want)
    assert not got[int(ids[p0])].any() or got[int(ids[p0])].max() <= 1e-6 * max(v.max() for v in got.values())

"""numpy restatement of the selected inversion behind HipSolver.covariance (csrc/ba_covariance.hip: selinv_diag_inverse_kernel,
selinv_u_kernel, selinv_off_level_kernel, selinv_diag_level_kernel), driven by the arrays of its symbolic phase (capi.selinv_plan) on top
of the exact solver's plan (capi.sparse_plan).  Test infrastructure: the CPU suite checks the plan -- gather lists, transposed bits,
level schedule -- by inverting a matrix through it and comparing with LAPACK.  Every step asserts the dependency the schedule promises
(a gathered Sigma tile was written by an earlier step)."""
import numpy as np

TP, TS = 5, 32


def permuted_dense(plan, P, A):
    """A (6P x 6P) in the factor's unknown order: 32 unknowns per tile column, identity on the padded ones"""
    T = plan["T"]
    idx = np.zeros(6 * P, dtype=int)
    for p in range(P):
        idx[6 * p:6 * p + 6] = TS * plan["posOfSeg"][p // TP] + 6 * (p % TP) + np.arange(6)
    Ap = np.eye(TS * T)
    Ap[np.ix_(idx, idx)] = A
    return Ap, idx


def factor_tiles(plan, Ap):
    """L of Ap cut into the factor's tiles (the numeric factorisation itself is sparse_chol_emulator's subject); asserts that L vanishes
    outside the pattern"""
    nT, colPtr, rowIdx = plan["nTiles"], plan["colPtr"], plan["rowIdx"]
    L = np.linalg.cholesky(Ap)
    tiles = np.zeros((nT, TS, TS))
    seen = np.zeros((plan["T"], plan["T"]), dtype=bool)
    for j in range(plan["T"]):
        for t in range(colPtr[j], colPtr[j + 1]):
            i = rowIdx[t]
            tiles[t] = L[TS * i:TS * i + TS, TS * j:TS * j + TS]
            seen[i, j] = True
    for i in range(plan["T"]):
        for j in range(i):
            if not seen[i, j]:
                assert np.abs(L[TS * i:TS * i + TS, TS * j:TS * j + TS]).max() <= 1e-12 * np.abs(L).max(), "fill outside the factor's pattern"
    return tiles


def selected_inverse(plan, sel, Ltiles):
    """Sigma on the factor's pattern, [tile][row][col], by the recurrence of the device phase in the plan's order"""
    nT, colPtr = plan["nTiles"], plan["colPtr"]
    T = plan["T"]
    colOf = np.zeros(nT, dtype=int)
    for k in range(T):
        colOf[colPtr[k]:colPtr[k + 1]] = k
    # phase 1 (no dependencies): L_jj^-1, U_kj = L_kj L_jj^-1
    Linv = {j: np.linalg.inv(Ltiles[colPtr[j]]) for j in range(T)}
    U = np.zeros_like(Ltiles)
    for t in range(nT):
        if t != colPtr[colOf[t]]:
            U[t] = Ltiles[t] @ Linv[colOf[t]]
    sigma = np.zeros_like(Ltiles)
    written = np.zeros(nT, dtype=bool)
    rec = sel["offRec"].reshape(-1, 4)
    G = sel["gather"].reshape(-1, 2)
    for s in range(sel["nLevels"]):
        # off-diagonal tiles of the step: Sigma_ij = -sum_k Sigma_ik U_kj
        new = {}
        for t, j, g0, n in rec[sel["stepPtr"][s]:sel["stepPtr"][s + 1]]:
            acc = np.zeros((TS, TS))
            ks = []
            for ts, tu in G[g0:g0 + n]:
                st, tr = ts & 0x3fffffff, ts >> 30
                assert written[st], "a gathered Sigma tile was not written at an earlier step"
                assert colOf[tu] == j and tu != colPtr[j]
                ks.append(plan["rowIdx"][tu])
                acc -= (sigma[st].T if tr else sigma[st]) @ U[tu]
            assert ks == sorted(ks) and len(ks) == colPtr[j + 1] - colPtr[j] - 1, "gather list is not column j's rows in ascending order"
            new[t] = acc
        for t, v in new.items():
            sigma[t] = v; written[t] = True
        # diagonal tiles: Sigma_jj = L_jj^-T L_jj^-1 - sum_k U_kj^T Sigma_kj (lower triangle, mirrored)
        new = {}
        for j in sel["cols"][sel["colStepPtr"][s]:sel["colStepPtr"][s + 1]]:
            acc = Linv[j].T @ Linv[j]
            for t in range(colPtr[j] + 1, colPtr[j + 1]):
                assert written[t], "the diagonal tile reads an off-diagonal Sigma tile of a later step"
                acc -= U[t].T @ sigma[t]
            new[colPtr[j]] = np.tril(acc) + np.tril(acc, -1).T
        for t, v in new.items():
            sigma[t] = v; written[t] = True
    assert written.all()
    return sigma

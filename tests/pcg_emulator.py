"""Plain fp64 restatement of the reduced solve's PCG (csrc/ba_pcg.hip, csrc/ba_coarse.hip): textbook preconditioned
conjugate gradients from x0 = 0 on A = S + lambda I, with the two-level preconditioner

    M^-1 r = blockdiag(A)^-1 r + P Ac^-1 P^T r,   Ac = P^T A P,

P holding, per aggregate of `agg` consecutive INTERNAL pose indices and per pose component, a constant function and (cl = 2) the linear one
with weight (2 (i % agg) + 1 - agg) / agg -- 0 for a lone last pose when Pf % agg == 1, whose linear-linear block of Ac is then the
identity (coarse_assemble_kernel).  agg = 0 is block-Jacobi alone.  Ac^-1 comes from LAPACK, optionally rounded to fp32 (option
"precond_fp32").  Test infrastructure: the GPU suite compares the device's iterates with this one's, the CPU suite checks it against
scipy's direct solve."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp


def reduced_matrix(rp, ci, v, lam=0.0):
    """Full symmetric scipy CSR matrix of an upper-triangular BSR (rowptr, colind, values[nblk][row][col]) as HipSolver.hsc() returns it,
    plus lam on the diagonal.  Only the upper triangles of the diagonal blocks are read."""
    rp, ci = np.asarray(rp), np.asarray(ci)
    P = len(rp) - 1
    row = np.repeat(np.arange(P), np.diff(rp))
    v = np.array(v, dtype=np.float64)
    diag = row == ci
    iu = np.triu_indices(6, 1)
    d = v[diag]
    d[:, iu[1], iu[0]] = d[:, iu[0], iu[1]]
    d += lam * np.eye(6)
    v[diag] = d
    upper = sp.bsr_matrix((v, ci, rp), shape=(6 * P, 6 * P)).tocsr()
    off = sp.bsr_matrix((np.where(diag[:, None, None], 0.0, v), ci, rp), shape=(6 * P, 6 * P)).tocsr()
    return (upper + off.T).tocsr(), d


def agg_weights(Pf, agg):
    """weight of every pose (internal index) in the linear coarse function of its aggregate (agg_weight in csrc/ba_device.hpp)"""
    i = np.arange(Pf)
    w = (2.0 * (i % agg) + 1.0 - agg) / agg
    if Pf % agg == 1:
        w[Pf - 1] = 0.0
    return w


def prolongation(Pf, agg, cl):
    """P (6 Pf x 6 cl nc) in the internal pose order: coarse unknown (J, a, c) has index 6 cl J + 6 a + c"""
    nc = (Pf + agg - 1) // agg
    i = np.repeat(np.arange(Pf), 6)
    c = np.tile(np.arange(6), Pf)
    J = i // agg
    rows, cols, vals = [6 * i + c], [6 * cl * J + c], [np.ones(6 * Pf)]
    if cl == 2:
        rows.append(6 * i + c); cols.append(6 * cl * J + 6 + c); vals.append(np.repeat(agg_weights(Pf, agg), 6))
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * Pf, 6 * cl * nc)), nc


class TwoLevelPCG:
    """A = S + lam I from the caller-ordered upper BSR; `order[i]` = the caller's index of internal pose i (HipSolver.pcg_config()'s
    pose_order; identity when None).  Vectors in and out are in the caller's order."""

    def __init__(self, rp, ci, v, lam, agg, cl, order=None, coarse_fp32=False, patch=True):
        A, d = reduced_matrix(rp, ci, v, lam)
        Pf = len(rp) - 1
        self.Pf, self.agg, self.cl = Pf, agg, cl
        order = np.arange(Pf) if order is None else np.asarray(order)
        assert sorted(order.tolist()) == list(range(Pf))
        self.idx = (6 * order[:, None] + np.arange(6)).ravel()          # internal unknown -> caller unknown
        self.A = A                                                       # caller order
        self.Ai = A[self.idx][:, self.idx].tocsr()                       # internal order
        self.Dinv = np.linalg.inv(d)[order]                              # 6 x 6 block-Jacobi inverses, internal order
        self.P = None
        if agg > 0:
            self.P, self.nc = prolongation(Pf, agg, cl)
            Ac = (self.P.T @ (self.Ai @ self.P)).toarray()
            if patch and cl == 2 and Pf % agg == 1:
                k = 6 * cl * (self.nc - 1) + 6
                Ac[k:k + 6, k:k + 6] = np.eye(6)
            self.Ac = 0.5 * (Ac + Ac.T)
            inv = scipy.linalg.cho_solve(scipy.linalg.cho_factor(self.Ac), np.eye(len(Ac)))
            inv = 0.5 * (inv + inv.T)
            self.Acinv = inv.astype(np.float32).astype(np.float64) if coarse_fp32 else inv

    def _minv(self, r):
        z = np.einsum("irc,ic->ir", self.Dinv, r.reshape(-1, 6)).ravel()
        if self.P is not None:
            z += self.P @ (self.Acinv @ (self.P.T @ r))
        return z

    def minv(self, r):
        """M^-1 r, caller order"""
        r = np.asarray(r, dtype=np.float64)
        out = np.empty_like(r)
        out[self.idx] = self._minv(r[self.idx])
        return out

    def matvec(self, x):
        return self.A @ np.asarray(x, dtype=np.float64)

    def run(self, b, kmax, keep=()):
        """kmax iterations of textbook PCG from x0 = 0, whatever the residual (it ends early only where p.Ap is no longer positive: exact
        convergence).  Returns dict(x={k: x_k for k in keep}, rz=[r_k.z_k for k = 0..], x_last), vectors in the caller's order."""
        b = np.asarray(b, dtype=np.float64)[self.idx]
        x = np.zeros_like(b)
        r = b.copy()
        z = self._minv(r)
        p = z.copy()
        rz = [float(r @ z)]
        xs = {}
        if 0 in keep:
            xs[0] = self._caller(x)
        for k in range(kmax):
            q = self.Ai @ p
            pq = float(p @ q)
            if not pq > 0:       # converged to rounding (p = 0): the iterate stays
                break
            alpha = rz[-1] / pq
            x += alpha * p
            r -= alpha * q
            z = self._minv(r)
            rz.append(float(r @ z))
            p = z + (rz[-1] / rz[-2]) * p
            if k + 1 in keep:
                xs[k + 1] = self._caller(x)
        for k in keep:
            xs.setdefault(k, self._caller(x))
        return dict(x=xs, rz=np.array(rz), x_last=self._caller(x))

    def _caller(self, xi):
        out = np.empty_like(xi)
        out[self.idx] = xi
        return out


def stop_iteration(rz, tol):
    """the first k with r_k.z_k <= tol^2 r_0.z_0 (the device's stop test: iterations done), or None within len(rz)"""
    hit = np.nonzero(np.asarray(rz) <= tol * tol * rz[0])[0]
    return int(hit[0]) if len(hit) else None

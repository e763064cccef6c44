"""The CPR preconditioner as dense algebra in numpy - a yardstick for oracle/cpr.hpp and csrc/cpr.hip that shares no code, no data
layout and no summation order with either.  What it states (the header of cpr.hip):

    M^-1 d = E_p V W^T d + ILU0^-1 (d - A E_p V W^T d)

W^T: the weighted sum over a block's three components; E_p: injection into the pressure slot; ILU0: the block ILU0 (relaxation 1) of A
in the stored order; V: one V(1,1) cycle from x = 0 on A_p[i,j] = sum_r A_ij[r][p] w_i[r] with Galerkin operators P^T A_l P (P the 0/1
aggregate matrix), smoother S = (2/3) D^-1, prolongation damped by 1.6, the coarsest level solved exactly:

    x = S b;  x += 1.6 P V_c P^T (b - A x);  x += S (b - A x)

With ilu0_level0 the smoother of level 0 is a scalar ILU0 (relaxation 1) of A_p in the stored order, S = U^-1 L^-1, unless level 0 is
the only level (then the direct solve takes it); the levels below stay Jacobi.  Everything is evaluated in ONE working dtype
(np.float64 or np.longdouble), operators are applied to vectors (several at once, as columns), no inverse is formed.  Sizes: meant for
a few hundred cells (dense (3 Nb)^2 arrays)."""
import numpy as np

PRESSURE = 1          # pressureVarIndex of the black-oil indices
OMEGA_NUM, OMEGA_DEN = 2.0, 3.0
DAMP = 1.6


def solve_dense(A, b, dtype=np.longdouble):
    """Gaussian elimination with partial pivoting in `dtype`; b: a vector or a matrix of columns"""
    A, x = np.array(A, dtype=dtype), np.array(b, dtype=dtype)
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], x[[k, p]] = A[[p, k]], x[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:])
        x[k + 1:] -= np.multiply.outer(f, x[k])
    for k in range(n - 1, -1, -1):
        x[k] = (x[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


class DenseCpr:
    """Nb, rowptr, col, val: the block matrix in the order the preconditioner sees it; w: weights (Nb, 3); aggs: per level that has a
    coarser one, the aggregate of every node"""

    def __init__(self, Nb, rowptr, col, val, w, aggs, dtype=np.longdouble, ilu0_level0=False):
        self.Nb, self.dtype = Nb, dtype
        rowptr, col = np.asarray(rowptr), np.asarray(col)
        blk = np.asarray(val, np.float64).reshape(-1, 3, 3).astype(dtype)
        row = np.repeat(np.arange(Nb), np.diff(rowptr))
        A4 = np.zeros((Nb, 3, Nb, 3), dtype)
        A4[row, :, col, :] = blk
        self.A = A4.reshape(3 * Nb, 3 * Nb)
        self.w = np.asarray(w, np.float64).reshape(Nb, 3).astype(dtype)
        self.mask = np.zeros((Nb, Nb), bool)                 # the block pattern: what both ILU0s keep
        self.mask[row, col] = True
        Ap = A4[:, 0, :, PRESSURE] * self.w[:, 0:1] + A4[:, 1, :, PRESSURE] * self.w[:, 1:2] + A4[:, 2, :, PRESSURE] * self.w[:, 2:3]
        self.levels = [Ap]
        self.P = []
        for agg in aggs:
            agg = np.asarray(agg)
            n = self.levels[-1].shape[0]
            assert len(agg) == n and agg.min() == 0
            P = np.zeros((n, int(agg.max()) + 1), dtype)
            P[np.arange(n), agg] = 1
            self.P.append(P)
            self.levels.append(P.T @ self.levels[-1] @ P)
        self.omega = dtype(OMEGA_NUM) / dtype(OMEGA_DEN)
        self.damp = dtype(DAMP)              # (1.6 as the double both implementations hold)
        self.pilu = self._scalar_ilu0(Ap) if ilu0_level0 and len(self.levels) > 1 else None
        self.bilu = self._block_ilu0()

    # ---- factorisations on the pattern, plain IKJ ------------------------------------------------------------------------------------
    def _scalar_ilu0(self, Ap):
        F, n = Ap.copy(), Ap.shape[0]
        idx = np.arange(n)
        for i in range(n):
            for k in idx[self.mask[i] & (idx < i)]:
                F[i, k] = F[i, k] / F[k, k]
                js = self.mask[i] & (idx > k)
                F[i, js] -= F[i, k] * F[k, js]       # (row k holds nothing outside its own pattern)
        return F

    def _block_ilu0(self):
        Nb, idx = self.Nb, np.arange(self.Nb)
        F = self.A.copy().reshape(Nb, 3, Nb, 3)
        for i in range(Nb):
            for k in idx[self.mask[i] & (idx < i)]:
                # L_ik = A_ik U_kk^-1, i.e. U_kk^T L_ik^T = A_ik^T
                Lik = solve_dense(F[k, :, k, :].T, F[i, :, k, :].T, self.dtype).T
                F[i, :, k, :] = Lik
                for j in idx[self.mask[i] & self.mask[k] & (idx > k)]:
                    F[i, :, j, :] -= Lik @ F[k, :, j, :]
        return F

    def _block_ilu0_solve(self, R):
        Nb, idx, F = self.Nb, np.arange(self.Nb), self.bilu
        Y = np.array(R, dtype=self.dtype).reshape(Nb, 3, -1)
        for i in range(Nb):
            for k in idx[self.mask[i] & (idx < i)]:
                Y[i] -= F[i, :, k, :] @ Y[k]
        for i in range(Nb - 1, -1, -1):
            for j in idx[self.mask[i] & (idx > i)]:
                Y[i] -= F[i, :, j, :] @ Y[j]
            Y[i] = solve_dense(F[i, :, i, :], Y[i], self.dtype)
        return Y.reshape(3 * Nb, -1)

    # ---- the cycle ---------------------------------------------------------------------------------------------------------------------
    def _smooth(self, l, B):
        A = self.levels[l]
        if l == 0 and self.pilu is not None:
            F, n = self.pilu, A.shape[0]
            X = B.copy()
            for i in range(1, n):
                X[i] -= F[i, :i] @ X[:i]
            for i in range(n - 1, -1, -1):
                X[i] = (X[i] - F[i, i + 1:] @ X[i + 1:]) / F[i, i]
            return X
        return self.omega * B / np.diag(A)[:, None]

    def vcycle(self, B, l=0):
        A = self.levels[l]
        if l + 1 == len(self.levels):
            return solve_dense(A, B, self.dtype)
        P = self.P[l]
        X = self._smooth(l, B)
        X = X + self.damp * (P @ self.vcycle(P.T @ (B - A @ X), l + 1))
        return X + self._smooth(l, B - A @ X)

    def apply(self, D):
        """M^-1 applied to the columns of D (or to one vector)"""
        one = np.ndim(D) == 1
        D = np.array(D, dtype=self.dtype).reshape(3 * self.Nb, -1)
        D3 = D.reshape(self.Nb, 3, -1)
        Rp = D3[:, 0] * self.w[:, 0:1] + D3[:, 1] * self.w[:, 1:2] + D3[:, 2] * self.w[:, 2:3]
        Xc = self.vcycle(Rp)
        V = np.zeros_like(D3)
        V[:, PRESSURE] = Xc
        V = V.reshape(3 * self.Nb, -1)
        V = V + self._block_ilu0_solve(D - self.A @ V)
        return V[:, 0] if one else V


def probes(Nb, seed):
    """the vectors every comparison uses, as columns: two random ones at scales 1 and 1e-3, and unit vectors - first, last and an interior
    cell, each of the three components (a dropped entry is not averaged away in the image of a unit vector)"""
    rng = np.random.default_rng(seed)
    cols = [rng.standard_normal(3 * Nb), 1e-3 * rng.standard_normal(3 * Nb)]
    for cell in sorted({0, Nb // 2, Nb - 1}):
        for k in range(3):
            e = np.zeros(3 * Nb)
            e[3 * cell + k] = 1.0
            cols.append(e)
    return np.ascontiguousarray(np.array(cols).T)


FACTOR = 16.0   # another elimination and summation order than the dense form's (the factor of test_badly_scaled_rows, for the same reason)


def error_ratios(v, v_ld, v_f64):
    """per probe (column) and component class (Sw, p, X): max|v - v_ld| / max(e_ref, eps max|v_ld|), e_ref = max|v_f64 - v_ld| the dense
    form's own float64 error against its longdouble evaluation.  -> array (columns, 3)"""
    eps = np.finfo(np.float64).eps
    n = v_ld.shape[0] // 3
    sh = (n, 3, -1)
    v, vl, vf = np.asarray(v).reshape(sh), np.asarray(v_ld).reshape(sh), np.asarray(v_f64).reshape(sh)
    err = np.abs(v.astype(np.longdouble) - vl).max(axis=0)
    e_ref = np.abs(vf.astype(np.longdouble) - vl).max(axis=0)
    yard = np.maximum(e_ref, eps * np.abs(vl).max(axis=0))
    assert np.all(np.isfinite(np.asarray(v_ld, np.float64))) and np.all(yard > 0), "the dense form itself failed"
    return np.asarray(err / yard, np.float64).T


def assert_within(v, v_ld, v_f64, what):
    """the criterion, every probe and component class: max|v - v_ld| <= 16 max(e_ref, eps max|v_ld|); prints and returns the largest ratio"""
    q = error_ratios(v, v_ld, v_f64)
    worst = float(q.max())
    print("%s: largest error ratio %.3g (probe %d, component %d; admitted %g)" % ((what, worst) + tuple(int(t) for t in np.unravel_index(q.argmax(), q.shape)) + (FACTOR,)))
    assert np.all(np.isfinite(np.asarray(v))) and worst <= FACTOR, (what, q)
    return worst

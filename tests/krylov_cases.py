"""Case builders for the BiCGStab edge tests (tests/test_gpu_bicgstab_edges.py; checked on their own, without a GPU, by
tests/test_krylov_cases.py): block systems built without a Python loop over the rows, right-hand sides shaped for the device's ordering,
a restatement of the oracle's two recurrences whose scalar products are summed in extended precision - the yardstick for "only the
summation order differs" -, and the parameters the CPU test settled (the long solve, the family searched for a drifted verdict).
No GPU and no product code in here."""
import numpy as np


def cartesian_pattern_fast(nx, ny, nz):
    """helpers.cartesian_pattern (7-point block pattern, natural order i + nx (j + ny k), columns ascending) without the loop over the
    rows: the same (Nb, rowptr, col)"""
    Nb = nx * ny * nz
    idx = np.arange(Nb, dtype=np.int64).reshape(nz, ny, nx)
    a = np.concatenate([idx[:, :, :-1].reshape(-1), idx[:, :-1, :].reshape(-1), idx[:-1, :, :].reshape(-1)])
    b = np.concatenate([idx[:, :, 1:].reshape(-1), idx[:, 1:, :].reshape(-1), idx[1:, :, :].reshape(-1)])
    d = np.arange(Nb, dtype=np.int64)
    key = np.sort(np.concatenate([d * Nb + d, a * Nb + b, b * Nb + a]))      # (row, col) pairs, row-major
    rows, cols = key // Nb, key % Nb
    rowptr = np.zeros(Nb + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=Nb))
    return Nb, rowptr, cols.astype(np.int32)


def block_row_sums(Nb, rowptr, col, val):
    """(s, diag): s[i, r] = sum of |entries| of scalar row r of block row i over its off-diagonal BLOCKS; diag[i, r] = its diagonal entry"""
    v = val.reshape(-1, 3, 3)
    rows = np.repeat(np.arange(Nb), np.diff(rowptr))
    off = col != rows
    a = np.abs(v).sum(axis=2)
    s = np.stack([np.bincount(rows[off], weights=a[off, r], minlength=Nb) for r in range(3)], axis=1)
    dk = np.flatnonzero(~off)
    assert len(dk) == Nb
    return s, v[dk][:, np.arange(3), np.arange(3)]


def cartesian_block_system(nx, ny, nz, seed=0, dominance=1.5):
    """The kind of system helpers.laplace_block_system makes - Cartesian 7-point pattern, random dense 3x3 blocks with entries in
    (-0.3, 0], diagonal blocks with entries in (-0.1, 0.1) off their diagonal and  dominance (s + 0.5) + U(0, 0.2)  on it, s = the scalar
    row's sum of |entries| over the off-diagonal blocks - built in array operations (not the same bits: the random numbers are drawn in
    another order).  dominance < 1 gives systems on which ILU0-BiCGStab needs many iterations, or none that suffice."""
    rng = np.random.default_rng(seed)
    Nb, rowptr, col = cartesian_pattern_fast(nx, ny, nz)
    val = rng.uniform(-1.0, 0.0, size=(len(col), 3, 3)) * 0.3
    rows = np.repeat(np.arange(Nb), np.diff(rowptr))
    dk = np.flatnonzero(col == rows)
    s, _ = block_row_sums(Nb, rowptr, col, val)
    D = rng.uniform(-0.1, 0.1, size=(Nb, 3, 3))
    D[:, np.arange(3), np.arange(3)] = dominance * (s + 0.5) + rng.uniform(0.0, 0.2, size=(Nb, 3))
    val[dk] = D
    return Nb, rowptr, col, np.ascontiguousarray(val.reshape(-1))


def dominance_margin(Nb, rowptr, col, val):
    """min over the scalar rows of  diagonal entry / (s + 0.5): at least the `dominance` the system was built with"""
    s, d = block_row_sums(Nb, rowptr, col, val)
    return float((d / (s + 0.5)).min())


def scale_rows(Nb, rowptr, val, decades, seed=0):
    """block row i times 10^k_i, k_i an integer drawn from [-decades, decades]: the right-preconditioned operator A M^-1 becomes
    D A M^-1 D^-1 - the same Krylov space in another norm, one whose residual entries span 2 x decades orders of magnitude"""
    if not decades:
        return val
    k = np.random.default_rng(seed).integers(-decades, decades + 1, size=Nb)
    f = np.repeat(10.0 ** k.astype(float), np.diff(rowptr))
    return np.ascontiguousarray((val.reshape(-1, 9) * f[:, None]).reshape(-1))


def heavy_last_row_rhs(b, fr, share=0.1):
    """b with the block row that comes LAST in the device's ordering (natural row fr[-1]) rescaled to carry `share` of |b|^2: the very last
    elements a vector kernel handles - alone in its last workgroup when 3 Nb is just past a multiple of the block - then weigh as much in
    every scalar product as a tenth of the vector"""
    b = np.array(b, float).reshape(-1, 3).copy()
    last = int(fr[-1])
    rest = float((b ** 2).sum() - (b[last] ** 2).sum())
    b[last] *= np.sqrt(share / (1.0 - share) * rest / float((b[last] ** 2).sum()))
    return np.ascontiguousarray(b.reshape(-1))


_DOTS = {"longdouble": lambda a, b: float(np.dot(a.astype(np.longdouble), b.astype(np.longdouble))), "pairwise": lambda a, b: float(np.dot(a, b))}


def bicgstab_longdouble(orc, Nb, rowptr, col, val, b, tol, maxit, w=0.9, fused=False, half_product=False, history=None, prec_val=None,
                        dots="longdouble"):
    """oracle/linalg.hpp's bicgstab / bicgstab_fused_reductions statement for statement with the oracle's own ILU0 application and product
    (orc.ilu0_apply and orc.spmv, or orc.preconditioned_product for the half-product form), the scalar products alone summed in np.longdouble
    and rounded once: the result of ANY summation order up to that order's rounding.  dots="pairwise": numpy's blocked float64 summation
    instead, a third order.  prec_val: the values the ILU0 is factored from where they are not the operator's (block-Jacobi ILU0 of a
    decomposed run: the couplings between the subdomains set to zero).  history: a list that receives, per half iteration, the norm the
    stopping rule saw over |b|.  -> (x, it, converged, reduction)"""
    lu = orc.ilu0_factor(Nb, rowptr, col, val if prec_val is None else prec_val)
    _ldot = _DOTS[dots]

    def prod(d):        # (A M^-1 d, M^-1 d)
        if half_product:
            return orc.preconditioned_product(Nb, rowptr, col, val, lu, d, w=w, mode="post_scale", half_product=True)
        z = orc.ilu0_apply(Nb, rowptr, col, lu, np.ascontiguousarray(d), w=w, mode="post_scale")
        return orc.spmv(Nb, rowptr, col, val, z), z

    n = 3 * Nb
    r, rw, p, v, x = b.copy(), b.copy(), b.copy(), np.zeros(n), np.zeros(n)
    rr = _ldot(r, r)
    norm0 = norm = np.sqrt(rr)
    rho, rhoh, alpha, omega, beta = (rr, rr, 1.0, 1.0, 0.0) if fused else (1.0, 0.0, 1.0, 1.0, 0.0)

    def clamp(q):
        return q if q > 0.0 else (q if q != q else 0.0)

    it = 0.5
    with np.errstate(all="ignore"):
        while it < maxit:
            if not fused:
                rhop, rho = rho, _ldot(rw, r)
                if it > 1:
                    beta = (rho / rhop) * (alpha / omega)
            if it > 1:
                p = (p - omega * v) * beta + r
            v, pw = prod(p)
            if fused:
                s0, s1, s2 = _ldot(v, rw), _ldot(v, v), _ldot(v, r)
                alpha = rho / s0
                rr = clamp((rr - 2.0 * alpha * s2) + alpha * alpha * s1)
                rhoh = rho - alpha * s0
                norm = np.sqrt(rr)
            else:
                alpha = rho / _ldot(rw, v)
            r = r - alpha * v
            x = x + alpha * pw
            if not fused:
                norm = np.sqrt(_ldot(r, r))
            if history is not None:
                history.append(norm / norm0)
            if norm < tol * norm0:
                break
            it += 0.5
            t, s = prod(r)
            if fused:
                s0, s1, s2 = _ldot(t, r), _ldot(t, t), _ldot(t, rw)
                omega = s0 / s1
                rr = clamp((rr - 2.0 * omega * s0) + omega * omega * s1)
                rhop, rho = rho, rhoh - omega * s2
                beta = (rho / rhop) * (alpha / omega)
                norm = np.sqrt(rr)
            else:
                omega = _ldot(t, r) / _ldot(t, t)
            x = x + omega * s
            r = r - omega * t
            if not fused:
                norm = np.sqrt(_ldot(r, r))
            if history is not None:
                history.append(norm / norm0)
            if norm < tol * norm0:
                break
            it += 0.5
        converged = it != maxit + 0.5
        if fused:
            norm = np.sqrt(_ldot(r, r))
            converged = converged and norm < 2.0 * tol * norm0
        return x, it, bool(converged), norm / norm0


def stopping_figures(orc, Nb, rowptr, col, val, b, tol, fused=False):
    """How comparable a solve is in the order it is given in, from the reference alone: (it of the oracle, whether the extended-precision
    and the pairwise sums stop on the same half iteration, the tolerance's figure for x between the oracle and the extended-precision
    sums, the last norm the stopping rule saw over its threshold, the smallest earlier one over it, |b - A x| of the oracle's iterate over
    tol |b|, the largest relative difference of the reported reduction between the three ways of summing)"""
    x, r = orc.solve(Nb, rowptr, col, val, b, tol=tol, maxit=200, w=0.9, fused_reductions=fused)
    h = []
    xl, it, conv, red = bicgstab_longdouble(orc, Nb, rowptr, col, val, b, tol, 200, fused=fused, history=h)
    xp, itp, convp, redp = bicgstab_longdouble(orc, Nb, rowptr, col, val, b, tol, 200, fused=fused, dots="pairwise")
    fig = tolerance_figure(xl, x, 1e-7, 1e-10 * np.abs(x).max()) if fused else tolerance_figure(xl, x, 1e-9, 1e-12)
    true = np.linalg.norm(b - orc.spmv(Nb, rowptr, col, val, x)) / (tol * np.linalg.norm(b))
    dred = max(abs(red - r.reduction), abs(redp - r.reduction)) / r.reduction
    return r.it, bool(r.converged) and r.it == it == itp, fig, h[-1] / tol, (min(h[:-1]) if len(h) > 1 else np.inf) / tol, true, dred


def long_enough(figs, halves, rtol, below, above):
    """long, comparable (order sensitivity a hundredth of the tolerance), stopping clear of the threshold - the norm of the last half
    iteration under `below` of it, every earlier one over `above` of it - and ending in a solution: |b - A x| < tol |b| for the oracle's
    own iterate (fused: < 2 tol |b|, its verdict's bound)"""
    it, same, fig, last, prev, true, dred = figs
    return bool(2 * it >= halves and same and fig <= rtol / 100.0 and last <= below and prev >= above and true < (1.0 if rtol == 1e-9 else 2.0))


def tolerance_figure(x, xref, rtol, atol):
    """max_i |x_i - xref_i| / (atol / rtol + |xref_i|): the number that np.testing.assert_allclose(x, xref, rtol, atol) compares with rtol"""
    return float(np.max(np.abs(x - xref) / (atol / rtol + np.abs(xref))))


# ---- the systems of tests/test_gpu_bicgstab_edges.py -----------------------------------------------------------------------------------
# builder "helper": helpers.laplace_block_system (the small system of section C, whose oracle results the issue tabulates); else the
# vectorised builder above.  decades / scale_seed: scale_rows.
SMALL = dict(shape=(6, 5, 4), seed=4, rhs_seed=9, builder="helper")
A1 = dict(shape=(41, 40, 40), seed=41, rhs_seed=42)        # 65 600 rows
A2 = dict(shape=(52, 52, 52), seed=52, rhs_seed=53)        # 140 608 rows
# "rest": >= 2050 tiles of 32 rows, so the rest schedule of the half-product form (tiles merged up to 64 rows) has >= 1025 positions
B_SHAPES = {"small": dict(shape=(28, 35, 14), seed=12, rhs_seed=7), "rest": dict(shape=(41, 40, 40), seed=33, rhs_seed=34)}
A4_SIZES = (682, 683, 2048, 2049)
# the long solves (tests/test_krylov_cases.py: test_long_solves_are_long_and_the_smallest_that_are): the default recurrence at 1e-8 needs
# 33.5 / 43.0 / 33.5 iterations in the oracle's natural / graph-coloured / level-scheduled order, the fused one at 1e-6 24.5 / 32.0 / 24.5.
# A solve this long is comparable in `it` only where it stops clear of its threshold in the order it RUNS in, and the device's orders
# exist only on the device: the GPU test takes the first of the candidates below that long_enough() accepts in the device's order,
# judged from the oracle's solves alone (the first one does in every order of the oracle).
LONG_DEFAULT = dict(shape=(16, 12, 10), seed=4, rhs_seed=9, dominance=0.8, decades=3, scale_seed=12, tol=1e-8)
LONG_DEFAULT_CANDIDATES = [LONG_DEFAULT] + [dict(LONG_DEFAULT, dominance=d, decades=k, scale_seed=q) for d, k, q in ((0.82, 1, 12), (0.82, 1, 5), (0.82, 4, 5), (0.85, 4, 12))]
LONG_FUSED = dict(shape=(16, 12, 10), seed=4, rhs_seed=17, dominance=0.8, tol=1e-6)
LONG_FUSED_CANDIDATES = [LONG_FUSED] + [dict(LONG_FUSED, rhs_seed=q) for q in (9, 11, 13, 14)]
LONG_MARGINS = {"default": (0.96, 1.04), "fused": (0.9, 1.1)}
LONG_SMALLER = [(12, 10, 8), (14, 12, 10)]     # the next smaller shapes, which do not do for the default recurrence
# the family searched for a "drifted" verdict of the fused recurrence at 1e-6 (135 systems, milder scalings first); DRIFTED: its first
# member that, in the level-scheduled order, drifts on the same half iteration whichever way the scalar products are summed
DRIFT_TOL = 1e-6


def drift_family():
    for decades in range(9):
        for dominance in (1.5, 1.2, 1.0, 0.9, 0.8):
            for scale_seed in (5, 6, 7):
                yield dict(shape=(6, 5, 4), seed=4, rhs_seed=9, dominance=dominance, decades=decades, scale_seed=scale_seed)


DRIFTED = dict(shape=(6, 5, 4), seed=4, rhs_seed=9, dominance=1.2, decades=3, scale_seed=5)
DRIFT_SLICE = [c for c in drift_family() if 3 <= c["decades"] <= 4]      # 30 systems on one pattern: the verdict's own consistency


def system(case):
    """(Nb, rowptr, col, val, b) of one of the dicts above"""
    if case.get("builder") == "helper":
        from helpers import laplace_block_system
        Nb, rp, ci, v = laplace_block_system(*case["shape"], seed=case["seed"])
    else:
        Nb, rp, ci, v = cartesian_block_system(*case["shape"], seed=case["seed"], dominance=case.get("dominance", 1.5))
    v = scale_rows(Nb, rp, v, case.get("decades", 0), seed=case.get("scale_seed", 0))
    return Nb, rp, ci, v, np.random.default_rng(case["rhs_seed"]).standard_normal(3 * Nb)


def a4_system(Nb):
    """random pattern, rows of varying length: 3 Nb = 2046, 2049, 6144, 6147 elements - one short of, one past one / three blocks of 2048"""
    from helpers import random_block_system
    n, rp, ci, v = random_block_system(Nb, pattern="random", seed=Nb, extra=3)
    return n, rp, ci, v, np.random.default_rng(Nb + 1).standard_normal(3 * n)


def in_order(orc, Nb, rp, ci, v, b, reorder):
    """the system permuted into one of the oracle's own orderings ("none": as it is) -> (rowptr, col, val, b, to, fr)"""
    if reorder == "none":
        to = fr = np.arange(Nb, dtype=np.int32)
    else:
        to, fr, _ = orc.reorder(Nb, rp, ci, reorder)
    rr, rc, rv = orc.reorder_matrix(Nb, rp, ci, v, to, fr)
    return rr, rc, rv, np.ascontiguousarray(b.reshape(Nb, 3)[fr].reshape(-1)), to, fr

"""Block ILU(n) (--ilu-fillin-level) on the device at its edges, against two references.

Bits: the oracle's natural-order block ILU0 of the matrix permuted into the device's order and padded with zero blocks to the filled
pattern (tests/test_gpu_ilun.py: compare_factors) - factors, one M^-1 application in both relaxation modes, whole solves.
Correctness, independent of the oracle: the identity ((I + L)(D + U))_ij = A_ij on every (i, j) of the filled pattern in extended
precision, and the exact-LU limit - with n >= Nb the factors are the complete LU, M^-1 = A^-1 and BiCGStab stops after half an iteration.
Shapes are chosen on the CPU with the fill rule restated in tests/test_ilun_pattern.py: n = 2 and 3 in every ordering (refusals
predicted by the rule), filled rows too long for a tile's LDS image (the unstaged branch of tile_row_product, forward and reversed),
patterns without fill, the library's own zero-diagonal fix, a refactorisation, the wells operator, fused reductions, half-iteration
stops, the device-assembled Jacobian, poisoned allocations and 1.25 x 10^5 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_bind
from helpers import laplace_block_system
from test_gpu_ilun import check_against_oracle, compare_factors, padded, spe1_jacobian, zero_diag_fixed
from test_gpu_random_graphs import graph
from test_ilun_pattern import BUDGET, restated_fill

pytestmark = pytest.mark.gpu
ORDERINGS = ["level_scheduling", "graph_coloring", "graph_coloring_greedy", "line_coloring", "distance2", "auto"]
BOTH = (("post_scale", 0.9), ("in_sweep", 0.9))


def rows_of(rp, ci):
    return [set(ci[rp[i]:rp[i + 1]].tolist()) for i in range(len(rp) - 1)]


def to_csr(rows):
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, np.concatenate([sorted(r) for r in rows]).astype(np.int32)


def dominant_system(rows, seed):
    """random 3x3 blocks on the pattern, each row's diagonal block dominant"""
    rp, ci = to_csr(rows)
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (len(ci), 3, 3)) * 0.2
    row = np.repeat(np.arange(len(rows)), np.diff(rp))
    s = np.zeros((len(rows), 3))
    np.add.at(s, row, np.abs(v).sum(axis=2))
    dk = np.flatnonzero(ci == row)
    for e in range(3):
        v[dk, e, e] = 1.5 * (s[:, e] + 0.5) * np.sign(rng.uniform(-1, 1, len(dk)))
    return len(rows), rp, ci, np.ascontiguousarray(v.reshape(-1))


def chains(rp, ci, maxlen):
    """csrc/reorder.cpp: build_chains, restated - chains along each row's farthest mutual lower neighbour"""
    Nb = len(rp) - 1
    succ = np.full(Nb, -1)
    for i in range(Nb):
        last = ci[rp[i + 1] - 1]
        if last > i and ci[rp[last]] == i:
            succ[i] = last
    chain_of, pos = np.full(Nb, -1), np.zeros(Nb, np.int64)
    nid = 0
    for i in range(Nb):
        if chain_of[i] >= 0:
            continue
        cur, k = i, 0
        while cur >= 0 and chain_of[cur] < 0 and k < maxlen:
            chain_of[cur], pos[cur] = nid, k
            k += 1
            cur = succ[cur]
        nid += 1
    return chain_of, pos


def elimination_order(pkg, Nb, rp, ci, reorder):
    """natural row -> position in the order the symbolic ILU(n) eliminates in (reorder.cpp: the fill's base order): the natural order for
    level scheduling, colour by colour otherwise (line colouring: colour, chain, step) - the colours of the same ordering's ILU0 context
    (the ordering does not depend on n; "auto" with n >= 1 is the distance-2 colouring)"""
    if reorder == "level_scheduling":
        return np.arange(Nb)
    s = pkg.capi.HipSolver(reorder="distance2" if reorder == "auto" else reorder)
    s.set_pattern(Nb, rp, ci)
    to, _, rpc = s.ordering()
    chain_length = s.ordering_info()["chain_length"]
    s.close()
    colour = np.searchsorted(np.cumsum(rpc), to, side="right")
    if reorder == "line_coloring":
        chain_of, pos = chains(rp, ci, chain_length)
        ibase = np.lexsort((pos, chain_of, colour))
    else:
        ibase = np.lexsort((np.arange(Nb), colour))
    base = np.empty(Nb, np.int64)
    base[ibase] = np.arange(Nb)
    return base


def split_counts(fill, base):
    """(L blocks, U blocks) of a filled pattern given as (row, column) pairs in natural numbering, in the elimination order base"""
    nl = sum(1 for i, j in fill if base[j] < base[i])
    nu = sum(1 for i, j in fill if base[j] > base[i])
    return nl, nu


def solve_against_oracle(pkg, orc, Nb, rp, ci, v, b, reorder, n, mode="post_scale", w=0.9, tol=1e-8, maxit=400, wells=None, fused=0):
    """ILU(n)-BiCGStab on the device against the oracle's ILU0-BiCGStab of the permuted, padded matrix: the same half iteration, x, and
    a reported reduction that is the true residual's (the operator's, wells included)"""
    s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=n, relax_mode=mode, ilu_relaxation=w, tolerance=tol, maxit=maxit,
                           fused_reductions=fused)
    res = s.solve_system(Nb, rp, ci, np.array(v, np.float64), b, wells=wells)
    x = s.get_result()
    vf = zero_diag_fixed(Nb, rp, ci, v)
    f = s.ilu_factors(values=False)
    prp, pcl, pv, _, fr = padded(orc, Nb, rp, ci, vf, f)
    to = f["to"]
    W = None
    if wells:
        W = dict(wells)
        W["Ccols"] = np.ascontiguousarray(to[wells["Ccols"]], np.int32)
        W["Bcols"] = np.ascontiguousarray(to[wells["Bcols"]], np.int32)
    xo, reso = orc.solve(Nb, prp, pcl, pv, np.ascontiguousarray(b.reshape(Nb, 3)[fr].reshape(-1)), tol=tol, maxit=maxit, w=w, mode=mode,
                         reorder="none", wells=W, fused_reductions=bool(fused))
    xo = xo.reshape(Nb, 3)[to].reshape(-1)
    assert res.converged and reso.converged and res.it == reso.it, (res.it, reso.it)
    np.testing.assert_allclose(x, xo, rtol=1e-6, atol=1e-8 * np.abs(xo).max())
    y = orc.spmv(Nb, rp, ci, vf, x)
    if wells:
        y = orc.wells_apply(wells, x, y)
    true = np.linalg.norm(b - y) / np.linalg.norm(b)
    # fused reductions report the residual vector's own norm; the default recurrence its updated residual, within rounding of the truth.
    # Solves that reach the rounding floor (the exact-LU-like small cases) agree to that floor only: the residual's rounding, |A||x| + |b|
    floor = 32 * np.finfo(np.float64).eps * np.linalg.norm(orc.spmv(Nb, rp, ci, np.abs(vf), np.abs(x)) + np.abs(b)) / np.linalg.norm(b)
    assert abs(res.reduction - true) <= (1e-6 if fused else 1e-4) * true + floor, (res.reduction, true, floor)
    assert true < 2.0 * tol
    s.close()
    return res


# ---- 1 + 2: the exact-LU limit ----------------------------------------------------------------------------------------------------------
EXACT_GRIDS = [(6, 5, 1), (4, 3, 2), (5, 4, 3), (8, 6, 1), (1, 1, 30)]   # natural order: the complete fill fits 8 x nnzb


@pytest.mark.parametrize("shape", EXACT_GRIDS)
def test_fill_level_of_the_size_is_the_exact_lu(pkg, orc, shape):
    Nb, rp, ci, v = laplace_block_system(*shape, seed=sum(shape))
    full = restated_fill(rows_of(rp, ci), np.arange(Nb), Nb)
    _, pcl, _, fr, to, _ = check_against_oracle(pkg, orc, Nb, rp, ci, v, "level_scheduling", n=Nb, modes=(("post_scale", 1.0), ("in_sweep", 1.0)),
                                               fill=None, identity=True)
    assert len(pcl) == len(full)
    s = pkg.capi.HipSolver(reorder="level_scheduling", ilu_fillin_level=Nb, relax_mode="post_scale", ilu_relaxation=1.0)
    s.set_pattern(Nb, rp, ci)
    s.upload_system(v)
    s.ilu0_factor(want_factors=False)
    d = np.random.default_rng(9).standard_normal(3 * Nb)
    z = s.ilu0_apply(d)
    A = np.zeros((3 * Nb, 3 * Nb))
    v3 = v.reshape(-1, 3, 3)
    for i in range(Nb):
        for k in range(rp[i], rp[i + 1]):
            A[3 * i:3 * i + 3, 3 * ci[k]:3 * ci[k] + 3] = v3[k]
    P = (3 * fr[:, None] + np.arange(3)).reshape(-1)                # the permuted matrix, as the device holds it
    zd = np.linalg.solve(A[np.ix_(P, P)], d[P])
    zd_nat = np.empty_like(zd)
    zd_nat[P] = zd
    eps = np.finfo(np.float64).eps
    for cand in (z, zd_nat):                                         # M^-1 d = A^-1 d: a backward-stable residual, as the dense solve's
        r = np.abs((A.astype(np.longdouble) @ cand.astype(np.longdouble)) - d).astype(np.float64)
        bound = 8 * 3 * Nb * eps * (np.abs(A) @ np.abs(cand) + np.abs(d))
        assert np.all(r <= bound), float(np.max(r / bound))
    np.testing.assert_allclose(z, zd_nat, rtol=0, atol=1e3 * 3 * Nb * eps * np.linalg.cond(A) * np.abs(zd_nat).max())
    s.close()
    b = np.random.default_rng(10).standard_normal(3 * Nb)
    for w in (0.9, 1.0):
        g = pkg.capi.HipSolver(reorder="level_scheduling", ilu_fillin_level=Nb, relax_mode="post_scale", ilu_relaxation=w, tolerance=1e-10)
        res = g.solve_system(Nb, rp, ci, v.copy(), b)
        assert res.converged and res.it == 0.5, (w, res.it, res.reduction)
        g.close()


# ---- 3: n = 2 and 3 in every ordering ---------------------------------------------------------------------------------------------------
def level_matrices(pkg, orc):
    out = {}
    for g in [(20, 20, 1), (8, 6, 3), (6, 5, 4)]:
        out["grid%dx%dx%d" % g] = laplace_block_system(*g, seed=g[0] + g[2])
    Nb, rp, ci, j, _ = spe1_jacobian(pkg, orc)
    out["spe1"] = (Nb, rp, ci, j)
    for kind, n, seed in [("random", 65, 11), ("star", 33, 12), ("random", 50, 1)]:
        rp, ci, v = graph(kind, n, np.random.default_rng(seed))
        out["%s%d" % (kind, n)] = (n, rp, ci, v)
    return out


@pytest.fixture(scope="module")
def matrices(pkg, orc):
    return level_matrices(pkg, orc)


ACCEPTED = {}


@pytest.mark.parametrize("name", ["grid20x20x1", "grid8x6x3", "grid6x5x4", "spe1", "random65", "star33", "random50"])
@pytest.mark.parametrize("n", [2, 3])
def test_levels_two_and_three_in_every_ordering(pkg, orc, matrices, name, n):
    Nb, rp, ci, v = matrices[name]
    rows = rows_of(rp, ci)
    nnzb = len(ci)
    outcome = []
    for reorder in ORDERINGS:
        s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=n)
        try:
            s.set_pattern(Nb, rp, ci)
        except pkg.capi.OpmHipError as e:
            assert e.code == pkg.capi.INVALID_ARGUMENT and ("ILU(%d)" % n) in str(e) and "refused" in str(e), str(e)
            base = elimination_order(pkg, Nb, rp, ci, reorder)
            assert restated_fill(rows, base, n, limit=BUDGET * nnzb) is None, (reorder, n)   # the rule's fill is over the budget
            outcome.append((reorder, "refused"))
            continue
        finally:
            s.close()
        check_against_oracle(pkg, orc, Nb, rp, ci, v, reorder, n=n, modes=BOTH, fill=True, identity=True)
        outcome.append((reorder, "accepted"))
        ACCEPTED.setdefault(n, []).append((name, reorder))
    print("ILU(%d) %s: %s" % (n, name, ", ".join("%s %s" % o for o in outcome)))


def test_every_level_had_an_accepted_case():
    # runs after the cases above (file order); on its own it would see nothing
    assert set(ACCEPTED) == {2, 3} and all(len(v) >= 5 for v in ACCEPTED.values()), ACCEPTED


# ---- 4: filled rows longer than a tile's LDS image -------------------------------------------------------------------------------------
def long_row_pattern():
    """every matrix row holds at most 224 blocks (the ILU0 tile limit); in natural order the fill gives row 2 440 U blocks (rows 0 and 1
    pivot it) and row 940 442 L blocks"""
    N = 941
    rows = [{i} for i in range(N)]
    rows[0] |= set(range(500, 720))
    rows[1] |= set(range(720, 940))
    rows[2] |= {0, 1}
    rows[940] |= {0, 1}
    return rows


@pytest.mark.parametrize("reorder", ["level_scheduling", "graph_coloring_greedy", "line_coloring", "distance2"])
@pytest.mark.parametrize("n", [1, 2])
def test_filled_rows_too_long_for_lds(pkg, orc, reorder, n):
    rows = long_row_pattern()
    Nb, rp, ci, v = dominant_system(rows, seed=41 + n)
    assert np.diff(rp).max() <= 224
    b = np.random.default_rng(43).standard_normal(3 * Nb)
    for mode, w in BOTH:
        s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=n, relax_mode=mode, ilu_relaxation=w)
        s.set_pattern(Nb, rp, ci)
        s.upload_system(v)
        s.ilu0_factor(want_factors=False)
        f = s.ilu_factors(values=False)
        # the precondition: a row of L and a row of U with more blocks than a staged tile holds (TILE_CAP_BLOCKS + 1 = 225, plus the
        # alignment block), so the forward and the backward sweep both read a row from memory
        assert np.diff(f["lrowptr"]).max() >= 226 and np.diff(f["urowptr"]).max() >= 226, (np.diff(f["lrowptr"]).max(), np.diff(f["urowptr"]).max())
        compare_factors(orc, s, Nb, rp, ci, v, mode, w, fill=True, identity=True)
        s.close()
        solve_against_oracle(pkg, orc, Nb, rp, ci, v, b, reorder, n, mode=mode, w=w, tol=1e-10)


# ---- 5: patterns with no fill, or hardly any -------------------------------------------------------------------------------------------
def degenerate(name):
    if name.startswith("grid"):
        shape = tuple(int(t) for t in name[4:].split("x"))
        return laplace_block_system(*shape, seed=len(name))
    if name == "chain40":
        return dominant_system([{i, i - 1, i + 1} & set(range(40)) for i in range(40)], seed=3)
    if name == "blockdiag50":
        return dominant_system([{i} for i in range(50)], seed=4)
    if name == "pairs30":   # 2 x 2 block-diagonal rows: independent pairs of coupled cells
        return dominant_system([{i, i ^ 1} for i in range(30)], seed=5)
    raise KeyError(name)


@pytest.mark.parametrize("reorder", ["level_scheduling", "distance2"])
@pytest.mark.parametrize("name", ["grid1x1x1", "grid2x1x1", "grid1x1x7", "grid3x2x1", "grid1x33x1", "grid2x2x2", "chain40", "blockdiag50", "pairs30"])
@pytest.mark.parametrize("n", [1, 2])
def test_degenerate_patterns(pkg, orc, name, reorder, n):
    Nb, rp, ci, v = degenerate(name)
    rows = rows_of(rp, ci)
    s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=n)
    s.set_pattern(Nb, rp, ci)
    info = s.ilu_info()
    s.close()
    base = elimination_order(pkg, Nb, rp, ci, reorder)
    fill = restated_fill(rows, base, n)
    assert (info["nl"], info["nu"]) == split_counts(fill, base), (info, split_counts(fill, base))
    assert info["nl"] + info["nu"] + Nb == len(fill)
    check_against_oracle(pkg, orc, Nb, rp, ci, v, reorder, n=n, modes=BOTH, fill=len(fill) > len(ci), identity=True)
    b = np.random.default_rng(Nb).standard_normal(3 * Nb)
    solve_against_oracle(pkg, orc, Nb, rp, ci, v, b, reorder, n, tol=1e-10)


# ---- 6 + 7: the library's zero-diagonal fix, refactorisation ---------------------------------------------------------------------------
def with_zero_diagonals(Nb, rp, ci, v, cells):
    """cells[0]: an all-zero diagonal block in a row and column of its own (its couplings zeroed); the others: zeros on the diagonal of
    the diagonal block only"""
    v = np.array(v, np.float64).reshape(-1, 3, 3)
    row = np.repeat(np.arange(Nb), np.diff(rp))
    iso = cells[0]
    v[(row == iso) | (ci == iso)] = 0.0
    for c in cells[1:]:
        k = rp[c] + int(np.nonzero(ci[rp[c]:rp[c + 1]] == c)[0][0])
        v[k][np.arange(3), np.arange(3)] = 0.0
        v[k] += np.array([[0, 2.0, 0.5], [0.5, 0, 2.0], [2.0, 0.5, 0]]) * np.abs(v[k]).max(initial=1.0)
    return np.ascontiguousarray(v.reshape(-1))


@pytest.mark.parametrize("reorder", ["level_scheduling", "distance2"])
@pytest.mark.parametrize("n", [1, 2])
def test_zero_diagonal_fix_on_the_device(pkg, orc, reorder, n):
    Nb, rp, ci, v0 = laplace_block_system(6, 5, 4, seed=21)
    cells = [37, 50, 88]
    v = with_zero_diagonals(Nb, rp, ci, v0, cells)
    check_against_oracle(pkg, orc, Nb, rp, ci, v, reorder, n=n, modes=BOTH, identity=True, device_fix=True)
    s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=n)
    s.set_pattern(Nb, rp, ci)
    s.upload_system(v)
    e = np.zeros(3 * Nb)
    e[3 * cells[0]:3 * cells[0] + 3] = 1.0
    assert np.array_equal(s.spmv(e).reshape(-1, 3)[cells[0]], np.full(3, 1e-15))   # the fix is in the matrix the operator reads
    s.close()


@pytest.mark.parametrize("n", [1, 2])
def test_refactorisation_on_one_context(pkg, orc, n):
    Nb, rp, ci, v0 = laplace_block_system(8, 6, 3, seed=31)
    s = pkg.capi.HipSolver(reorder="distance2", ilu_fillin_level=n)
    s.set_pattern(Nb, rp, ci)
    rng = np.random.default_rng(32)
    clean2 = laplace_block_system(8, 6, 3, seed=33)[3]
    for v in (v0, with_zero_diagonals(Nb, rp, ci, v0 * rng.uniform(0.9, 1.1, v0.shape), [17, 60]), clean2):
        s.upload_system(v)
        s.ilu0_factor(want_factors=False)
        compare_factors(orc, s, Nb, rp, ci, zero_diag_fixed(Nb, rp, ci, v), "post_scale", 0.9, identity=True)
    s.close()


# ---- 8: solve paths ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_wells_operator(pkg, orc, n):
    Nb, rp, ci, v = laplace_block_system(16, 14, 9, seed=14)
    if n == 2:
        Nb, rp, ci, v = laplace_block_system(12, 10, 6, seed=14)
    rng = np.random.default_rng(15)
    nw, perf = 3, 4
    cells = rng.choice(Nb, size=nw * perf, replace=False).astype(np.int32)
    W = dict(numWells=nw, val_pointers=np.arange(0, nw * perf + 1, perf, dtype=np.int32), Ccols=cells.copy(), Bcols=cells.copy(),
             Cnnzs=rng.uniform(-0.05, 0.05, nw * perf * 12), Bnnzs=rng.uniform(-0.05, 0.05, nw * perf * 12),
             Dnnzs=np.concatenate([(np.eye(4) + rng.uniform(-0.1, 0.1, (4, 4))).reshape(-1) for _ in range(nw)]))
    b = rng.standard_normal(3 * Nb)
    for reorder in ("distance2", "level_scheduling" if n == 1 else "graph_coloring_greedy"):   # natural-order ILU(2) of a 3-D grid is refused
        for fused in (0, 1):
            solve_against_oracle(pkg, orc, Nb, rp, ci, v, b, reorder, n, tol=1e-6, wells=W, fused=fused)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("n", [1, 2])
def test_whole_and_half_iteration_stops(pkg, orc, n, fused):
    Nb, rp, ci, v = laplace_block_system(20, 16, 4, seed=6)
    b = np.random.default_rng(7).standard_normal(3 * Nb)
    kinds = set()
    for reorder in ("distance2", "graph_coloring_greedy"):
        for tol in (0.2, 0.05, 1e-2, 2e-3, 1e-4, 1e-6):
            res = solve_against_oracle(pkg, orc, Nb, rp, ci, v, b, reorder, n, tol=tol, fused=fused)
            kinds.add(res.it % 1.0)
    assert kinds == {0.0, 0.5}


# ---- 9: the device-assembled Jacobian ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,reorder", [(1, "distance2"), (1, "level_scheduling"), (2, "distance2"), (2, "graph_coloring_greedy")])
def test_device_assembled_jacobian(pkg, orc, n, reorder):
    case = pkg.decks.cartesian_case(12, 10, 6, state="mixed", heterogeneous=True)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=100.0)
    m = pkg.capi.HipModel(case, reorder=reorder, ilu_fillin_level=n, tolerance=1e-8, maxit=400)
    o = oracle_bind.OracleModel(orc, case)
    for q in (m, o):
        q.set_state(case["pv"], case["meaning"])
        q.set_source(src)
    jm, rm = m.assemble(86400.0, 0)
    jo, ro = o.assemble(86400.0, 0)
    assert np.array_equal(jm, jo) and np.array_equal(rm, ro)
    res = m.solve_jacobian_system()
    Nb, rp, ci = case["Nb"], case["rowptr"], case["col"]
    jf = zero_diag_fixed(Nb, rp, ci, jo)
    prp, pcl, pv, fr, to, _ = compare_factors(orc, m, Nb, rp, ci, jf, "post_scale", 0.9, identity=True)
    xo, reso = orc.solve(Nb, prp, pcl, pv, np.ascontiguousarray(ro.reshape(Nb, 3)[fr].reshape(-1)), tol=1e-8, maxit=400, w=0.9, reorder="none")
    xo = xo.reshape(Nb, 3)[to].reshape(-1)
    assert res.converged and reso.converged and res.it == reso.it, (res.it, reso.it)
    np.testing.assert_allclose(m.get_result(), xo, rtol=1e-6, atol=1e-8 * np.abs(xo).max())


@pytest.mark.parametrize("n", [1, 2])
def test_zero_diagonal_fix_of_the_device_assembled_jacobian(pkg, orc, n):
    """tests/test_gpu_assembly.py's cut-off cell with ILU(n): k_ilun_scatter puts 1e-15 on the all-zero diagonal block it scatters - in
    the factors and in the matrix the operator reads"""
    case = pkg.decks.cartesian_case(6, 5, 4, state="mixed", heterogeneous=True)
    cut = 37
    rp, ci = np.asarray(case["rowptr"]), np.asarray(case["col"])
    case["poro"] = np.asarray(case["poro"], float).copy()
    case["poro"][cut] = 0.0
    tr = np.asarray(case["trans"], float).copy()
    tr[rp[cut]:rp[cut + 1]] = 0.0
    tr[ci == cut] = 0.0
    case["trans"] = tr
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=50.0)
    src.reshape(-1, 3)[cut] = 0.0
    m = pkg.capi.HipModel(case, reorder="distance2", ilu_fillin_level=n)
    o = oracle_bind.OracleModel(orc, case)
    for q in (m, o):
        q.set_state(case["pv"], case["meaning"])
        q.set_source(src)
    jm, rm = m.assemble(86400.0, 0)
    jo, ro = o.assemble(86400.0, 0)
    assert np.array_equal(jm, jo) and np.array_equal(rm, ro)
    Nb = case["Nb"]
    kd = [k for k in range(rp[cut], rp[cut + 1]) if ci[k] == cut][0]
    assert np.all(jm.reshape(-1, 9)[kd] == 0.0)
    res = m.solve_jacobian_system()
    jf = zero_diag_fixed(Nb, rp, ci, jo)
    prp, pcl, pv, fr, to, _ = compare_factors(orc, m, Nb, rp, ci, jf, "post_scale", 0.9, identity=True)
    xo, reso = orc.solve(Nb, prp, pcl, pv, np.ascontiguousarray(ro.reshape(Nb, 3)[fr].reshape(-1)), tol=1e-2, maxit=200, w=0.9, reorder="none")
    xo = xo.reshape(Nb, 3)[to].reshape(-1)
    assert res.converged and reso.converged and res.it == reso.it
    x = m.get_result()
    assert np.all(np.isfinite(x)) and np.all(x.reshape(-1, 3)[cut] == 0.0)
    np.testing.assert_allclose(x, xo, rtol=1e-8, atol=1e-12 * np.abs(xo).max())
    e = np.zeros(3 * Nb)
    e[3 * cut:3 * cut + 3] = 1.0
    assert np.array_equal(m.spmv(e).reshape(-1, 3)[cut], np.full(3, 1e-15))


# ---- 10: poisoned allocations ------------------------------------------------------------------------------------------------------------
def test_ilun_solves_under_poisoned_allocations(tmp_path):
    """OPMHIP_POISON_ALLOC=1: every floating-point device array starts as NaNs - an ILU(2) solve and two ILU(1) Newton iterations of the
    device-assembled path read nothing they have not written: the same bits as without the switch"""
    code = r'''
import importlib, sys
import numpy as np
sys.path.insert(0, "tests")
from helpers import laplace_block_system
pkg = importlib.import_module("opm-autodiff_amd")
out = []
Nb, rp, ci, v = laplace_block_system(12, 10, 6, seed=3)
b = np.random.default_rng(4).standard_normal(3 * Nb)
for kw in (dict(reorder="distance2"), dict(reorder="graph_coloring_greedy", relax_mode="in_sweep")):
    s = pkg.capi.HipSolver(tolerance=1e-8, maxit=200, ilu_fillin_level=2, **kw)
    res = s.solve_system(Nb, rp, ci, v.copy(), b)
    out.append(np.concatenate([[res.it, float(res.converged)], s.get_result()]))
case = pkg.decks.cartesian_case(9, 8, 6, state="mixed", heterogeneous=True)
m = pkg.capi.HipModel(case, tolerance=1e-6, ilu_fillin_level=1)
m.set_state(case["pv"], case["meaning"])
m.set_source(pkg.decks.five_spot_source(case, rate_sm3_per_day=20.0))
for it in range(2):
    m.assemble(86400.0, it, fetch=False)
    res = m.solve_jacobian_system()
    out.append(np.concatenate([[res.it, float(res.converged)], m.get_result()]))
    m.update(None, 1.0)
out.append(m.get_state()[0])
np.save(sys.argv[1], np.concatenate(out))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = []
    for tag, extra in (("plain", {}), ("poison", {"OPMHIP_TUNING": "1", "OPMHIP_POISON_ALLOC": "1"})):
        f = str(tmp_path / (tag + ".npy"))
        env = dict(os.environ, **extra)
        if not extra:
            env.pop("OPMHIP_POISON_ALLOC", None)
        r = subprocess.run([sys.executable, "-c", code, f], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        if extra:
            assert "OPMHIP_POISON_ALLOC=1 is in force" in r.stderr
        got.append(np.load(f))
    assert np.all(np.isfinite(got[0])) and np.array_equal(got[0], got[1])


# ---- 11: size ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", ["distance2", "line_coloring"])
def test_ilu1_at_125000_rows(pkg, orc, reorder):
    case = pkg.decks.cartesian_case(50, 50, 50, state="mixed", heterogeneous=True)
    m = pkg.capi.HipModel(case, reorder=reorder, ilu_fillin_level=1)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(pkg.decks.five_spot_source(case, rate_sm3_per_day=100.0))
    j, _ = m.assemble(86400.0, 0)
    Nb, rp, ci = case["Nb"], case["rowptr"], case["col"]
    s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=1, relax_mode="in_sweep" if reorder == "line_coloring" else "post_scale")
    s.set_pattern(Nb, rp, ci)
    jf = zero_diag_fixed(Nb, rp, ci, j)
    s.upload_system(jf)
    s.ilu0_factor(want_factors=False)
    assert s.ilu_info()["levels"] > 2
    compare_factors(orc, s, Nb, rp, ci, jf, "in_sweep" if reorder == "line_coloring" else "post_scale", 0.9, identity=True, identity_rows=8000)
    s.close()

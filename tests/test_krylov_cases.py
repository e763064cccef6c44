"""The case builders of tests/krylov_cases.py and the oracle-side facts tests/test_gpu_bicgstab_edges.py leans on, checked without a GPU.

Order sensitivity.  The GPU tests compare the device's solves with the oracle's under the project's tolerances, which rest on "only the
summation order of the scalar products differs".  oracle_bind exposes the threaded recurrence (bicgstab_mt) only behind a black-oil
model, so the yardstick here is krylov_cases.bicgstab_longdouble: the oracle's recurrence, preconditioner and product with the scalar
products summed in np.longdouble.  Largest figures measured (x: max |dx_i| / (atol / rtol + |x_i|), the number assert_allclose compares
with rtol; every system in the natural, the graph-coloured and the level-scheduled order of the oracle, the 140 608-row ones in the first two):
    default recurrence, rtol 1e-9, atol 1e-12        x 1.8e-14 (A1), 1.6e-14 (A2), 1.5e-14 (B), 8.4e-15 (A4), 2.6e-15 (small); reduction 2.7e-12
    fused recurrence, rtol 1e-7, atol 1e-10 max|x|   x 5.2e-11 (A1), 2.4e-10 (A2, both product forms), 2.7e-14 (small)
    decomposed (A3), rtol 1e-6, atol 1e-10 max|x|    x 4.4e-10, reduction 1.1e-12
    long solves                                      x 1e-12 (default, 1e-8), 1.6e-10 (fused, 1e-6)
all at least 100 times below their tolerance, so the tolerances stand.  (The fused recurrence's REPORTED reduction moves by up to 1.1e-6
relative with the summation order at 140 608 rows: the GPU tests hold it against the iterate's own residual, as test_gpu_fused_reductions.py
does, not against the oracle's figure.)

Long solves.  dominance < 0.8 makes solves long but not comparable: at (6, 5, 4) and dominance 0.7 / 0.6 / 0.5 the two summation orders
differ by 3e-7 / 4e-6 / 2e-6 in x at 1e-8 and disagree on the half iteration.  So the dominance was RAISED to 0.8 and the length comes from
the size and a mild row scaling: LONG_DEFAULT = (16, 12, 10), dominance 0.8, rows times 10^k, |k| <= 3: 67 / 86 / 67 half iterations at
1e-8 in the three orders, the three ways of summing agree on the half iteration, x moves by 1e-12 at most, and the oracle's own iterate
is a solution under the plain bound (|b - A x| = 0.69 / 0.97 / 0.69 of tol |b|).  (Wider scalings make longer solves on smaller shapes,
but their iterates are not solutions: with |k| <= 5 at (10, 8, 6) the oracle's leaves 1e-6 |b| at tol 1e-8.)  The residual ends in
rounding, so the REPORTED reduction differs by 8e-2 and more between the ways of summing and is not compared.  (12, 10, 8) and
(14, 12, 10) disagree on the half iteration or move x by 7e-11.  The fused recurrence cannot resolve 1e-6 on row-scaled systems, so it has
a system of its own: LONG_FUSED = (16, 12, 10), dominance 0.8, unscaled, rhs 17: 49 / 64 / 49 half iterations.  ((12, 10, 8) is long
enough and comparable in the oracle's orders, but in the device's line-coloured order its x moves by 2.6e-9 with the way of summing.)
The device's line-coloured order exists only on the device, and in it LONG_DEFAULT's three ways of summing stop on different half
iterations: the GPU test therefore takes the first of krylov_cases.LONG_*_CANDIDATES that krylov_cases.long_enough accepts in the order
the solve runs in, judged from the oracle's solves alone.

The drifted verdict.  Family: (6, 5, 4), seed 4, rhs 9, dominance in {1.5, 1.2, 1.0, 0.9, 0.8} x rows times 10^k, |k| <= 0 ... 8 x three
scalings = 135 systems, fused recurrence at 1e-6.  The oracle reports "recurred norm met the tolerance, true norm >= 2 tol" for about a
third of them in any one order; most of these verdicts hang on the way of summing (the recurred |r|^2 goes through a cancellation that
rounding decides), but in the level-scheduled order six members give the verdict on the same half iteration under serial,
extended-precision and pairwise sums.  DRIFTED, the first of them (dominance 1.2, |k| <= 3, scaling 5): it 5.5, reduction 3.67e-6
against 2 tol = 2e-6 in all three, x to 2.9e-13; the default recurrence converges on it in 6.0 iterations."""
import time

import numpy as np
import pytest

import krylov_cases as K
from helpers import cartesian_pattern

ORDERS = ("none", "graph_coloring", "level_scheduling")


def test_pattern_is_the_helpers():
    for shape in [(6, 5, 4), (1, 1, 5), (3, 1, 1), (7, 3, 2), (1, 1, 1)]:
        Nb, rp, ci = cartesian_pattern(*shape)
        Nb2, rp2, ci2 = K.cartesian_pattern_fast(*shape)
        assert Nb == Nb2 and np.array_equal(rp, rp2) and np.array_equal(ci, ci2) and ci2.dtype == np.int32 and rp2.dtype == np.int32


@pytest.mark.parametrize("dominance", [1.5, 1.0])
def test_builder_is_dominant_quick_and_solvable(orc, dominance):
    t0 = time.perf_counter()
    Nb, rp, ci, v = K.cartesian_block_system(41, 40, 40, seed=41, dominance=dominance)
    assert time.perf_counter() - t0 < 1.0 and Nb == 65600          # (the row loop of helpers.laplace_block_system: 1.4 s)
    # every scalar row: diagonal >= dominance (sum of |entries| over the off-diagonal blocks + 0.5); the rest of the diagonal block small
    assert dominance <= K.dominance_margin(Nb, rp, ci, v) < dominance + 0.4
    blocks = v.reshape(-1, 3, 3)
    rows = np.repeat(np.arange(Nb), np.diff(rp))
    assert np.all(blocks[ci != rows] <= 0.0) and np.all(blocks[ci != rows] > -0.3)
    offd = blocks[ci == rows][:, ~np.eye(3, dtype=bool)]
    assert np.all(np.abs(offd) < 0.1)
    assert K.cartesian_block_system(5, 4, 3, seed=2)[3].tobytes() == K.cartesian_block_system(5, 4, 3, seed=2)[3].tobytes()
    b = np.random.default_rng(42).standard_normal(3 * Nb)
    x, res = orc.solve(Nb, rp, ci, v, b, tol=1e-6, maxit=200, w=0.9)
    assert res.converged and np.linalg.norm(b - orc.spmv(Nb, rp, ci, v, x)) < 1e-6 * np.linalg.norm(b) * (1 + 1e-9)


def test_row_scaling_and_the_heavy_last_row():
    Nb, rp, ci, v, b = K.system(dict(shape=(5, 4, 3), seed=1, rhs_seed=2))
    vs = K.scale_rows(Nb, rp, v, 3, seed=5)
    f = vs.reshape(-1, 9)[:, 0] / v.reshape(-1, 9)[:, 0]
    k = np.rint(np.log10(f))
    assert np.allclose(f, 10.0 ** k, rtol=1e-15) and k.min() == -3 and k.max() == 3
    for i in range(Nb):
        assert len(set(k[rp[i]:rp[i + 1]])) == 1
    assert K.scale_rows(Nb, rp, v, 0) is v
    fr = np.random.default_rng(3).permutation(Nb).astype(np.int32)
    bh = K.heavy_last_row_rhs(b, fr)
    last = int(fr[-1])
    assert abs((bh.reshape(-1, 3)[last] ** 2).sum() / (bh ** 2).sum() - 0.1) < 1e-14
    keep = np.ones(Nb, bool)
    keep[last] = False
    assert np.array_equal(bh.reshape(-1, 3)[keep], b.reshape(-1, 3)[keep])


def test_small_system_on_the_oracle(orc):
    """the rows of the table in section C of the GPU module: what the device is held to, here pinned on the oracle itself"""
    Nb, rp, ci, v, b = K.system(K.SMALL)
    for tol in (0.999, 1.0, 2.0):
        x, r = orc.solve(Nb, rp, ci, v, b, tol=tol, maxit=200, w=0.9)
        assert (r.it, r.iterations, r.converged) == (0.5, 0, 1) and abs(r.reduction - 0.01437) < 5e-6
    x, r = orc.solve(Nb, rp, ci, v, b, tol=0.5, maxit=1, w=0.9)
    assert (r.it, r.iterations, r.converged) == (0.5, 0, 1)
    x, r = orc.solve(Nb, rp, ci, v, b, tol=1e-2, maxit=1, w=0.9)
    assert (r.it, r.iterations, r.converged) == (1.0, 1, 1)
    x, r = orc.solve(Nb, rp, ci, v, b, tol=1e-12, maxit=1, w=0.9)
    assert (r.it, r.iterations, r.converged) == (1.5, 1, 0) and abs(r.reduction - 4.6e-4) < 5e-6
    for fused in (False, True):
        x, r = orc.solve(Nb, rp, ci, v, np.zeros(3 * Nb), tol=1e-2, maxit=5, w=0.9, fused_reductions=fused)
        assert (r.it, r.iterations, r.converged) == (5.5, 5, 0) and np.isnan(r.reduction) and np.isnan(x).all()


def _sensitivity(orc, Nb, rp, ci, v, b, tol, fused=False, half_product=False, maxit=200, prec_val=None, owner=None, history=None):
    """(it of the oracle, it of the extended-precision sums, the tolerance's figure for x, relative difference of the reduction)"""
    x, r = orc.solve(Nb, rp, ci, v, b, tol=tol, maxit=maxit, w=0.9, fused_reductions=fused, half_product=half_product, owner=owner)
    xl, it, conv, red = K.bicgstab_longdouble(orc, Nb, rp, ci, v, b, tol, maxit, fused=fused, half_product=half_product, prec_val=prec_val, history=history)
    if fused or owner is not None:
        fig = K.tolerance_figure(xl, x, 1e-7 if owner is None else 1e-6, 1e-10 * np.abs(x).max())
    else:
        fig = K.tolerance_figure(xl, x, 1e-9, 1e-12)
    assert bool(r.converged) == conv
    return r.it, it, fig, abs(red - r.reduction) / r.reduction


def _check(figs, fused=False, rtol=None):
    it, itl, fig, dred = figs
    rtol = rtol or (1e-7 if fused else 1e-9)
    assert it == itl, figs
    assert fig <= rtol / 100.0, figs
    if not fused:
        assert dred <= 1e-9 / 100.0, figs         # (fused: the reported reduction is held against the iterate's own residual)


SYSTEMS = [("A1", K.A1, ORDERS), ("A2", K.A2, ORDERS[:2]), ("B-small", K.B_SHAPES["small"], ORDERS), ("B-rest", K.B_SHAPES["rest"], ORDERS),
           ("small", K.SMALL, ORDERS)]


@pytest.mark.parametrize("name,case,orders", SYSTEMS, ids=[s[0] for s in SYSTEMS])
def test_summation_order_moves_x_by_less_than_a_hundredth_of_the_tolerance(orc, name, case, orders):
    Nb, rp, ci, v, b = K.system(case)
    for ro in orders:
        rr, rc, rv, rb, to, fr = K.in_order(orc, Nb, rp, ci, v, b, ro)
        _check(_sensitivity(orc, Nb, rr, rc, rv, rb, 1e-6))
        if name in ("A1", "A2", "small"):
            _check(_sensitivity(orc, Nb, rr, rc, rv, rb, 1e-6, fused=True), fused=True)
        if name == "A2":
            _check(_sensitivity(orc, Nb, rr, rc, rv, rb, 1e-6, fused=True, half_product=True), fused=True)
        if name.startswith("B"):
            _check(_sensitivity(orc, Nb, rr, rc, rv, rb, 1e-6, half_product=True))
        if name == "small":
            for tol, maxit in ((1.0, 200), (1e-2, 1), (1e-12, 1)):
                _check(_sensitivity(orc, Nb, rr, rc, rv, rb, tol, maxit=maxit))


@pytest.mark.parametrize("Nb", K.A4_SIZES)
def test_summation_order_on_the_block_boundary_systems(orc, Nb):
    n, rp, ci, v, b = K.a4_system(Nb)
    assert 3 * n in (2046, 2049, 6144, 6147)
    for ro in ("graph_coloring", "level_scheduling"):
        to, fr, _ = orc.reorder(n, rp, ci, ro)
        rr, rc, rv, rb, to, fr = K.in_order(orc, n, rp, ci, v, K.heavy_last_row_rhs(b, fr), ro)
        assert abs((rb[-3:] ** 2).sum() / (rb ** 2).sum() - 0.1) < 1e-14       # the last block row in the order the solve runs in
        _check(_sensitivity(orc, n, rr, rc, rv, rb, 1e-6))


def test_summation_order_on_the_decomposed_case(orc, pkg):
    """A3: two subdomains of 52^3 cells each (test_gpu_dd.global_and_parts(pkg, 52, 2): 104 x 52 x 52 cells).  Building, assembling and
    solving it on the oracle takes 0.8 + 0.5 + 2.1 s on one CPU core; the block-Jacobi ILU0 of the oracle's owner= solve is the ILU0 of the matrix
    with the couplings between the subdomains set to zero"""
    import oracle_bind
    from test_gpu_dd import global_and_parts
    g, owner, parts = global_and_parts(pkg, 52, 2, state="mixed", heterogeneous=True)
    assert [p["Nb"] for p in parts] == [140608, 140608]
    o = oracle_bind.OracleModel(orc, g)
    o.set_state(g["pv"], g["meaning"])
    o.set_source(pkg.decks.five_spot_source(g, rate_sm3_per_day=30.0))
    jo, ro = o.assemble(86400.0, 0)
    rows = np.repeat(np.arange(g["Nb"]), np.diff(g["rowptr"]))
    pv = jo.reshape(-1, 9).copy()
    pv[owner[rows] != owner[g["col"]]] = 0.0
    figs = _sensitivity(orc, g["Nb"], g["rowptr"], g["col"], jo, ro, 1e-4, prec_val=np.ascontiguousarray(pv.reshape(-1)), owner=owner)
    assert figs[0] == figs[1] and figs[2] <= 1e-6 / 100.0 and figs[3] <= 1e-5 / 100.0, figs


def _long(orc, case, fused, shape=None):
    """krylov_cases.stopping_figures per order of the oracle"""
    c = dict(case, shape=shape or case["shape"])
    Nb, rp, ci, v, b = K.system(c)
    out = []
    for ro in ORDERS:
        rr, rc, rv, rb, to, fr = K.in_order(orc, Nb, rp, ci, v, b, ro)
        out.append(K.stopping_figures(orc, Nb, rr, rc, rv, rb, case["tol"], fused=fused))
    return out


def _long_enough(figs, halves, rtol, below, above):
    """krylov_cases.long_enough in every order.  The norms of the row-scaled system (|k| <= 3) differ by up to 0.01 of the threshold between
    the ways of summing (0.96 / 1.04); the fused recurrence's carry eps |r_0|^2 / (tol |r_0|)^2 = 1e-4 relative (0.9 / 1.1)."""
    return all(K.long_enough(f, halves, rtol, below, above) for f in figs)


def test_long_solves_are_long_and_the_smallest_that_are(orc):
    """>= 40 half iterations (ten trips round the four-slot read-back ring) at 1e-8 for the default recurrence, >= 20 at 1e-6 for the fused
    one, in every order of the oracle, with the order sensitivity the tolerances need; the next smaller shapes miss one or the other"""
    assert K.LONG_MARGINS == {"default": (0.96, 1.04), "fused": (0.9, 1.1)}
    assert K.LONG_DEFAULT_CANDIDATES[0] is K.LONG_DEFAULT and K.LONG_FUSED_CANDIDATES[0] is K.LONG_FUSED
    figs = _long(orc, K.LONG_DEFAULT, False)
    assert _long_enough(figs, 40, 1e-9, 0.96, 1.04) and [f[0] for f in figs] == [33.5, 43.0, 33.5], figs
    assert max(f[5] for f in figs) < 0.97                # the oracle's iterates are solutions at 1e-8: 0.69 / 0.97 / 0.69 of the bound
    # the residual of a row-scaled system ends in rounding: the reduction that is REPORTED differs by 1e-2 ... 2e-1 between the ways of
    # summing, against the 1e-11 that a comparison at 1e-9 would need - the GPU test does not compare it
    assert min(f[6] for f in figs) > 1e-5, figs
    for shape in K.LONG_SMALLER:
        assert not _long_enough(_long(orc, K.LONG_DEFAULT, False, shape), 40, 1e-9, 0.96, 1.04)
    figs = _long(orc, K.LONG_FUSED, True)
    assert _long_enough(figs, 20, 1e-7, 0.9, 1.1) and [f[0] for f in figs] == [24.5, 32.0, 24.5], figs
    # what lower dominance would have given: long, but decided by rounding
    Nb, rp, ci, v, b = K.system(dict(K.SMALL, builder=None, dominance=0.6))
    it, itl, fig, dred = _sensitivity(orc, Nb, rp, ci, v, b, 1e-8)
    assert 2 * it >= 40 and fig > 1e-9
    # ... and the fused recurrence on the default's row-scaled system: the recurred norm never gets there
    Nb, rp, ci, v, b = K.system(K.LONG_DEFAULT)
    x, r = orc.solve(Nb, rp, ci, v, b, tol=1e-6, maxit=200, w=0.9, fused_reductions=True)
    assert not r.converged


@pytest.mark.parametrize("case", [K.SMALL, K.A1], ids=["small", "A1"])
@pytest.mark.parametrize("fused", [False, True])
def test_oracle_is_scale_invariant(orc, case, fused):
    """b times 2^k: every operation of either recurrence commutes with a power of two (no absolute constant, no order that depends on
    magnitude), so the oracle's x is ldexp(x, k) bit for bit - the property the device is held to"""
    Nb, rp, ci, v, b = K.system(case)
    x, r = orc.solve(Nb, rp, ci, v, b, tol=1e-6, maxit=200, w=0.9, fused_reductions=fused)
    assert r.converged
    for k in (400, -400, 100, -100):
        xk, rk = orc.solve(Nb, rp, ci, v, np.ldexp(b, k), tol=1e-6, maxit=200, w=0.9, fused_reductions=fused)
        assert rk.it == r.it and rk.converged and rk.reduction == r.reduction and np.array_equal(xk, np.ldexp(x, k))


def _drift(orc, c, ro):
    """one member in one order of the oracle: (it, reduction, x) of the serial, extended-precision and pairwise sums, or None where the
    oracle does not report "drifted" (stopped before maxit, not converged)"""
    tol = K.DRIFT_TOL
    Nb, rp, ci, v, b = K.system(c)
    rr, rc, rv, rb, to, fr = K.in_order(orc, Nb, rp, ci, v, b, ro)
    x, r = orc.solve(Nb, rr, rc, rv, rb, tol=tol, maxit=200, w=0.9, fused_reductions=True)
    if r.it == 200.5 or r.converged:
        return None
    out = [(r.it, r.reduction, x)]
    for dots in ("longdouble", "pairwise"):
        xl, it, conv, red = K.bicgstab_longdouble(orc, Nb, rr, rc, rv, rb, tol, 200, fused=True, dots=dots)
        out.append((it if not conv else -1.0, red, xl))
    return out


def test_drifted_verdict_family_and_its_committed_member(orc):
    """the family of the module docstring in the level-scheduled order (the one the GPU test runs in: on a Cartesian pattern the device's
    level-scheduled ILU0 is the natural-order one): the oracle reports "drifted" for a good part of it, most of those verdicts hang on
    the way of summing, six do not, and DRIFTED is the first of them in the family's order.  On it the default recurrence converges to a
    solution, and the reduction the three ways of summing report agrees to 8.1e-5: a hundredth of the 1e-2 the GPU test holds it to."""
    tol = K.DRIFT_TOL
    family = list(K.drift_family())
    assert len(family) == 135
    drifted, robust = 0, []
    for c in family:
        Nb, rp, ci, v, b = K.system(c)
        assert orc.solve(Nb, rp, ci, v, b, tol=tol, maxit=200, w=0.9)[1].converged
        d = _drift(orc, c, "level_scheduling")
        if d is None:
            continue
        assert d[0][1] >= 2.0 * tol
        drifted += 1
        if len({it for it, red, x in d}) == 1:
            robust.append(c)
    assert drifted >= 30 and len(robust) == 6 and robust[0] == K.DRIFTED, (drifted, robust)
    d = _drift(orc, K.DRIFTED, "level_scheduling")
    assert [it for it, red, x in d] == [5.5, 5.5, 5.5]
    assert max(abs(red - d[0][1]) for it, red, x in d) <= 1e-4 * d[0][1] and 3.6e-6 < d[0][1] < 3.7e-6        # against 2 tol = 2e-6
    assert max(K.tolerance_figure(x, d[0][2], 1e-7, 1e-10 * np.abs(d[0][2]).max()) for it, red, x in d[1:]) <= 1e-9
    Nb, rp, ci, v, b = K.system(K.DRIFTED)
    rr, rc, rv, rb, to, fr = K.in_order(orc, Nb, rp, ci, v, b, "level_scheduling")
    x0, r0 = orc.solve(Nb, rr, rc, rv, rb, tol=tol, maxit=200, w=0.9)
    assert r0.converged and np.linalg.norm(rb - orc.spmv(Nb, rr, rc, rv, x0)) < 0.5 * tol * np.linalg.norm(rb)
    it, itl, fig, dred = _sensitivity(orc, Nb, rr, rc, rv, rb, tol)
    # (the default recurrence's REPORTED reduction moves by 1e-5 with the way of summing on this row-scaled system: the GPU test does not compare it)
    assert it == itl == 6.0 and fig <= 1e-9 / 100.0 and dred > 1e-9 / 100.0, (it, itl, fig, dred)


def test_drift_slice_on_the_oracle(orc):
    """DRIFT_SLICE (30 members, rows times 10^k with |k| <= 3 or 4), which the GPU module runs for the verdict's own consistency: in every
    order of the oracle the default recurrence's iterate is a solution under the plain bound (0.93 of it at most) and the reduction the
    fused recurrence reports is the iterate's own residual to 3.8e-5 relative - the GPU module allows a hundred times that"""
    tol = K.DRIFT_TOL
    assert len(K.DRIFT_SLICE) == 30
    worst_d = worst_f = 0.0
    for c in K.DRIFT_SLICE:
        Nb, rp, ci, v, b = K.system(c)
        for ro in ORDERS:
            rr, rc, rv, rb, to, fr = K.in_order(orc, Nb, rp, ci, v, b, ro)
            nb = np.linalg.norm(rb)
            x0, r0 = orc.solve(Nb, rr, rc, rv, rb, tol=tol, maxit=200, w=0.9)
            assert r0.converged
            worst_d = max(worst_d, np.linalg.norm(rb - orc.spmv(Nb, rr, rc, rv, x0)) / (tol * nb))
            xf, rf = orc.solve(Nb, rr, rc, rv, rb, tol=tol, maxit=200, w=0.9, fused_reductions=True)
            if rf.it != 200.5:
                t = np.linalg.norm(rb - orc.spmv(Nb, rr, rc, rv, xf)) / nb
                worst_f = max(worst_f, abs(rf.reduction - t) / t)
    assert worst_d < 0.95 and worst_f <= 1e-4, (worst_d, worst_f)

"""BiCGStab's scalar stage, vector kernels and stopping rule (csrc/solver.hip: k_bicg_*, k_dots, k_dots3, k_finalize, k_finalize3,
k_reduce_finalize, k_local_sums, finalize(), finalize3(), enqueue_half(), wait_half(), bicgstab()) at the places the ordinary solves of
the suite do not reach.  The reference is the oracle's solve in the device's ordering (helpers.oracle_solve_in_order) under the project's
tolerances - default recurrence: x to rtol 1e-9 / atol 1e-12 and the reduction to 1e-9, fused recurrence: x to rtol 1e-7 / atol
1e-10 max|x| and the reported reduction against the iterate's own residual -, which tests/test_krylov_cases.py shows to be at least 100
times the effect of the scalar products' summation order on every system used here.  Half iteration counts are compared for equality and
every solve that reports convergence is checked to be one: |b - A x| < tol |b| (1 + 1e-9) with the oracle's product.

A. Partial lists past RED1_SINGLE_MAX = 2048 (finalize(): count > 2048 -> k_reduce_finalize, 128 slices + ticket; k_finalize3: its loop
   past FU x VB = 2048).  A tile holds at most 32 rows, a launch of the product leaves one partial per workgroup:
   A1  (41, 40, 40) = 65 600 rows >= 2050 tiles, spmv_pipe_wgs = -1: launch_spmv_part -> k_spmv, one tile per workgroup, count >= 2050:
       FIN_ALPHA and FIN_OMEGA go through k_reduce_finalize.  With the default spmv_pipe_wgs = 2048 the same system is pipelined (more
       than 2048 positions, fewer than 4096: 2 steps, one partial per two tiles, e.g. 8 ceil(1025 / 8) = 1032): k_finalize.  The vector
       kernels leave 97 partials either way.
   A2  (52, 52, 52) = 140 608 rows >= 4394 tiles > spmv_pipe_wgs = 4096: pipelined, steps = ceil(4394 / 4096) = 2, grid >= 2197:
       k_reduce_finalize (default recurrence), k_finalize3's loop past 2048 (fused: the three sums ride in k_spmv_pipe_st<3, .>; in the
       half-product form the rest schedule's tiles hold up to 64 rows, >= 2197 positions, grid >= 2197 whether it takes one step or two).
   A3  two loopback subdomains of 52^3 = 140 608 owned rows each (test_gpu_dd.global_and_parts(pkg, 52, 2): 104 x 52 x 52 cells; >= 4394
       tiles per subdomain), spmv_pipe_wgs = -1: finalize()'s decomposed branch -> k_reduce_finalize in FIN_LOCAL mode -> all-reduce.
       Building, assembling and solving the global case on the oracle: 0.8 + 0.5 + 2.1 s on one CPU core.  (n = 52 is the case the issue
       names; it is not the smallest that crosses 2048 with this helper - n = 41, 68 921 rows and >= 2154 tiles per rank, would.)
   A4  3 Nb = 2046, 2049, 6144, 6147 elements around the vector kernels' block of VB x VPT = 2048, the last block row in the device's
       order carrying a tenth of |b|^2.
   A dropped or doubled slice of >= 2050 about equal partials moves alpha or omega by 5e-4 relative, a lost tail element of A4 by 0.1:
   both far above the 1e-9 on x (the solves run 3 - 5 half iterations; the error enters x in the first).
B. PIPE_MAX_STEPS = 128: (28, 35, 14) = 13 720 rows >= 429 tiles with spmv_pipe_wgs 1 and 2: ceil(429 / wgs) > 128, so steps = 128 and
   the grid, 8 ceil(ceil(429 / 128) / 8) = 8, exceeds the resident count it was asked for.  The rest product of the half-product form
   sizes itself for max(8, wgs) and its schedule merges tiles up to 64 rows, so its clamp needs more than 2 x 1024 plain tiles:
   (41, 40, 40) = 65 600 rows, >= 2050 tiles, >= 1025 rest positions (the test reads the count from product_form()), ceil(1025 / 8) =
   129 > 128, with spmv_pipe_wgs = 8, in both forms.  A mis-sized clamp reads schedule entries past the 128 kept in LDS or leaves tiles
   unvisited: rows of the product wrong.
C. The stopping rule and the driver on the small system (6, 5, 4), seed 4.
D. The fused recurrence's "drifted" verdict on the member of the searched family whose verdict does not hang on the way of summing
   (krylov_cases.DRIFTED, level-scheduled order), against the oracle; and the verdict's own consistency on 30 members.

The library reports a non-finite residual norm - a right-hand side that is zero, or not finite, gives one - as
OPMHIP_CREATE_PRECONDITIONER_FAILED (csrc/capi.cpp: opmhip_solve_system; tests/test_gpu_linalg.py::
test_failure_statuses_of_the_backend_interface holds it to that for a singular pivot), AFTER bicgstab() has returned and filled the result:
section C checks that status together with the result's fields through the C entry point itself."""
import ctypes as C
import time
import uuid

import numpy as np
import pytest

import krylov_cases as K
from helpers import oracle_solve_in_order

pytestmark = pytest.mark.gpu

MAXIT = 200


def _residual_ok(orc, sysm, x, tol):
    """|b - A x| < tol |b| (1 + 1e-9) with the oracle's product"""
    Nb, rp, ci, v, b = sysm
    return np.linalg.norm(b - orc.spmv(Nb, rp, ci, v, x)) < tol * np.linalg.norm(b) * (1 + 1e-9)


def _solve(pkg, sysm, tol, fused=0, maxit=MAXIT, solver=None, **cfg):
    Nb, rp, ci, v, b = sysm
    s = solver or pkg.capi.HipSolver(tolerance=tol, maxit=maxit, fused_reductions=fused, **cfg)
    res = s.solve_system(Nb, rp, ci, v.copy(), b)
    return s, res, s.get_result()


def _oracle(orc, s, sysm, tol, fused=0, maxit=MAXIT):
    Nb, rp, ci, v, b = sysm
    to, fr, _ = s.ordering()
    return oracle_solve_in_order(orc, Nb, rp, ci, v, b, to, fr, tol=tol, maxit=maxit, w=0.9, half_product=s.product_form()["half_product"],
                                 fused_reductions=bool(fused))


def _same_solve(orc, sysm, res, x, ro, xo, tol, fused=0, reduction=True):
    """the device's solve is the oracle's: half iteration, verdict, x and the reported reduction under the module's tolerances"""
    Nb, rp, ci, v, b = sysm
    print("it %.1f / %.1f  converged %d / %d  reduction %.6e / %.6e  max|dx| %.3e" % (res.it, ro.it, res.converged, ro.converged, res.reduction, ro.reduction,
                                                                                     np.abs(x - xo).max()))
    assert res.it == ro.it and res.iterations == ro.iterations and bool(res.converged) == bool(ro.converged)
    if fused:
        np.testing.assert_allclose(x, xo, rtol=1e-7, atol=1e-10 * np.abs(xo).max())
        true = np.linalg.norm(b - orc.spmv(Nb, rp, ci, v, x)) / np.linalg.norm(b)
        if reduction:
            assert abs(res.reduction - true) <= 1e-6 * true
    else:
        np.testing.assert_allclose(x, xo, rtol=1e-9, atol=1e-12)
        if reduction:
            assert abs(res.reduction - ro.reduction) <= 1e-9 * ro.reduction
    if res.converged:
        assert _residual_ok(orc, sysm, x, tol)


@pytest.fixture(scope="module")
def sys_a1():
    return K.system(K.A1)


@pytest.fixture(scope="module")
def sys_a2():
    return K.system(K.A2)


# ---- A. partial lists past 2048 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorder", ["level_scheduling", "graph_coloring", "line_coloring"])
def test_a1_one_tile_per_workgroup_leaves_more_than_2048_partials(pkg, orc, sys_a1, reorder):
    """catches: a slice of k_reduce_finalize dropped or doubled at a chunk boundary (count not a multiple of 128), the ticket not reset
    between the two launches of an iteration, slice sums read before they are visible"""
    assert sys_a1[0] == 65600 and 65600 / 32 >= 2050
    s, res, x = _solve(pkg, sys_a1, 1e-6, reorder=reorder, spmv_pipe_wgs=-1, half_product=-1)
    xo, ro = _oracle(orc, s, sys_a1, 1e-6)
    assert res.converged
    _same_solve(orc, sys_a1, res, x, ro, xo, 1e-6)
    # the same system with short lists (pipelined product in two steps, half as many partials as tiles: k_finalize)
    s2, res2, x2 = _solve(pkg, sys_a1, 1e-6, reorder=reorder, half_product=-1)
    assert res2.it == res.it and res2.converged
    np.testing.assert_allclose(x, x2, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("fused,hp", [(0, -1), (1, -1), (1, 1)])
def test_a2_pipelined_grid_of_more_than_2048_workgroups(pkg, orc, sys_a2, fused, hp):
    """catches: default - as A1, through the pipelined kernel's partials; fused - k_finalize3's loop past 2048 skipped or started at the
    wrong index (partials 2048 ... of all three lists lost: alpha off by some 7 %)"""
    assert sys_a2[0] == 140608 and 140608 / 32 >= 4394 > 4096 and (4394 + 1) // 2 >= 2197 > 2048
    s, res, x = _solve(pkg, sys_a2, 1e-6, fused=fused, reorder="line_coloring", spmv_pipe_wgs=4096, half_product=hp)
    assert s.product_form()["half_product"] == (hp > 0)
    xo, ro = _oracle(orc, s, sys_a2, 1e-6, fused=fused)
    assert res.converged
    _same_solve(orc, sys_a2, res, x, ro, xo, 1e-6, fused=fused)


def test_a3_decomposed_local_sums_of_more_than_2048_partials(pkg, orc):
    """catches: k_reduce_finalize's FIN_LOCAL mode writing its two sums anywhere but the all-reduce's buffer, or skipping the ticket reset
    it shares with the single-GPU modes (every rank's alpha wrong by the same factor: the ranks agree with each other, not with the oracle)"""
    import oracle_bind
    from test_gpu_dd import global_and_parts, run_ranks
    n, world, tol = 52, 2, 1e-4
    g, owner, parts = global_and_parts(pkg, n, world, state="mixed", heterogeneous=True)
    assert all(p["Nb"] == 140608 for p in parts) and 140608 / 32 >= 4394 > 2048
    src = pkg.decks.five_spot_source(g, rate_sm3_per_day=30.0)
    o = oracle_bind.OracleModel(orc, g)
    o.set_state(g["pv"], g["meaning"])
    o.set_source(src)
    dt = 86400.0
    jo, ro = o.assemble(dt, 0)
    xo, reso = orc.solve(g["Nb"], g["rowptr"], g["col"], jo, ro, tol=tol, maxit=MAXIT, w=0.9, owner=owner)
    group = "e" + uuid.uuid4().hex

    def rank_fn(r):
        c = parts[r]
        m = pkg.capi.HipModel(c, comm=("loopback", world, r, group), reorder="level_scheduling", tolerance=tol, spmv_pipe_wgs=-1)
        m.set_state(c["pv"], c["meaning"])
        m.set_source(np.ascontiguousarray(src.reshape(-1, 3)[c["gids"]].reshape(-1)))
        m.assemble(dt, 0, fetch=False)
        sol = m.solve_jacobian_system()
        return sol.it, sol.converged, sol.reduction, m.get_result()
    out = run_ranks(world, rank_fn)
    xg = np.zeros((g["Nb"], 3))
    for r, (it, ok, red, x) in enumerate(out):
        c = parts[r]
        gi = c["gids"][:c["Nb"]]
        print("rank %d: it %.1f / %.1f  reduction %.6e / %.6e" % (r, it, reso.it, red, reso.reduction))
        assert ok and reso.converged and it == reso.it
        np.testing.assert_allclose(x.reshape(-1, 3)[:c["Nb"]], xo.reshape(-1, 3)[gi], rtol=1e-6, atol=1e-10 * np.abs(xo).max())
        assert abs(red - reso.reduction) <= 1e-5 * reso.reduction
        xg[gi] = x.reshape(-1, 3)[:c["Nb"]]
    assert _residual_ok(orc, (g["Nb"], g["rowptr"], g["col"], jo, ro), xg.reshape(-1), tol)


@pytest.mark.parametrize("reorder", ["graph_coloring", "level_scheduling"])
@pytest.mark.parametrize("Nb", K.A4_SIZES)
def test_a4_vector_kernels_at_block_boundaries(pkg, orc, Nb, reorder):
    """catches: the last, partly filled block of k_bicg_init / pupdate / upd1 / upd2 / xhalf skipped or run past n, the last block's
    partial not counted (nb one short): the last block row holds a tenth of |b|^2"""
    n, rp, ci, v, b = K.a4_system(Nb)
    s = pkg.capi.HipSolver(tolerance=1e-6, maxit=MAXIT, reorder=reorder)
    s.set_pattern(n, rp, ci)
    to, fr, _ = s.ordering()
    sysm = (n, rp, ci, v, K.heavy_last_row_rhs(b, fr))
    s, res, x = _solve(pkg, sysm, 1e-6, solver=s)
    xo, ro = _oracle(orc, s, sysm, 1e-6)
    assert res.converged
    _same_solve(orc, sysm, res, x, ro, xo, 1e-6)


# ---- B. the pipelined product's step clamp --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wgs,reorder,hp", [("small", 1, "graph_coloring", -1), ("small", 2, "graph_coloring", -1), ("small", 1, "line_coloring", -1),
                                                  ("small", 2, "line_coloring", -1), ("small", 1, "line_coloring", 1), ("small", 2, "line_coloring", 1),
                                                  ("rest", 8, "line_coloring", 1), ("rest", 8, "line_coloring", -1)])
def test_b_more_tiles_than_128_steps_of_the_resident_workgroups(pkg, orc, shape, wgs, reorder, hp):
    """catches: the clamp min(., PIPE_MAX_STEPS) mis-sized against the grid (a workgroup with more than 128 schedule entries overruns its
    LDS copy; a grid too small leaves tiles unvisited) - rows of A x, and the partials riding in the same kernel, wrong"""
    sysm = K.system(K.B_SHAPES[shape])
    Nb, rp, ci, v, b = sysm
    tiles = -(-3 * Nb // 96)
    assert -(-tiles // wgs) > 128
    s = pkg.capi.HipSolver(tolerance=1e-6, maxit=MAXIT, reorder=reorder, spmv_pipe_wgs=wgs, half_product=hp)
    s.set_pattern(Nb, rp, ci)
    form = s.product_form()
    assert form["half_product"] == (hp > 0)
    if hp > 0 and shape == "rest":        # the rest product's own clamp: ceil(positions / max(8, wgs)) > 128
        print("rest positions", form["rest_positions"])
        assert -(-form["rest_positions"] // max(8, wgs)) > 128
    s.upload_system(v)
    to, fr, _ = s.ordering()
    rr, rc, rv = orc.reorder_matrix(Nb, rp, ci, v, to, fr)
    rng = np.random.default_rng(6)
    xv = rng.standard_normal(3 * Nb)
    yo = orc.spmv(Nb, rr, rc, rv, np.ascontiguousarray(xv.reshape(Nb, 3)[fr].reshape(-1))).reshape(Nb, 3)[to].reshape(-1)
    assert np.array_equal(s.spmv(xv), yo)
    s.ilu0_factor(want_factors=False)
    lu_o = orc.ilu0_factor(Nb, rr, rc, rv)
    d = rng.standard_normal(3 * Nb)
    t, z = s.preconditioned_product(d)
    t_o, z_o = orc.preconditioned_product(Nb, rr, rc, rv, lu_o, np.ascontiguousarray(d.reshape(Nb, 3)[fr].reshape(-1)), w=0.9, mode="post_scale", half_product=hp > 0)
    assert np.array_equal(z, z_o.reshape(Nb, 3)[to].reshape(-1)) and np.array_equal(t, t_o.reshape(Nb, 3)[to].reshape(-1))
    s, res, x = _solve(pkg, sysm, 1e-6, solver=s)
    xo, ro = _oracle(orc, s, sysm, 1e-6)
    assert res.converged
    _same_solve(orc, sysm, res, x, ro, xo, 1e-6)


# ---- C. stopping rule and driver ------------------------------------------------------------------------------------------------------
REORDERS_C = ["line_coloring", "graph_coloring"]


@pytest.fixture(scope="module")
def sys_small():
    return K.system(K.SMALL)


def _raw_solve(pkg, s, sysm):
    """opmhip_solve_system itself: (status, result) - the wrapper raises on a negative status"""
    Nb, rp, ci, v, b = sysm
    res = pkg.capi.Result()
    v, b = np.ascontiguousarray(v, np.float64).copy(), np.ascontiguousarray(b, np.float64)
    rc = pkg.capi.lib().opmhip_solve_system(s._h, 3 * Nb, 9 * len(ci), 3, v.ctypes.data_as(C.c_void_p), rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                            b.ctypes.data_as(C.c_void_p), None, C.byref(res))
    s.Nb, s.nnzb = Nb, len(ci)
    return rc, res


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("reorder", REORDERS_C)
def test_c1_first_half_exits_and_maxit_one(pkg, orc, sys_small, reorder, fused):
    """catches: x of a solve that ends on half iteration 0 formed twice or not at all (k_bicg_xhalf beside the speculative half 1 already
    queued: its k_bicg_upd2 must return on SC_DONE), `it` / `iterations` off by a half at maxit = 1, a stale SC_DONEH"""
    Nb = sys_small[0]
    tiny = 1e-6 if fused else 1e-12           # (the fused recurrence refuses tolerances under 1e-6)
    for tol, maxit, it, iterations, converged in [(0.999, MAXIT, 0.5, 0, 1), (1.0, MAXIT, 0.5, 0, 1), (2.0, MAXIT, 0.5, 0, 1), (0.5, 1, 0.5, 0, 1), (1e-2, 1, 1.0, 1, 1),
                                                  (tiny, 1, 1.5, 1, 0)]:
        s, res, x = _solve(pkg, sys_small, tol, fused=fused, maxit=maxit, reorder=reorder)
        xo, ro = _oracle(orc, s, sys_small, tol, fused=fused, maxit=maxit)
        assert (ro.it, ro.iterations, ro.converged) == (it, iterations, converged), (tol, maxit)     # the table of the issue, in this order too
        _same_solve(orc, sys_small, res, x, ro, xo, tol, fused=fused)
    # b = 0, maxit = 5: every norm is NaN from the first half on
    sysm = sys_small[:4] + (np.zeros(3 * Nb),)
    s = pkg.capi.HipSolver(tolerance=1e-2, maxit=5, reorder=reorder, fused_reductions=fused)
    rc, res = _raw_solve(pkg, s, sysm)
    xo, ro = _oracle(orc, s, sysm, 1e-2, fused=fused, maxit=5)
    assert (ro.it, ro.iterations, ro.converged) == (5.5, 5, 0) and np.isnan(ro.reduction) and np.isnan(xo).all()
    assert rc == pkg.capi.CREATE_PRECONDITIONER_FAILED
    assert (res.it, res.iterations, res.converged) == (5.5, 5, 0) and np.isnan(res.reduction) and np.isnan(s.get_result()).all()


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("reorder", REORDERS_C)
def test_c2_a_solve_that_wraps_the_read_back_ring_many_times(pkg, orc, reorder, fused):
    """catches: a ring slot of half iteration h answered by the record of h - 4 (rb_want / sequence numbers reused), a speculative half
    that is not inert, scalars that degrade over many iterations (beta from a stale rho)"""
    kind = "fused" if fused else "default"
    halves, rtol = (20, 1e-7) if fused else (40, 1e-9)
    s = pkg.capi.HipSolver(tolerance=1e-6 if fused else 1e-8, maxit=MAXIT, fused_reductions=fused, reorder=reorder)
    # A long solve is comparable in `it` only where it stops clear of its threshold IN THE ORDER IT RUNS IN, and the device's orders exist
    # only on the device: the system is the first of the stated candidates (one shape, one pattern) that krylov_cases.long_enough accepts
    # in this order - judged from the oracle's solves alone, before the device has solved anything
    candidates = K.LONG_FUSED_CANDIDATES if fused else K.LONG_DEFAULT_CANDIDATES
    Nb, rp, ci = K.cartesian_pattern_fast(*candidates[0]["shape"])
    s.set_pattern(Nb, rp, ci)
    to, fr, _ = s.ordering()
    for case in candidates:
        sysm = K.system(case)
        Nb, rp, ci, v, b = sysm
        rr, rc, rv = orc.reorder_matrix(Nb, rp, ci, v, to, fr)
        figs = K.stopping_figures(orc, Nb, rr, rc, rv, np.ascontiguousarray(b.reshape(Nb, 3)[fr].reshape(-1)), case["tol"], fused=bool(fused))
        print("candidate", case["dominance"], case.get("decades"), case.get("scale_seed"), case["rhs_seed"],
              "it %.1f same %d x %.1e last %.3f prev %.3f true %.3f dred %.1e" % figs)
        if K.long_enough(figs, halves, rtol, *K.LONG_MARGINS[kind]):
            break
    else:
        raise AssertionError("no stated system is long and comparable in this order")
    s, res, x = _solve(pkg, sysm, case["tol"], solver=s)
    xo, ro = _oracle(orc, s, sysm, case["tol"], fused=fused)
    assert res.converged and 2 * ro.it >= halves
    # (the default's system is row-scaled: the reduction that is REPORTED moves by 8e-2 and more with the way of summing, measured in
    #  tests/test_krylov_cases.py, so it is not compared; the iterate is held to the plain residual bound like every other)
    _same_solve(orc, sysm, res, x, ro, xo, case["tol"], fused=fused, reduction=bool(fused))


def _unusable_rhs(kind, b):
    b = b.copy()
    if kind == "zero":
        b[:] = 0.0
    else:
        b[len(b) // 2] = np.nan if kind == "nan" else np.inf
    return b


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("reorder", REORDERS_C)
@pytest.mark.parametrize("kind", ["zero", "nan", "inf"])
def test_c3_right_hand_sides_the_recurrence_cannot_use(pkg, sys_small, kind, reorder, fused):
    """catches: wait_half polling for a stopping-rule record that a finalize kernel does not write when its norm is not finite, the
    `!isfinite(norm)` break reporting anything but maxit exhausted"""
    sysm = sys_small[:4] + (_unusable_rhs(kind, sys_small[4]),)
    s = pkg.capi.HipSolver(tolerance=1e-2, maxit=5, reorder=reorder, fused_reductions=fused)
    t0 = time.perf_counter()
    rc, res = _raw_solve(pkg, s, sysm)
    dt = time.perf_counter() - t0
    print("status %d, it %.1f, %.3f s" % (rc, res.it, dt))
    assert dt < 5.0                               # (wait_half itself gives up after 120 s)
    # the status opmhip_solve_system gives ANY non-finite norm today.  For b = 0 or a non-finite b it is inherited from the singular-pivot
    # case, not wanted for its own sake: a change of csrc/capi.cpp that reports these as a plain unconverged solve (status 0) is no
    # regression - then change this line, and the like ones in C1 and C4, with it.  The result's fields below are what matters.
    assert rc == pkg.capi.CREATE_PRECONDITIONER_FAILED
    assert (res.converged, res.it, res.iterations) == (0, 5.5, 5) and not np.isfinite(res.reduction)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("reorder", REORDERS_C)
def test_c4_nothing_leaks_from_one_solve_into_the_next(pkg, orc, sys_small, reorder, fused):
    """catches: SC_DONE / SC_DONEH, the ticket, the ring's sequence numbers or NaN scalars surviving into the next solve.  Tolerance and
    maxit belong to the context (there is no setter), so the three kinds of ending come from the values instead, at tol 1e-6, maxit 3: a
    block-diagonal matrix (ILU0 exact: stops on half iteration 0), a weakly dominant one (maxit exhausted), a right-hand side with a NaN;
    then an ordinary solve with new values: the oracle's, and bit for bit that of a fresh context"""
    Nb, rp, ci, v, b = sys_small
    tol, maxit = 1e-6, 3
    rows = np.repeat(np.arange(Nb), np.diff(rp))
    vd = v.reshape(-1, 9).copy()
    vd[ci != rows] = 0.0
    vd = np.ascontiguousarray(vd.reshape(-1))
    vw = K.system(dict(K.SMALL, builder=None, dominance=0.8))[3]
    s = pkg.capi.HipSolver(tolerance=tol, maxit=maxit, reorder=reorder, fused_reductions=fused)
    r1 = s.solve_system(Nb, rp, ci, vd, b)
    assert r1.converged and r1.it == 0.5
    assert _residual_ok(orc, (Nb, rp, ci, vd, b), s.get_result(), tol)
    r2 = s.solve_system(Nb, None, None, vw, b)
    assert not r2.converged and r2.it == 3.5 and r2.iterations == 3
    rc, r3 = _raw_solve(pkg, s, (Nb, rp, ci, v, _unusable_rhs("nan", b)))
    assert rc == pkg.capi.CREATE_PRECONDITIONER_FAILED and r3.it == 3.5
    sysm = (Nb, rp, ci, v * 1.01, b)
    r4 = s.solve_system(Nb, None, None, sysm[3].copy(), b)
    x4 = s.get_result()
    xo, ro = _oracle(orc, s, sysm, tol, fused=fused, maxit=maxit)
    assert r4.converged
    _same_solve(orc, sysm, r4, x4, ro, xo, tol, fused=fused)
    s5, r5, x5 = _solve(pkg, sysm, tol, fused=fused, maxit=maxit, reorder=reorder)
    assert r5.it == r4.it and r5.reduction == r4.reduction and np.array_equal(x5, x4)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("which", ["small", "A1"])
def test_c5_scaling_b_by_a_power_of_two_scales_x(pkg, sys_small, sys_a1, which, fused):
    """catches: an absolute constant in the recurrence or the stopping rule (a floor under a denominator, an epsilon added to a norm), a
    summation whose order depends on magnitudes: x(2^k b) = 2^k x(b) bit for bit, as on the oracle (tests/test_krylov_cases.py)"""
    Nb, rp, ci, v, b = sys_small if which == "small" else sys_a1
    cfg = dict(reorder="line_coloring") if which == "small" else dict(reorder="line_coloring", spmv_pipe_wgs=-1, half_product=-1)
    s = pkg.capi.HipSolver(tolerance=1e-6, maxit=MAXIT, fused_reductions=fused, **cfg)
    r0 = s.solve_system(Nb, rp, ci, v.copy(), b)
    x0 = s.get_result()
    assert r0.converged
    for k in (400, -400, 100, -100):
        rk = s.solve_system(Nb, None, None, v.copy(), np.ldexp(b, k))
        assert rk.converged and rk.it == r0.it and rk.reduction == r0.reduction, (k, rk.it, r0.it, rk.reduction, r0.reduction)
        assert np.array_equal(s.get_result(), np.ldexp(x0, k)), k


# ---- D. the drifted verdict -----------------------------------------------------------------------------------------------------------
def test_d_the_device_reports_the_oracles_drifted_verdict(pkg, orc):
    """catches: the verdict formed from the recurred norm alone (the solve reported as converged), the final norm of the residual vector
    not formed or not read back, `it` reset by the verdict.  DRIFTED in the level-scheduled order: the oracle's fused recurrence meets
    1e-6 on half iteration 5.5 in its recurred norm while the residual vector's is 3.67e-6 >= 2 tol, under every way of summing
    (tests/test_krylov_cases.py: the reduction agrees to 8.1e-5 between them, held here to 1e-2; x to 2.9e-13)"""
    tol = K.DRIFT_TOL
    sysm = K.system(K.DRIFTED)
    Nb, rp, ci, v, b = sysm
    s, res, x = _solve(pkg, sysm, tol, fused=1, reorder="level_scheduling")
    xo, ro = _oracle(orc, s, sysm, tol, fused=1)
    print("it %.1f / %.1f  converged %d / %d  reduction %.6e / %.6e" % (res.it, ro.it, res.converged, ro.converged, res.reduction, ro.reduction))
    assert ro.it == 5.5 and not ro.converged and ro.reduction >= 2.0 * tol
    assert res.it == ro.it and res.iterations == ro.iterations and res.converged == 0
    assert abs(res.reduction - ro.reduction) <= 1e-2 * ro.reduction and res.reduction >= 2.0 * tol
    np.testing.assert_allclose(x, xo, rtol=1e-7, atol=1e-10 * np.abs(xo).max())


def test_d_the_default_recurrence_converges_on_the_drifted_system(pkg, orc):
    """catches: nothing new in the kernels - it shows that the verdict above is the fused recurrence's, not the system's: the default
    recurrence converges on it, on the oracle's half iteration, to a solution.  (Its REPORTED reduction moves by 1e-5 with the way of
    summing on this row-scaled system, tests/test_krylov_cases.py, and is not compared.)"""
    tol = K.DRIFT_TOL
    sysm = K.system(K.DRIFTED)
    s, res, x = _solve(pkg, sysm, tol, reorder="level_scheduling")
    xo, ro = _oracle(orc, s, sysm, tol)
    assert res.converged and ro.converged
    _same_solve(orc, sysm, res, x, ro, xo, tol, reduction=False)


def test_d_verdicts_agree_with_the_iterates_own_residual(pkg, orc):
    """catches: the verdict inverted or dropped on any member (a solve whose residual vector is over 2 tol reported as converged).  An
    extra beside the two tests above: which member drifts hangs on the way of summing for most of the family, so the oracle cannot say,
    but the iterate can.  On the 30 systems of DRIFT_SLICE: the default recurrence converges to a solution; where the fused one stops
    before maxit the reported reduction is the iterate's residual (to 4e-3: a hundred times what the oracle's own solves show,
    tests/test_krylov_cases.py) and `converged` is (reduction < 2 tol)"""
    tol = K.DRIFT_TOL
    sf = pkg.capi.HipSolver(tolerance=tol, maxit=MAXIT, reorder="graph_coloring", fused_reductions=1)
    sd = pkg.capi.HipSolver(tolerance=tol, maxit=MAXIT, reorder="graph_coloring")
    drifted = stopped = 0
    for i, c in enumerate(K.DRIFT_SLICE):
        Nb, rp, ci, v, b = sysm = K.system(c)
        first = i == 0
        rd = sd.solve_system(Nb, rp if first else None, ci if first else None, v.copy(), b)
        assert rd.converged and _residual_ok(orc, sysm, sd.get_result(), tol), c
        rf = sf.solve_system(Nb, rp if first else None, ci if first else None, v.copy(), b)
        if rf.it == MAXIT + 0.5:
            assert not rf.converged
            continue
        stopped += 1
        true = np.linalg.norm(b - orc.spmv(Nb, rp, ci, v, sf.get_result())) / np.linalg.norm(b)
        assert abs(rf.reduction - true) <= 4e-3 * true, (c, rf.reduction, true)
        assert bool(rf.converged) == (rf.reduction < 2.0 * tol), (c, rf.it, rf.reduction)
        drifted += not rf.converged
    print("stopped before maxit: %d of %d, drifted: %d" % (stopped, len(K.DRIFT_SLICE), drifted))
    assert drifted >= 1

"""Block ILU(n) (--ilu-fillin-level, opmhip_set_ilu_fillin_level) on the device against the oracle.

ILU(n) of A is the ILU0 of A padded with explicit zero blocks at the fill positions, taken in the same row order: so the oracle's
natural-order block ILU0 and ILU0-BiCGStab (oracle/linalg.hpp: bilu0_decompose, ilu0_apply, bicgstab), fed the permuted, padded matrix,
check the filled factors (csrc/solver.hip: k_ilun_scatter, k_ilun_factor), one M^-1 application (the tile sweeps over the filled
factors) and whole solves.  The device eliminates every row in ascending column order with the oracle's block products, so the factors
and M^-1 agree bit for bit.  Also: n = 0 through the new call is today's path, ILU(1) needs no more iterations than ILU0 on the
configs[2] Jacobian, the refusals, a 10^6-cell solve in the distance-2 colouring and a Newton loop."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind
from helpers import laplace_block_system, norne_shaped_case

pytestmark = pytest.mark.gpu


def zero_diag_fixed(Nb, rp, ci, v):
    """the matrix with the zero-diagonal fix both sides apply (bda/BdaBridge.cpp:125-161), so the oracle's factorisation sees it too"""
    v = np.array(v, np.float64).reshape(-1, 3, 3)
    rp, ci = np.asarray(rp), np.asarray(ci)
    dk = np.flatnonzero(ci == np.repeat(np.arange(Nb), np.diff(rp)))
    assert len(dk) == Nb
    d = v[dk][:, np.arange(3), np.arange(3)]
    v[dk[:, None], np.arange(3), np.arange(3)] = np.where(d == 0.0, 1e-15, d)
    return np.ascontiguousarray(v.reshape(-1))


def padded(orc, Nb, rp, ci, v, f):
    """A in the device's internal order, padded with zero blocks to the filled pattern of factors f (HipSolver.ilu_factors):
    (rowptr, col, values, positions of L / diagonal / U entries in it)"""
    to = f["to"]
    fr = np.empty_like(to)
    fr[to] = np.arange(Nb, dtype=to.dtype)
    rr, rc, rv = orc.reorder_matrix(Nb, rp, ci, v, to, fr)
    lrp, urp = f["lrowptr"].astype(np.int64), f["urowptr"].astype(np.int64)
    nl, nu = np.diff(lrp), np.diff(urp)
    prp = np.zeros(Nb + 1, np.int64)
    prp[1:] = np.cumsum(nl + 1 + nu)
    lrow, urow = np.repeat(np.arange(Nb), nl), np.repeat(np.arange(Nb), nu)
    lpos = prp[lrow] + np.arange(len(lrow)) - lrp[lrow]
    dpos = prp[:-1] + nl
    upos = prp[urow] + nl[urow] + 1 + np.arange(len(urow)) - urp[urow]
    pcl = np.empty(int(prp[-1]), np.int32)
    pcl[lpos], pcl[dpos], pcl[upos] = f["lcol"], np.arange(Nb), f["ucol"]
    key = np.repeat(np.arange(Nb, dtype=np.int64), np.diff(prp)) * Nb + pcl          # ascending: rows, then L < diagonal < U
    akey = np.repeat(np.arange(Nb, dtype=np.int64), np.diff(rr)) * Nb + rc
    at = np.minimum(np.searchsorted(key, akey), len(key) - 1)
    assert np.array_equal(key[at], akey)                        # every entry of A has its place in the filled pattern
    pv = np.zeros((len(pcl), 3, 3))
    pv[at] = rv.reshape(-1, 3, 3)
    return prp.astype(np.int32), pcl, np.ascontiguousarray(pv.reshape(-1)), (lpos, dpos, upos), fr


def _inv3(m):
    """inverses of a stack of 3x3 blocks in the dtype given (np.linalg.inv has no extended precision)"""
    a, b, c, d, e, g, h, i, k = (m[:, r, s] for r in range(3) for s in range(3))
    co = np.stack([e * k - g * i, -(b * k - c * i), b * g - c * e,
                   -(d * k - g * h), a * k - c * h, -(a * g - c * d),
                   d * i - e * h, -(a * i - b * h), a * e - b * d], axis=1).reshape(-1, 3, 3)
    det = a * co[:, 0, 0] + b * co[:, 1, 0] + c * co[:, 2, 0]
    return co / det[:, None, None]


def ilu_identity_error(prp, pcl, pv, lpos, dpos, upos, f, rows=None):
    """the defining identity of ILU on its pattern, ((I + L)(D + U))_ij = A_ij for every (i, j) of the filled pattern, D = inv(invD),
    all products formed in extended precision: -> max over the pattern of |A - (I + L)(D + U)| / (eps * bound), bound = the magnitudes
    the rounding of the elimination can reach (|L||U| summed over k, the entry's own term, A) times the terms in the entry.  rows: a
    boolean mask of the rows to check (every row by default; a row's identity needs only its own L and the U rows it meets)"""
    ld = np.longdouble
    Nb = len(prp) - 1
    sel = np.ones(Nb, bool) if rows is None else np.asarray(rows, bool)
    L, U, iD = f["L"].astype(ld), f["U"].astype(ld), f["invD"].astype(ld)
    aL, aU, aiD = np.abs(f["L"]), np.abs(f["U"]), np.abs(f["invD"])
    D = _inv3(iD)
    aD = np.abs(D).astype(np.float64)
    A = pv.reshape(-1, 3, 3).astype(ld)
    aA = np.abs(pv.reshape(-1, 3, 3))
    nnz = len(pcl)
    key = np.repeat(np.arange(Nb, dtype=np.int64), np.diff(prp)) * Nb + pcl
    lrow = np.repeat(np.arange(Nb, dtype=np.int64), np.diff(f["lrowptr"]))
    lk = f["lcol"].astype(np.int64)
    urp = f["urowptr"].astype(np.int64)
    cnt = np.where(sel[lrow], urp[lk + 1] - urp[lk], 0)            # every L_ik meets row k of U
    a = np.repeat(np.arange(len(lk)), cnt)
    b = np.arange(len(a)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(urp[lk], cnt)
    tk = lrow[a] * Nb + f["ucol"][b]
    at = np.minimum(np.searchsorted(key, tk), nnz - 1)
    hit = key[at] == tk                                             # products that fall outside the pattern are dropped by ILU
    a, b, at = a[hit], b[hit], at[hit]
    S = np.zeros((nnz, 3, 3), ld)
    M = np.zeros((nnz, 3, 3))
    terms = np.zeros(nnz)
    order = np.argsort(at, kind="stable")
    a, b, at = a[order], b[order], at[order]
    if len(at):
        starts = np.flatnonzero(np.r_[True, at[1:] != at[:-1]])
        S[at[starts]] = np.add.reduceat(np.matmul(L[a], U[b]), starts, axis=0)
        M[at[starts]] = np.add.reduceat(np.matmul(aL[a], aU[b]), starts, axis=0)
        terms[at[starts]] = np.diff(np.r_[starts, len(at)])
    own = np.zeros((nnz, 3, 3), ld)
    aown = np.zeros((nnz, 3, 3))
    ls, us = sel[lrow], sel[np.repeat(np.arange(Nb), np.diff(f["urowptr"]))]
    lp, lc, dp, up = lpos[ls], f["lcol"][ls], dpos[sel], upos[us]
    own[lp] = np.matmul(L[ls], D[lc])
    aown[lp] = np.matmul(np.matmul(aA[lp] + M[lp], aiD[lc]), aD[lc])
    own[dp] = D[sel]
    aown[dp] = np.matmul(np.matmul(aD[sel], aiD[sel]), aD[sel])
    own[up] = U[us]
    aown[up] = aU[us]
    chk = np.repeat(sel, np.diff(prp))
    R = np.abs(A[chk] - S[chk] - own[chk]).astype(np.float64)
    bound = (3.0 * terms[chk] + 8.0)[:, None, None] * (M[chk] + aown[chk] + aA[chk]) * np.finfo(np.float64).eps
    return float(np.max(R / np.maximum(bound, np.finfo(np.float64).tiny)))


IDENTITY_ULPS = 4.0   # ilu_identity_error's bound is already a first-order rounding bound; a few of it


def compare_factors(orc, s, Nb, rp, ci, v, mode, w, fill=True, identity=True, cache=None, identity_rows=None):
    """the factors and one M^-1 application of context s (v, the matrix it factored - the zero-diagonal fix applied - uploaded or
    assembled, factored) against the oracle's ILU0 of the permuted matrix padded to the filled pattern: bit for bit.  fill: True - the
    pattern has fill, False - none, None - either.  identity: the ILU identity in extended precision as well.  cache: a dict that keeps
    the padded matrix and the oracle's factors for the next call with the same filled pattern (another relaxation mode).  identity_rows:
    check the identity on that many rows drawn at random (large systems: the products in extended precision are slow)"""
    info = s.ilu_info()
    assert not s.product_form()["half_product"] and not s.product_form()["u_is_upper_a"]
    f = s.ilu_factors()
    assert len(f["lcol"]) == info["nl"] and len(f["ucol"]) == info["nu"]
    assert s.ordering_info()["colors"] == info["levels"]
    same = cache is not None and "f" in cache and all(np.array_equal(cache["f"][k], f[k]) for k in ("to", "lrowptr", "lcol", "urowptr", "ucol"))
    if same:
        prp, pcl, pv, (lpos, dpos, upos), fr, lu_o = cache["padded"]
    else:
        prp, pcl, pv, (lpos, dpos, upos), fr = padded(orc, Nb, rp, ci, v, f)
        lu_o = orc.ilu0_factor(Nb, prp, pcl, pv).reshape(-1, 3, 3)
        if cache is not None:
            cache.update(f=f, padded=(prp, pcl, pv, (lpos, dpos, upos), fr, lu_o))
    if fill is not None:
        assert (len(pcl) > len(ci)) == fill                     # there is fill / there is none
    for dev, ora in ((f["L"], lu_o[lpos]), (f["U"], lu_o[upos]), (f["invD"], lu_o[dpos])):
        np.testing.assert_allclose(dev, ora, rtol=1e-12, atol=1e-12 * max(np.abs(ora).max(initial=0.0), 1e-300))
        assert np.array_equal(dev, ora)                         # same elimination order, same block products
    if identity and not same:
        rows = None
        if identity_rows is not None and identity_rows < Nb:
            rows = np.zeros(Nb, bool)
            rows[np.random.default_rng(6).choice(Nb, identity_rows, replace=False)] = True
        err = ilu_identity_error(prp, pcl, pv, lpos, dpos, upos, f, rows)
        assert err <= IDENTITY_ULPS, err
    to = f["to"]
    d = np.random.default_rng(5).standard_normal(3 * Nb)
    z = s.ilu0_apply(d)
    zo = orc.ilu0_apply(Nb, prp, pcl, lu_o.reshape(-1), np.ascontiguousarray(d.reshape(Nb, 3)[fr].reshape(-1)), w=w, mode=mode)
    assert np.array_equal(z, zo.reshape(Nb, 3)[to].reshape(-1))
    return prp, pcl, pv, fr, to, f


def check_against_oracle(pkg, orc, Nb, rp, ci, v, reorder, n=1, modes=(("post_scale", 0.9), ("in_sweep", 0.9)), fill=True, identity=False,
                         device_fix=False):
    """device_fix: the matrix goes up as it is and the library's zero-diagonal fix must make it the oracle's"""
    vf = zero_diag_fixed(Nb, rp, ci, v)
    cache = {}
    for mode, w in modes:
        s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=n, relax_mode=mode, ilu_relaxation=w)
        s.set_pattern(Nb, rp, ci)
        assert s.ilu_info()["fill_level"] == n
        s.upload_system(np.array(v, np.float64) if device_fix else vf)
        s.ilu0_factor(want_factors=False)
        prp, pcl, pv, fr, to, _ = compare_factors(orc, s, Nb, rp, ci, vf, mode, w, fill=fill, identity=identity, cache=cache)
        s.close()
    return prp, pcl, pv, fr, to, vf


def spe1_jacobian(pkg, orc):
    case = pkg.decks.spe1_case()
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    j, r = o.assemble(86400.0, 0)
    return case["Nb"], case["rowptr"], case["col"], j, r


def cartesian_jacobian(pkg, orc, nx, ny, nz):
    case = pkg.decks.cartesian_case(nx, ny, nz, state="mixed", heterogeneous=True)
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    o.set_source(pkg.decks.five_spot_source(case, rate_sm3_per_day=100.0))
    j, r = o.assemble(86400.0, 0)
    return case["Nb"], case["rowptr"], case["col"], j, r


def well_clique_system(nx=10, ny=9, nz=8, seed=3):
    """a 7-point grid with two wells whose perforated cells are all coupled to each other (add_well_contributions patterns)"""
    Nb, rp, ci, _ = laplace_block_system(nx, ny, nz, seed=seed)
    rows = [set(ci[rp[i]:rp[i + 1]].tolist()) for i in range(Nb)]
    for c0 in (3 + nx * 4, 7 + nx * 2):
        well = [c0 + nx * ny * k for k in range(nz)]
        for a in well:
            rows[a].update(well)
    rp2, cl2 = [0], []
    for r in rows:
        cl2.extend(sorted(r))
        rp2.append(len(cl2))
    rp2, cl2 = np.array(rp2, np.int32), np.array(cl2, np.int32)
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (len(cl2), 3, 3)) * 0.2
    for i in range(Nb):
        ks = np.arange(rp2[i], rp2[i + 1])
        dk = ks[cl2[ks] == i][0]
        v[dk][np.arange(3), np.arange(3)] = 1.5 * (np.abs(v[ks]).sum(axis=(0, 2)) + 0.5)
    return Nb, rp2, cl2, np.ascontiguousarray(v.reshape(-1))


@pytest.mark.parametrize("reorder", ["level_scheduling", "distance2", "graph_coloring_greedy"])
def test_factors_and_apply_spe1(pkg, orc, reorder):
    Nb, rp, ci, j, _ = spe1_jacobian(pkg, orc)
    check_against_oracle(pkg, orc, Nb, rp, ci, j, reorder)


@pytest.mark.parametrize("reorder", ["level_scheduling", "distance2", "line_coloring", "auto"])
def test_factors_and_apply_assembled_20x20x10(pkg, orc, reorder):
    Nb, rp, ci, j, _ = cartesian_jacobian(pkg, orc, 20, 20, 10)
    check_against_oracle(pkg, orc, Nb, rp, ci, j, reorder)


def test_factors_and_apply_norne_shaped(pkg, orc):
    case, _, _ = norne_shaped_case(pkg)
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    j, _ = o.assemble(86400.0, 0)
    check_against_oracle(pkg, orc, case["Nb"], case["rowptr"], case["col"], j, "level_scheduling", modes=(("post_scale", 0.9),))
    check_against_oracle(pkg, orc, case["Nb"], case["rowptr"], case["col"], j, "distance2", modes=(("in_sweep", 0.9),))


@pytest.mark.parametrize("reorder", ["level_scheduling", "distance2"])
def test_factors_and_apply_well_cliques(pkg, orc, reorder):
    Nb, rp, ci, v = well_clique_system()
    check_against_oracle(pkg, orc, Nb, rp, ci, v, reorder)


@pytest.mark.parametrize("reorder", ["level_scheduling", "distance2"])
def test_ilu1_bicgstab_matches_the_oracle_on_the_padded_matrix(pkg, orc, reorder):
    Nb, rp, ci, j, r = cartesian_jacobian(pkg, orc, 20, 20, 10)
    prp, pcl, pv, fr, to, jf = check_against_oracle(pkg, orc, Nb, rp, ci, j, reorder, modes=(("post_scale", 0.9),))
    s = pkg.capi.HipSolver(reorder=reorder, ilu_fillin_level=1, tolerance=1e-10, maxit=400)
    res = s.solve_system(Nb, rp, ci, jf, r)
    x = s.get_result()
    xo, reso = orc.solve(Nb, prp, pcl, pv, np.ascontiguousarray(r.reshape(Nb, 3)[fr].reshape(-1)), tol=1e-10, maxit=400, w=0.9, reorder="none")
    xo = xo.reshape(Nb, 3)[to].reshape(-1)
    assert res.converged and reso.converged and res.it == reso.it, (res.it, reso.it)
    assert res.reduction < 1e-10
    np.testing.assert_allclose(x, xo, rtol=1e-6, atol=1e-8 * np.abs(xo).max())


def test_level_zero_through_the_new_call_is_todays_path(pkg, orc):
    Nb, rp, ci, j, r = cartesian_jacobian(pkg, orc, 20, 20, 10)
    out = []
    for call in (False, True):
        s = pkg.capi.HipSolver(reorder="level_scheduling")
        if call:
            s.set_ilu_fillin_level(0)
        res = s.solve_system(Nb, rp, ci, j, r)
        out.append((res.it, res.reduction, s.get_result(), s.ilu_info()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    assert out[1][3]["fill_level"] == 0 and out[0][3] == out[1][3]


def test_ilu1_needs_no_more_iterations_than_ilu0_on_configs2(pkg, orc):
    Nb, rp, ci, j, r = cartesian_jacobian(pkg, orc, 24, 25, 15)
    its = []
    for n in (0, 1):
        s = pkg.capi.HipSolver(reorder="level_scheduling", ilu_fillin_level=n)
        res = s.solve_system(Nb, rp, ci, j, r)
        assert res.converged
        its.append(res.it)
    assert its[1] <= its[0], its


def test_refusals(pkg):
    capi = pkg.capi
    s = capi.HipSolver()
    with pytest.raises(capi.OpmHipError) as e:
        s.set_ilu_fillin_level(-1)
    assert e.value.code == capi.INVALID_ARGUMENT
    Nb, rp, ci, _ = laplace_block_system(4, 3, 2)
    s.set_pattern(Nb, rp, ci)
    with pytest.raises(capi.OpmHipError) as e:
        s.set_ilu_fillin_level(1)
    assert e.value.code == capi.INVALID_ARGUMENT
    # a decomposed context (loopback communicator): refused whichever call comes first
    L = capi.lib()
    L.opmhip_comm_init_loopback.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p]
    d = capi.HipSolver()
    assert L.opmhip_comm_init_loopback(d._h, 1, 0, b"ilun-refusal-a") == capi.SUCCESS
    with pytest.raises(capi.OpmHipError) as e:
        d.set_ilu_fillin_level(1)
    assert e.value.code == capi.INVALID_ARGUMENT and "decomposed" in str(e.value)
    d2 = capi.HipSolver(ilu_fillin_level=1)
    assert L.opmhip_comm_init_loopback(d2._h, 1, 0, b"ilun-refusal-b") == capi.INVALID_ARGUMENT
    # the memory guard at set_pattern: ILU(2) of a 20^3 grid fills far beyond 8 x nnzb
    Nb, rp, ci, _ = laplace_block_system(20, 20, 20)
    g = capi.HipSolver(reorder="level_scheduling", ilu_fillin_level=2)
    with pytest.raises(capi.OpmHipError) as e:
        g.set_pattern(Nb, rp, ci)
    assert e.value.code == capi.INVALID_ARGUMENT and "ILU(2)" in str(e.value)
    # the CPR's fine smoother stays ILU0: the level is ignored
    c = capi.HipSolver(preconditioner="cpr", ilu_fillin_level=1)
    Nb, rp, ci, _ = laplace_block_system(4, 3, 2)
    c.set_pattern(Nb, rp, ci)
    assert c.ilu_info()["fill_level"] == 0


def test_full_size_distance2_ilu1(pkg, case100):
    case, src = case100["case"], case100["src"]
    m = pkg.capi.HipModel(case, reorder="distance2", ilu_fillin_level=1)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src)
    m.assemble(86400.0, 0)
    res = m.solve_jacobian_system()
    x = m.get_result()
    info = m.ilu_info()
    assert res.converged and np.all(np.isfinite(x)) and np.abs(x).max() > 0
    assert info["fill_level"] == 1 and 11 <= info["levels"] <= 16, info
    assert m.ordering_info()["ilu_ordering"] == "distance2"


def test_newton_loop_ilu1_reaches_the_ilu0_state(pkg):
    states = []
    for n in (0, 1):
        case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
        m = pkg.capi.HipModel(case, reorder="level_scheduling", ilu_fillin_level=n)
        m.set_state(case["pv"], case["meaning"])
        m.set_source(pkg.decks.five_spot_source(case, rate_sm3_per_day=100.0))
        model = pkg.newton.BlackoilModelHip(m)
        model.begin_time_step(86400.0)
        rep = model.step(86400.0)
        assert rep.converged
        states.append((m.get_state(), rep.total_linear_iterations, rep.total_newton_iterations))
    (p0, m0), (p1, m1) = states[0][0], states[1][0]
    assert np.array_equal(m0, m1)
    p0, p1 = p0.reshape(-1, 3), p1.reshape(-1, 3)
    np.testing.assert_allclose(p1[:, 1], p0[:, 1], rtol=1e-4)                 # pressure
    np.testing.assert_allclose(p1[:, [0, 2]], p0[:, [0, 2]], rtol=1e-3, atol=1e-4)

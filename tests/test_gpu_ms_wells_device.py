"""Multisegment wells in their device-resident form (opmhip_set_ms_wells): D inverted on the device with partial pivoting, the operator
y -= C^T (D^-1 (B x)) applied by one kernel after every product, no host callback.  The reference's D^-1 is UMFPack, which is not
available, so the yardstick is a float64 restatement in numpy (dense B, C, D; np.linalg.solve), as tests/test_gpu_host_cpp.py::_ms_well does.

The elementwise bound of the operator tests, from first-order error analysis of a pivoted solve (not tuned):
    |d| <= 2 (|C|^T 1) M eps cond_inf(D) |z2|_inf + 16 eps |C|^T |z2| + 2 eps (|p| + |w|)
(the solve's forward error on either side; the 3- and 4-term sums of B x and C^T z2; the two roundings of y -= ... and p - w)."""
import os
import subprocess
import uuid

import numpy as np
import pytest

from cpr_dense import solve_dense
from helpers import laplace_block_system

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "opm-autodiff_amd", "host")
EPS = np.finfo(np.float64).eps


def _exe(name):
    p = os.path.join(HOST, name)
    if not os.path.exists(p):
        subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    return p


def _well_term_and_bound(pkg, wells, Nb, x, z2_error=None):
    """sum over the wells of C^T D^-1 B x in float64, and the elementwise bound of the module's docstring without its last term.
    z2_error: per well an absolute error admitted in z2 in place of the term in cond(D)."""
    term, bound = np.zeros(3 * Nb), np.zeros(3 * Nb)
    for n, w in enumerate(wells):
        B, C, D = pkg.mswells.dense_operators(w, Nb)
        z2 = np.linalg.solve(D, B @ x)
        term += C.T @ z2
        ez = 2 * len(D) * EPS * np.linalg.cond(D, np.inf) * np.abs(z2).max() if z2_error is None else z2_error[n]
        bound += np.abs(C).T @ np.ones(len(D)) * ez + 16 * EPS * (np.abs(C).T @ np.abs(z2))
    return term, bound


def _operator_difference(pkg, s, wells, x):
    """(p - w, p, w): the product without the device list minus the product with it - both carry the same bits of A x"""
    s.set_ms_wells(wells)
    w = s.spmv(x)
    assert s.ms_wells_info()["wells"] == len(wells)
    s.set_ms_wells(None)
    p = s.spmv(x)
    return p - w, p, w


def _grid_solver(pkg, reorder, seed=3, **kw):
    Nb, rp, ci, v = laplace_block_system(12, 10, 6, seed=seed)
    s = pkg.capi.HipSolver(reorder=reorder, **kw)
    s.set_pattern(Nb, rp, ci)
    s.upload_system(v)
    return s, Nb, rp, ci, v


def _check_operator(pkg, s, wells, Nb, x, z2_error=None):
    d, p, w = _operator_difference(pkg, s, wells, x)
    term, bound = _well_term_and_bound(pkg, wells, Nb, x, z2_error)
    bound = bound + 2 * EPS * (np.abs(p) + np.abs(w))
    err = np.abs(d - term)
    print("largest |error| / bound: %.3g; largest well term %.3g" % (np.max(err / np.maximum(bound, 1e-300)), np.abs(term).max()))
    assert np.abs(term).max() > 1e-3 and np.all(np.isfinite(w))
    assert np.all(err <= bound), (np.max(err / np.maximum(bound, 1e-300)), int(np.argmax(err / np.maximum(bound, 1e-300))))


@pytest.mark.parametrize("reorder", ["level_scheduling", "graph_coloring", "line_coloring"])
def test_operator_against_numpy(pkg, reorder):
    """wells of Mb = 1, 2, 7, 33 and the largest the cap admits in one list, no cell shared (plain stores), in three orderings (the cells
    are translated to the internal order at upload)"""
    s, Nb, _, _, _ = _grid_solver(pkg, reorder)
    capM, _ = pkg.capi.ms_wells_caps()
    sizes = [1, 2, 7, 33, capM // 4]
    rng = np.random.default_rng(21)
    cells = rng.permutation(Nb)
    wells, at = [], 0
    for n, Mb in enumerate(sizes):
        nblk = Mb + 2
        wells.append(pkg.mswells.tree_well(Mb, cells[at:at + nblk], seed=100 + n))
        at += nblk
    x = rng.standard_normal(3 * Nb)
    _check_operator(pkg, s, wells, Nb, x)
    info_before = s.ms_wells_info()
    assert info_before["wells"] == 0            # cleared by the helper
    s.set_ms_wells(wells)
    info = s.ms_wells_info()
    assert info["wells"] == len(sizes) and info["max_m"] == capM and info["kib"] >= 8 * capM * capM // 1024


def _matr33(pkg, golden):
    Nb, rp, ci, v, _ = pkg.mmio.read_block_matrix(os.path.join(golden, "linalg", "matr33.txt"))
    b = pkg.mmio.read_block_vector(os.path.join(golden, "linalg", "rhs3.txt"))
    A = np.zeros((3 * Nb, 3 * Nb))
    for i in range(Nb):
        for k in range(rp[i], rp[i + 1]):
            A[3 * i:3 * i + 3, 3 * ci[k]:3 * ci[k] + 3] = v[9 * k:9 * k + 9].reshape(3, 3)
    return Nb, rp, ci, v, b, A


def _driver_ms_well(pkg, Nb):
    """the multisegment well of host/test_hipSolver.cpp (mswells / msonly) as the per-well dict: two segments, three perforations"""
    Bv = np.array([0.03 * (1 + (i * 5) % 7) - 0.05 for i in range(36)])
    Cv = np.array([0.02 * (1 + (i * 3) % 5) for i in range(36)])
    D = np.array([[2.0 + 0.1 * r if r == c else 0.05 * ((r * 3 + c * 5) % 4) - 0.04 for c in range(8)] for r in range(8)])
    cp, ri, dv = pkg.mswells.csc(D)
    return dict(Brows=[0, 1, 3], Bcols=[0, 2, Nb - 1], Bvals=Bv, Cvals=Cv, Dcolptr=cp, Drows=ri, Dvals=dv)


def _driver_std_well(Nb):
    Cs = np.array([0.01 * (1 + (i * 7) % 5) for i in range(24)])
    Bs = np.array([0.02 * (1 + (i * 3) % 7) for i in range(24)])
    Ds = np.array([0.5 if i % 5 == 0 else 0.01 * (i % 3) for i in range(16)])
    Bd, Cd = np.zeros((4, 3 * Nb)), np.zeros((4, 3 * Nb))
    for blk, col in enumerate([1, Nb - 2]):
        Bd[:, 3 * col:3 * col + 3] += Bs[12 * blk:12 * blk + 12].reshape(4, 3)
        Cd[:, 3 * col:3 * col + 3] += Cs[12 * blk:12 * blk + 12].reshape(4, 3)
    return dict(numWells=1, val_pointers=[0, 2], Ccols=[1, Nb - 2], Bcols=[1, Nb - 2], Cnnzs=Cs, Dnnzs=Ds, Bnnzs=Bs), Cd.T @ (Ds.reshape(4, 4) @ Bd)


@pytest.mark.parametrize("std_well", [False, True])
def test_solve_with_the_device_list_in_place_of_the_callback(pkg, golden, std_well):
    """the system and well of test_hipSolverBackend_with_a_multisegment_well: converged, |A_eff x - b| <= tol |b| (1 + 1e-6) at tol = 1e-10
    with A_eff formed densely, for ILU0 in two orderings, ILU(1) and cpr_quasiimpes, with and without the standard well beside it; and the
    same x as the callback form gives (two differently rounded well operators)"""
    Nb, rp, ci, v, b, A = _matr33(pkg, golden)
    msw = _driver_ms_well(pkg, Nb)
    B, Cm, D = pkg.mswells.dense_operators(msw, Nb)
    Aeff = A - Cm.T @ np.linalg.solve(D, B)
    wells = None
    if std_well:
        wells, S = _driver_std_well(Nb)
        Aeff = Aeff - S
    for kw in (dict(reorder="level_scheduling"), dict(reorder="graph_coloring"), dict(reorder="level_scheduling", ilu_fillin_level=1),
               dict(reorder="level_scheduling", preconditioner="cpr_quasiimpes")):
        s = pkg.capi.HipSolver(tolerance=1e-10, maxit=50, ilu_relaxation=1.0, **kw)
        s.set_pattern(Nb, rp, ci)
        s.set_ms_wells([msw])
        res = s.solve_system(Nb, rp, ci, v.copy(), b, wells=wells)
        x = s.get_result()
        assert res.converged and s.ms_wells_info()["wells"] == 1
        assert np.linalg.norm(Aeff @ x - b) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)
        # the callback form of the same context's configuration
        cb = dict(wells or dict(numWells=0))
        cb.update(numMsWells=1, N=3 * Nb, ms_apply=lambda hx, hy: hy.__isub__(Cm.T @ np.linalg.solve(D, B @ hx)))
        s2 = pkg.capi.HipSolver(tolerance=1e-10, maxit=50, ilu_relaxation=1.0, **kw)
        res2 = s2.solve_system(Nb, rp, ci, v.copy(), b, wells=cb)
        assert res2.converged
        np.testing.assert_allclose(x, s2.get_result(), rtol=1e-5, atol=1e-7 * np.abs(x).max())


def test_solve_in_the_half_product_form_with_fused_reductions(pkg, orc):
    """half_product > 0 on a grid large enough for the pipelined kernels, without and with fused_reductions = 1: the forms engage
    (opmhip_get_product_form) and the solution solves (A - sum C^T D^-1 B) x = b.  The plain recurrence is held to the solve test's own
    assertion at tol = 1e-10.  fused_reductions stops on a recurred norm and is refused by opmhip_create below tol = 1e-6; there the
    criterion is the one tests/test_gpu_fused_reductions.py holds it to: the reported reduction is the iterate's own residual (1e-6
    relative) and that residual is below 2 tol."""
    Nb, rp, ci, v = laplace_block_system(28, 35, 14, seed=12)
    rng = np.random.default_rng(5)
    cells = rng.permutation(Nb)
    wells = [pkg.mswells.tree_well(7, cells[:9], seed=31), pkg.mswells.tree_well(30, cells[9:49], seed=32)]
    for w in wells:
        w["Bvals"] = 0.05 * w["Bvals"]
    b = rng.standard_normal(3 * Nb)
    for tol, fused in ((1e-10, 0), (1e-6, 1)):
        kw = dict(tolerance=tol, maxit=200, reorder="line_coloring", chain_length=8, spmv_pipe_wgs=24, half_product=1, fused_reductions=fused)
        s = pkg.capi.HipSolver(**kw)
        s.set_pattern(Nb, rp, ci)
        assert s.product_form()["half_product"]
        s.set_ms_wells(wells)
        res = s.solve_system(Nb, None, None, v.copy(), b)
        x = s.get_result()
        assert res.converged and s.product_form()["half_product"] and s.ms_wells_info()["wells"] == 2
        term, _ = _well_term_and_bound(pkg, wells, Nb, x)
        true = np.linalg.norm(orc.spmv(Nb, rp, ci, v, x) - term - b) / np.linalg.norm(b)
        print("tol %g fused %d: iterations %.1f, true reduction %.3e, reported %.3e" % (tol, fused, res.it, true, res.reduction))
        if fused:
            assert abs(res.reduction - true) <= 1e-6 * true and true < 2.0 * tol
        else:
            assert true <= tol * (1 + 1e-6)
        # the wells do something
        s0 = pkg.capi.HipSolver(**kw)
        s0.solve_system(Nb, rp, ci, v.copy(), b)
        assert np.abs(x - s0.get_result()).max() > 1e-6 * np.abs(x).max()


def test_no_host_in_the_loop(pkg):
    """a device list and a callback-free opmhip_wells: the solve succeeds; identical arrays are not factored again, changed Dvals are,
    once, and give the new operator; clearing the list gives the plain operator's bits back"""
    s, Nb, rp, ci, v = _grid_solver(pkg, "line_coloring", tolerance=1e-8)
    rng = np.random.default_rng(9)
    cells = rng.permutation(Nb)
    wells = [pkg.mswells.tree_well(5, cells[:7], seed=41), pkg.mswells.tree_well(12, cells[7:21], seed=42)]
    for w in wells:
        w["Bvals"] = 0.05 * w["Bvals"]
    b = rng.standard_normal(3 * Nb)
    s.set_ms_wells(wells)
    res = s.solve_system(Nb, None, None, v.copy(), b, wells=dict(numWells=0))
    assert res.converged
    x1 = s.get_result()
    info = s.ms_wells_info()
    assert info["wells"] == 2 and info["max_m"] == 48 and info["factorisations"] == 1
    s.set_ms_wells([dict(w) for w in wells])                       # Flow rebuilds its wells for every solve: the same values in new arrays
    res = s.solve_system(Nb, None, None, v.copy(), b)
    assert res.converged and np.array_equal(s.get_result(), x1) and s.ms_wells_info()["factorisations"] == 1
    changed = [dict(w) for w in wells]
    changed[1]["Dvals"] = changed[1]["Dvals"] * 1.25
    s.set_ms_wells(changed)
    assert s.ms_wells_info()["factorisations"] == 2
    x = rng.standard_normal(3 * Nb)
    _check_operator(pkg, s, changed, Nb, x)                        # the new operator (the helper sets the list again: same values, no inversion)
    assert s.ms_wells_info()["factorisations"] == 2
    s.set_ms_wells(None)
    plain, _, _, _, _ = _grid_solver(pkg, "line_coloring", tolerance=1e-8)
    assert np.array_equal(s.spmv(x), plain.spmv(x))
    assert s.ms_wells_info()["wells"] == 0


def test_pivoting_across_the_blocks(pkg):
    """a D whose leading 4 x 4 block is singular while D is not (two block rows exchanged): within the bound of the operator test - an
    elimination that exchanges rows only inside a block fails here"""
    s, Nb, _, _, _ = _grid_solver(pkg, "graph_coloring")
    rng = np.random.default_rng(13)
    cells = rng.permutation(Nb)
    for Mb, seed in ((3, 51), (20, 52)):
        w = pkg.mswells.tree_well(Mb, cells[:Mb + 2], seed=seed)
        _, _, D = pkg.mswells.dense_operators(w, Nb)
        other = [i for i in range(1, Mb) if not D[4 * i:4 * i + 4, 0:4].any()][0]
        P = np.arange(4 * Mb)
        P[0:4], P[4 * other:4 * other + 4] = np.arange(4 * other, 4 * other + 4), np.arange(0, 4)
        D = D[P]
        assert np.linalg.matrix_rank(D[:4, :4]) < 4 and np.linalg.matrix_rank(D) == 4 * Mb
        w["Dcolptr"], w["Drows"], w["Dvals"] = pkg.mswells.csc(D)
        _check_operator(pkg, s, [w], Nb, rng.standard_normal(3 * Nb))


@pytest.mark.parametrize("Mb", [2, 7, 33, 64])
def test_badly_scaled_rows(pkg, Mb):
    """rows of D scaled by 10^U(-4, 4), the rows of B with them (z2 is unchanged in exact arithmetic).  No bound in cond(D) is useful here,
    so the yardstick is numpy itself: e_ref = the larger error of np.linalg.solve and inv(D) @ z1 against an elimination in np.longdouble
    for the same matrix; 16 e_ref is admitted in z2 (another pivot order, another summation order in D^-1 z1), propagated to y through
    |C|^T 1.  The accuracy for badly scaled D is that of an explicit inverse (include/opmhip.h)."""
    s, Nb, _, _, _ = _grid_solver(pkg, "level_scheduling")
    rng = np.random.default_rng(60 + Mb)
    cells = rng.permutation(Nb)
    w = pkg.mswells.tree_well(Mb, cells[:Mb + 2], seed=70 + Mb)
    B, C, D = pkg.mswells.dense_operators(w, Nb)
    sc = 10.0 ** rng.uniform(-4, 4, 4 * Mb)
    D = sc[:, None] * D
    w["Dcolptr"], w["Drows"], w["Dvals"] = pkg.mswells.csc(D)
    Bv = w["Bvals"].reshape(-1, 4, 3).copy()
    brow = np.repeat(np.arange(Mb), np.diff(w["Brows"]))
    for blk in range(len(Bv)):
        Bv[blk] *= sc[4 * brow[blk]:4 * brow[blk] + 4, None]
    w["Bvals"] = Bv.reshape(-1)
    x = rng.standard_normal(3 * Nb)
    B, C, D = pkg.mswells.dense_operators(w, Nb)
    z1 = B @ x
    z_ld = solve_dense(D, z1, np.longdouble)   # Gaussian elimination with partial pivoting in np.longdouble
    e_ref = float(max(np.abs(np.linalg.solve(D, z1) - z_ld).max(), np.abs(np.linalg.inv(D) @ z1 - z_ld).max()))
    d, p, wv = _operator_difference(pkg, s, [w], x)
    z2 = np.asarray(z_ld, dtype=np.float64)
    term = C.T @ z2
    bound = np.abs(C).T @ np.ones(4 * Mb) * 16 * e_ref + 16 * EPS * (np.abs(C).T @ np.abs(z2)) + 2 * EPS * (np.abs(p) + np.abs(wv))
    err = np.abs(d - term)
    # the error in z2 the device's result implies where C^T carries it alone, against numpy's own: the measured ratio
    print("Mb %d: e_ref %.3g, largest |error| / bound %.3g, |error| / (|C|^T 1 e_ref) up to %.3g" %
          (Mb, e_ref, np.max(err / bound), np.max(err / np.maximum(np.abs(C).T @ np.ones(4 * Mb) * e_ref, 1e-300))))
    assert np.all(err <= bound), np.max(err / bound)


def test_refusals(pkg, golden):
    """a singular D, a cell out of range, a well over the cap, a decomposed context, callback and device list together: each refused with
    its status and a text that names the cause; the context solves a plain system correctly afterwards"""
    s, Nb, rp, ci, v = _grid_solver(pkg, "line_coloring", tolerance=1e-8)
    rng = np.random.default_rng(17)
    cells = rng.permutation(Nb)
    good = pkg.mswells.tree_well(4, cells[:6], seed=81)
    fresh = pkg.capi.HipSolver()
    with pytest.raises(pkg.capi.OpmHipError) as e:
        fresh.set_ms_wells([good])
    assert e.value.code == pkg.capi.NOT_READY and "pattern" in str(e.value)
    # singular: an empty row of D - flagged on the device, reported at the latest by the operator application that follows
    _, _, D = pkg.mswells.dense_operators(good, Nb)
    D[5, :] = 0.0
    sing = dict(good)
    sing["Dcolptr"], sing["Drows"], sing["Dvals"] = pkg.mswells.csc(D)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([good, sing])
        s.solve_system(Nb, None, None, v.copy(), rng.standard_normal(3 * Nb))
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "singular" in str(e.value) and "well 1" in str(e.value)
    assert s.ms_wells_info()["wells"] == 0
    bad = dict(good)
    bad["Bcols"] = np.array(good["Bcols"])
    bad["Bcols"][2] = Nb
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([bad])
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "out of range" in str(e.value)
    capM, _ = pkg.capi.ms_wells_caps()
    big = pkg.mswells.tree_well(capM // 4 + 1, cells[:8], seed=82)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([good, big])
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "cap" in str(e.value) and s.ms_wells_info()["wells"] == 0
    ragged = dict(good)
    ragged["Dcolptr"] = np.array(good["Dcolptr"])
    ragged["Dcolptr"][3] = ragged["Dcolptr"][4] + 1            # not ascending: the struct builder lets lengths through, the library looks inside
    with pytest.raises((pkg.capi.OpmHipError, ValueError)):
        s.set_ms_wells([ragged])
    # callback and device list together
    s.set_ms_wells([good])
    b = rng.standard_normal(3 * Nb)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.solve_system(Nb, None, None, v.copy(), b, wells=dict(numWells=0, numMsWells=1, N=3 * Nb, ms_apply=lambda hx, hy: None))
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "twice" in str(e.value)
    # ... and the context is whole: a plain solve gives the bits of a context that never had wells
    s.set_ms_wells(None)
    res = s.solve_system(Nb, None, None, v.copy(), b)
    plain, _, _, _, _ = _grid_solver(pkg, "line_coloring", tolerance=1e-8)
    res0 = plain.solve_system(Nb, None, None, v.copy(), b)
    assert res.converged and res.it == res0.it and np.array_equal(s.get_result(), plain.get_result())
    # a decomposed context (loopback, two ranks): out of scope, refused like the callback form
    case = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    m = pkg.capi.HipModel(case, comm=("loopback", 2, 0, "msw" + uuid.uuid4().hex), reorder="level_scheduling")
    with pytest.raises(pkg.capi.OpmHipError) as e:
        m.set_ms_wells([pkg.mswells.tree_well(2, [0, 1, 2], seed=83)])
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "decomposed" in str(e.value)


def test_two_wells_on_one_cell_take_the_atomic_path(pkg):
    s, Nb, _, _, _ = _grid_solver(pkg, "graph_coloring")
    rng = np.random.default_rng(23)
    cells = rng.permutation(Nb)
    shared = cells[:3]
    wells = [pkg.mswells.tree_well(6, np.concatenate([shared, cells[3:8]]), seed=91),
             pkg.mswells.tree_well(9, np.concatenate([cells[8:16], shared[::-1]]), seed=92)]
    _check_operator(pkg, s, wells, Nb, rng.standard_normal(3 * Nb))


@pytest.mark.parametrize("mode", ["mswells_dev", "msonly_dev"])
def test_plugin_with_the_wells_on_the_device(pkg, golden, mode):
    """host/test_hipSolver mswells_dev / msonly_dev (bda::hipSolverBackend<3> with ms_wells_on_device) in both include modes: the same
    output in both builds, and the solution solves A_eff x = b"""
    args = [os.path.join(golden, "linalg", "matr33.txt"), os.path.join(golden, "linalg", "rhs3.txt"), "1e-10", "50", "level_scheduling", mode]
    outs = []
    for exe in ("test_hipSolver", "test_hipSolver_opmhdr"):
        out = subprocess.run([_exe(exe)] + args, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        outs.append(out.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("converged 1")
    x = np.array([float(t) for t in outs[0].strip().splitlines()[1:]])
    Nb, rp, ci, v, b, A = _matr33(pkg, golden)
    B, Cm, D = pkg.mswells.dense_operators(_driver_ms_well(pkg, Nb), Nb)
    Aeff = A - Cm.T @ np.linalg.solve(D, B)
    if mode == "mswells_dev":
        Aeff = Aeff - _driver_std_well(Nb)[1]
    assert np.linalg.norm(Aeff @ x - b) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)
    # the device form and the callback form of the same driver: two differently rounded well operators
    cb = subprocess.run([_exe("test_hipSolver")] + args[:-1] + [mode[:-4]], capture_output=True, text=True)
    xc = np.array([float(t) for t in cb.stdout.strip().splitlines()[1:]])
    np.testing.assert_allclose(x, xc, rtol=1e-5, atol=1e-7 * np.abs(x).max())

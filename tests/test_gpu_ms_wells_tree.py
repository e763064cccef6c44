"""The tree form of the device-resident multisegment wells (opmhip_set_ms_wells_form, OPMHIP_MS_WELLS_TREE / _AUTO): D eliminated block by
block over the segment tree, leaves first, 48 doubles per segment, wells of up to ms_wells_tree_cap() segments.  The yardsticks are those of
tests/test_gpu_ms_wells_device.py, on its 12 x 10 x 6 Laplace grid: for unscaled D the elementwise bound
    |d| <= 2 (|C|^T 1) M eps cond_inf(D) |z2|_inf + 16 eps |C|^T |z2| + 2 eps (|p| + |w|)
against np.linalg.solve, and for badly scaled rows 16 e_ref admitted in z2, e_ref being numpy's own error against an elimination in
np.longdouble.  tests/test_ms_wells_tree_numpy.py holds the same elimination, stated in numpy, to 16 e_ref on the CPU."""
import uuid

import numpy as np
import pytest

import ms_tree_shapes as shapes
from cpr_dense import solve_dense
from helpers import laplace_block_system

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _grid_solver(pkg, reorder, seed=3, **kw):
    Nb, rp, ci, v = laplace_block_system(12, 10, 6, seed=seed)
    s = pkg.capi.HipSolver(reorder=reorder, **kw)
    s.set_pattern(Nb, rp, ci)
    s.upload_system(v)
    return s, Nb, rp, ci, v


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


def _operator_difference(pkg, s, wells, x, form):
    """(p - w, p, w): the product without the device list minus the product with it - both carry the same bits of A x"""
    s.set_ms_wells(wells, form=form)
    w = s.spmv(x)
    assert s.ms_wells_info()["wells"] == len(wells)
    s.set_ms_wells(None)
    p = s.spmv(x)
    return p - w, p, w


def _check_operator(pkg, s, wells, Nb, x, form="tree", term_and_bound=None):
    d, p, w = _operator_difference(pkg, s, wells, x, form)
    term, bound = term_and_bound or _well_term_and_bound(pkg, wells, Nb, x)
    bound = bound + 2 * EPS * (np.abs(p) + np.abs(w))
    err = np.abs(d - term)
    print("largest |error| / bound: %.3g; largest well term %.3g" % (np.max(err / np.maximum(bound, 1e-300)), np.abs(term).max()))
    assert np.abs(term).max() > 1e-3 and np.all(np.isfinite(w))
    assert np.all(err <= bound), (np.max(err / np.maximum(bound, 1e-300)), int(np.argmax(err / np.maximum(bound, 1e-300))))
    return d, bound


# the operator test's list: shape, cells (720 in the grid, none shared)
OPERATOR_LIST = (("chain1", 3), ("chain2", 4), ("chain5", 7), ("chain65", 67), ("chain130", 100), ("star71", 73), ("comb120", 100), ("random150", 110),
                 ("random300", 200))
_reference = {}


def _operator_list(pkg, Nb):
    """the wells, x and the float64 reference with its bound: computed once, shared by the orderings, left unchanged"""
    if "list" not in _reference:
        rng = np.random.default_rng(21)
        cells = rng.permutation(Nb)
        wells, at = [], 0
        for n, (name, ncell) in enumerate(OPERATOR_LIST):
            wells.append(shapes.well(pkg, shapes.SHAPES[name], cells[at:at + ncell], seed=200 + n))
            at += ncell
        assert at <= Nb
        x = rng.standard_normal(3 * Nb)
        _reference["list"] = (wells, x, _well_term_and_bound(pkg, wells, Nb, x))
    return _reference["list"]


@pytest.mark.parametrize("reorder", ["level_scheduling", "line_coloring"])
def test_operator_against_numpy(pkg, reorder):
    """chains of 1, 2, 5, 65 (one above the dense cap, deeper than a wavefront) and 130 segments, a star of 71 (one parent, 70 children: the
    ordered gather, a level wider than a wavefront), a comb of 120, random trees of 150 and 300 (M = 1200: more equations than threads) in
    one list, no cell shared, in two orderings; every well within the bound in cond_inf(D)"""
    s, Nb, _, _, _ = _grid_solver(pkg, reorder)
    wells, x, ref = _operator_list(pkg, Nb)
    _check_operator(pkg, s, wells, Nb, x, term_and_bound=ref)
    s.set_ms_wells(wells, form="tree")
    info, finfo = s.ms_wells_info(), s.ms_wells_form_info()
    assert info["wells"] == len(wells) and info["max_m"] == 1200
    assert finfo == dict(form="tree", dense=0, tree=len(wells), tree_max_segments=300, tree_max_depth=130, tree_kib=-(-48 * 8 * sum(len(shapes.SHAPES[n]) for n, _ in OPERATOR_LIST) // 1024))


def test_tree_cap(pkg):
    """a chain of ms_wells_tree_cap() segments is taken and lies within the bound; one segment more is refused and no list stays set"""
    s, Nb, _, _, _ = _grid_solver(pkg, "level_scheduling")
    cap = pkg.capi.ms_wells_tree_cap()
    rng = np.random.default_rng(31)
    cells = rng.permutation(Nb)
    w = shapes.well(pkg, shapes.chain(cap), cells[:48], seed=301)
    _check_operator(pkg, s, [w], Nb, rng.standard_normal(3 * Nb))
    s.set_ms_wells([w], form="tree")
    assert s.ms_wells_form_info()["tree_max_depth"] == cap and s.ms_wells_info()["wells"] == 1
    big = shapes.well(pkg, shapes.chain(cap + 1), cells[:48], seed=302)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([big], form="tree")
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "cap" in str(e.value) and s.ms_wells_info()["wells"] == 0
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([big], form="auto")
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "cap" in str(e.value) and s.ms_wells_info()["wells"] == 0


def test_a_wide_well_too_large_for_the_lds(pkg):
    """a star of 400 segments beside a chain of 3: levels wider than a wavefront (the whole workgroup walks them, a barrier per level) and
    more blocks than the LDS holds (they are read from global memory), while the small well of the same launch stages its own"""
    s, Nb, _, _, _ = _grid_solver(pkg, "line_coloring")
    rng = np.random.default_rng(33)
    cells = rng.permutation(Nb)
    wells = [shapes.well(pkg, shapes.star(400), cells[:300], seed=331), shapes.well(pkg, shapes.chain(3), cells[300:305], seed=332)]
    _check_operator(pkg, s, wells, Nb, rng.standard_normal(3 * Nb))
    s.set_ms_wells(wells, form="tree")
    fi = s.ms_wells_form_info()
    assert (fi["tree"], fi["tree_max_segments"], fi["tree_max_depth"]) == (2, 400, 3)


def test_same_list_dense_and_tree(pkg):
    """wells of 7, 33 and 64 segments in both forms: each within its bound, so the two products differ by no more than the sum of the bounds"""
    s, Nb, _, _, _ = _grid_solver(pkg, "graph_coloring")
    rng = np.random.default_rng(41)
    cells = rng.permutation(Nb)
    wells = [pkg.mswells.tree_well(7, cells[:9], seed=401), pkg.mswells.tree_well(33, cells[9:44], seed=402), pkg.mswells.tree_well(64, cells[44:110], seed=403)]
    x = rng.standard_normal(3 * Nb)
    ref = _well_term_and_bound(pkg, wells, Nb, x)
    dd, bd = _check_operator(pkg, s, wells, Nb, x, form="dense", term_and_bound=ref)
    s.set_ms_wells(wells, form="dense")
    assert s.ms_wells_form_info() == dict(form="dense", dense=3, tree=0, tree_max_segments=0, tree_max_depth=0, tree_kib=0)
    dt, bt = _check_operator(pkg, s, wells, Nb, x, form="tree", term_and_bound=ref)
    s.set_ms_wells(wells, form="tree")
    fi = s.ms_wells_form_info()
    assert (fi["form"], fi["dense"], fi["tree"], fi["tree_max_segments"], fi["tree_kib"]) == ("tree", 0, 3, 64, -(-48 * 8 * 104 // 1024))
    assert np.all(np.abs(dd - dt) <= bd + bt)
    assert np.abs(dd - dt).max() > 0.0          # (two eliminations, two roundings)


def test_auto_chooses_per_well(pkg):
    s, Nb, _, _, _ = _grid_solver(pkg, "line_coloring")
    rng = np.random.default_rng(43)
    cells = rng.permutation(Nb)
    wells = [pkg.mswells.tree_well(30, cells[:32], seed=411), pkg.mswells.tree_well(64, cells[32:98], seed=412), pkg.mswells.tree_well(100, cells[98:200], seed=413)]
    _check_operator(pkg, s, wells, Nb, rng.standard_normal(3 * Nb), form="auto")
    s.set_ms_wells(wells, form="auto")
    fi = s.ms_wells_form_info()
    assert (fi["form"], fi["dense"], fi["tree"], fi["tree_max_segments"]) == ("auto", 2, 1, 100) and s.ms_wells_info()["wells"] == 3
    capM, _ = pkg.capi.ms_wells_caps()
    assert s.ms_wells_info()["kib"] >= 8 * (120 * 120 + capM * capM) // 1024
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([wells[2]], form="dense")
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "cap" in str(e.value) and s.ms_wells_info()["wells"] == 0
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([wells[2]])                   # the default form is the dense one, as before
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "OPMHIP_MS_WELLS_MAX_M" in str(e.value)


@pytest.mark.parametrize("name", ["chain65", "star71"])
def test_badly_scaled_rows(pkg, name):
    """the construction of tests/test_gpu_ms_wells_device.py::test_badly_scaled_rows in the tree form: rows of D scaled by 10^U(-4, 4), the
    rows of B with them; 16 e_ref admitted in z2, e_ref numpy's own error (solve and inv) against an elimination in np.longdouble"""
    s, Nb, _, _, _ = _grid_solver(pkg, "level_scheduling")
    par = shapes.SHAPES[name]
    Mb = len(par)
    rng = np.random.default_rng(60 + Mb)
    cells = rng.permutation(Nb)
    w = shapes.scale_rows(pkg, shapes.well(pkg, par, cells[:Mb + 2], seed=70 + Mb), rng)
    x = rng.standard_normal(3 * Nb)
    B, C, D = pkg.mswells.dense_operators(w, Nb)
    z1 = B @ x
    z_ld = solve_dense(D, z1, np.longdouble)
    e_ref = float(max(np.abs(np.linalg.solve(D, z1) - z_ld).max(), np.abs(np.linalg.inv(D) @ z1 - z_ld).max()))
    d, p, wv = _operator_difference(pkg, s, [w], x, "tree")
    z2 = np.asarray(z_ld, dtype=np.float64)
    term = C.T @ z2
    bound = np.abs(C).T @ np.ones(4 * Mb) * 16 * e_ref + 16 * EPS * (np.abs(C).T @ np.abs(z2)) + 2 * EPS * (np.abs(p) + np.abs(wv))
    err = np.abs(d - term)
    print("%s: e_ref %.3g, largest |error| / bound %.3g, |error| / (|C|^T 1 e_ref) up to %.3g" %
          (name, e_ref, np.max(err / bound), np.max(err / np.maximum(np.abs(C).T @ np.ones(4 * Mb) * e_ref, 1e-300))))
    assert np.all(err <= bound), np.max(err / bound)


def test_two_tree_wells_on_shared_cells_take_the_atomic_path(pkg):
    s, Nb, _, _, _ = _grid_solver(pkg, "graph_coloring")
    rng = np.random.default_rng(23)
    cells = rng.permutation(Nb)
    shared = cells[:3]
    wells = [pkg.mswells.tree_well(70, np.concatenate([shared, cells[3:72]]), seed=91),
             pkg.mswells.tree_well(9, np.concatenate([cells[72:80], shared[::-1]]), seed=92)]
    _check_operator(pkg, s, wells, Nb, rng.standard_normal(3 * Nb))


def test_refactorisation(pkg):
    """identical arrays are not factored again and give the same bits, changed Dvals are, once, and give the new operator; clearing the
    list gives the plain operator's bits back"""
    s, Nb, _, _, _ = _grid_solver(pkg, "line_coloring")
    rng = np.random.default_rng(9)
    cells = rng.permutation(Nb)
    wells = [shapes.well(pkg, shapes.SHAPES["chain65"], cells[:67], seed=41), pkg.mswells.tree_well(12, cells[67:81], seed=42)]
    x = rng.standard_normal(3 * Nb)
    s.set_ms_wells(wells, form="tree")
    y1 = s.spmv(x)
    f0 = s.ms_wells_info()["factorisations"]
    s.set_ms_wells([dict(w) for w in wells], form="tree")          # the same values in new arrays
    assert np.array_equal(s.spmv(x), y1) and s.ms_wells_info()["factorisations"] == f0
    changed = [dict(w) for w in wells]
    changed[0]["Dvals"] = changed[0]["Dvals"] * 1.25
    s.set_ms_wells(changed, form="tree")
    assert s.ms_wells_info()["factorisations"] == f0 + 1
    assert not np.array_equal(s.spmv(x), y1)
    _check_operator(pkg, s, changed, Nb, x)                        # the new operator (the helper clears the list and sets it again: one more)
    s.set_ms_wells(None)
    plain, _, _, _, _ = _grid_solver(pkg, "line_coloring")
    assert np.array_equal(s.spmv(x), plain.spmv(x))
    assert s.ms_wells_info()["wells"] == 0 and s.ms_wells_form_info()["tree"] == 0


def test_solve(pkg):
    """a random tree of 100 segments, B scaled by 0.05 as the dense form's solve tests do: ILU0 (line colouring) and cpr_quasiimpes converge
    at tol = 1e-10, and |A_eff x - b| <= tol |b| (1 + 1e-6) with A_eff formed densely"""
    Nb, rp, ci, v = laplace_block_system(12, 10, 6, seed=3)
    rng = np.random.default_rng(5)
    cells = rng.permutation(Nb)
    w = shapes.well(pkg, shapes.random_tree(100, 11), cells[:102], seed=51)
    w["Bvals"] = 0.05 * w["Bvals"]
    A = np.zeros((3 * Nb, 3 * Nb))
    for i in range(Nb):
        for k in range(rp[i], rp[i + 1]):
            A[3 * i:3 * i + 3, 3 * ci[k]:3 * ci[k] + 3] = v[9 * k:9 * k + 9].reshape(3, 3)
    B, C, D = pkg.mswells.dense_operators(w, Nb)
    Aeff = A - C.T @ np.linalg.solve(D, B)
    b = rng.standard_normal(3 * Nb)
    for kw in (dict(reorder="line_coloring"), dict(reorder="level_scheduling", preconditioner="cpr_quasiimpes")):
        s = pkg.capi.HipSolver(tolerance=1e-10, maxit=200, **kw)
        s.set_pattern(Nb, rp, ci)
        s.set_ms_wells([w], form="tree")
        res = s.solve_system(Nb, rp, ci, v.copy(), b)
        x = s.get_result()
        print("%s: %.1f iterations, reduction %.3e" % (kw, res.it, res.reduction))
        assert res.converged and s.ms_wells_form_info()["tree"] == 1
        assert np.linalg.norm(Aeff @ x - b) <= 1e-10 * np.linalg.norm(b) * (1 + 1e-6)
        s0 = pkg.capi.HipSolver(tolerance=1e-10, maxit=200, **kw)       # the well does something
        s0.solve_system(Nb, rp, ci, v.copy(), b)
        assert np.abs(x - s0.get_result()).max() > 1e-6 * np.abs(x).max()


def _pattern_is_a_forest(D):
    Mb = len(D) // 4
    edges = {(min(i, j), max(i, j)) for i in range(Mb) for j in range(Mb) if i != j and D[4 * i:4 * i + 4, 4 * j:4 * j + 4].any()}
    root = list(range(Mb))

    def find(a):
        while root[a] != a:
            a = root[a]
        return a
    for i, j in sorted(edges):
        a, b = find(i), find(j)
        if a == b:
            return False
        root[a] = b
    return True


def test_a_pattern_that_is_no_tree_is_refused(pkg):
    s, Nb, _, _, _ = _grid_solver(pkg, "line_coloring")
    rng = np.random.default_rng(61)
    cells = rng.permutation(Nb)
    good = shapes.well(pkg, shapes.chain(4), cells[:6], seed=601)
    w = shapes.well(pkg, shapes.chain(6), cells[6:14], seed=602)
    _, _, D = pkg.mswells.dense_operators(w, Nb)
    D[4:8, 16:20] = 0.1 * rng.uniform(-1, 1, (4, 4))             # segments 1 and 4: neither is the other's parent
    w["Dcolptr"], w["Drows"], w["Dvals"] = pkg.mswells.csc(D)
    assert not _pattern_is_a_forest(D)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([good, w], form="tree")
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "tree" in str(e.value) and "well 1" in str(e.value)
    assert s.ms_wells_info()["wells"] == 0
    s.set_ms_wells([good, w], form="dense")                      # the dense form takes any pattern
    assert s.ms_wells_info()["wells"] == 2
    # under AUTO a well inside the dense caps never meets the tree form
    s.set_ms_wells([good, w], form="auto")
    assert s.ms_wells_form_info()["dense"] == 2


def _expect_singular_or_pattern_refusal(pkg, s, Nb, rp, ci, v, w, D, segment):
    """form "tree" on a well whose block `segment` is singular at its elimination: INVALID_ARGUMENT naming well and segment at the latest by
    the next product if the pattern is a tree, the pattern's refusal otherwise; the list is cleared and a plain solve has a fresh context's bits"""
    rng = np.random.default_rng(77)
    x = rng.standard_normal(3 * Nb)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.set_ms_wells([w], form="tree")
        s.spmv(x)
    assert e.value.code == pkg.capi.INVALID_ARGUMENT and "well 0" in str(e.value)
    if _pattern_is_a_forest(D):
        assert "segment %d" % segment in str(e.value) and "dense form" in str(e.value) and "inside a segment's block" in str(e.value)
    else:
        assert "tree" in str(e.value) and "cycle" in str(e.value)
    assert s.ms_wells_info()["wells"] == 0
    b = rng.standard_normal(3 * Nb)
    res = s.solve_system(Nb, None, None, v.copy(), b)
    plain, _, _, _, _ = _grid_solver(pkg, "graph_coloring", tolerance=1e-8)
    res0 = plain.solve_system(Nb, None, None, v.copy(), b)
    assert res.converged and res.it == res0.it and np.array_equal(s.get_result(), plain.get_result())


def test_singular_pivot_block(pkg):
    """the permuted D of tests/test_gpu_ms_wells_device.py::test_pivoting_across_the_blocks at Mb = 20 (two block rows exchanged: the leading
    block singular, D regular).  Which refusal applies is decided from the pattern."""
    s, Nb, rp, ci, v = _grid_solver(pkg, "graph_coloring", tolerance=1e-8)
    rng = np.random.default_rng(13)
    cells = rng.permutation(Nb)
    Mb, seed = 20, 52
    w = pkg.mswells.tree_well(Mb, cells[:Mb + 2], seed=seed)
    _, _, D = pkg.mswells.dense_operators(w, Nb)
    other = [i for i in range(1, Mb) if not D[4 * i:4 * i + 4, 0:4].any()][0]
    P = np.arange(4 * Mb)
    P[0:4], P[4 * other:4 * other + 4] = np.arange(4 * other, 4 * other + 4), np.arange(0, 4)
    D = D[P]
    assert np.linalg.matrix_rank(D[:4, :4]) < 4 and np.linalg.matrix_rank(D) == 4 * Mb
    w["Dcolptr"], w["Drows"], w["Dvals"] = pkg.mswells.csc(D)
    _expect_singular_or_pattern_refusal(pkg, s, Nb, rp, ci, v, w, D, 0)


def test_singular_block_inside_a_tree(pkg):
    """a chain whose last segment has a rank-deficient diagonal block while D is regular: the pattern is a tree, so the refusal is the
    device's - the flag of k_ms_wells_tree_factor, found at the next synchronisation; the dense form solves the same well"""
    s, Nb, rp, ci, v = _grid_solver(pkg, "graph_coloring", tolerance=1e-8)
    rng = np.random.default_rng(14)
    cells = rng.permutation(Nb)
    w = shapes.well(pkg, shapes.chain(5), cells[:7], seed=141)
    _, _, D = pkg.mswells.dense_operators(w, Nb)
    D[16:20, 16:20] = 0.0
    D[16, 16] = D[17, 17] = 1.0
    assert np.linalg.matrix_rank(D) == 20 and _pattern_is_a_forest(D)
    w["Dcolptr"], w["Drows"], w["Dvals"] = pkg.mswells.csc(D)
    _expect_singular_or_pattern_refusal(pkg, s, Nb, rp, ci, v, w, D, 4)
    _check_operator(pkg, s, [w], Nb, rng.standard_normal(3 * Nb), form="dense")


def test_other_refusals(pkg):
    s, Nb, _, _, _ = _grid_solver(pkg, "line_coloring")
    good = shapes.well(pkg, shapes.chain(4), [0, 5, 9, 2], seed=81)
    for bad in (3, -1):
        with pytest.raises(pkg.capi.OpmHipError) as e:
            s.set_ms_wells([good], form=bad)
        assert e.value.code == pkg.capi.INVALID_ARGUMENT and "form" in str(e.value)
    with pytest.raises(KeyError):
        s.set_ms_wells([good], form="sparse")
    assert s.ms_wells_form_info()["form"] == "dense" and s.ms_wells_info()["wells"] == 0
    # the form may be set before the pattern; the list may not
    fresh = pkg.capi.HipSolver()
    with pytest.raises(pkg.capi.OpmHipError) as e:
        fresh.set_ms_wells([good], form="tree")
    assert e.value.code == pkg.capi.NOT_READY and fresh.ms_wells_form_info()["form"] == "tree"
    # changing the form clears a list that is set
    s.set_ms_wells([good], form="tree")
    assert s.ms_wells_info()["wells"] == 1
    assert pkg.capi.lib().opmhip_set_ms_wells_form(s._h, 0) == 0
    assert s.ms_wells_info()["wells"] == 0 and s.ms_wells_form_info() == dict(form="dense", dense=0, tree=0, tree_max_segments=0, tree_max_depth=0, tree_kib=0)
    # a decomposed context (loopback, two ranks): refused in every form
    case = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    m = pkg.capi.HipModel(case, comm=("loopback", 2, 0, "mswt" + uuid.uuid4().hex), reorder="level_scheduling")
    for form in ("tree", "auto"):
        with pytest.raises(pkg.capi.OpmHipError) as e:
            m.set_ms_wells([shapes.well(pkg, shapes.chain(2), [0, 1, 2], seed=83)], form=form)
        assert e.value.code == pkg.capi.INVALID_ARGUMENT and "decomposed" in str(e.value)

"""mswells.tree_solve - the block elimination over the segment tree that the device's tree form runs, stated in numpy - against an elimination
with partial pivoting in np.longdouble (cpr_dense.solve_dense), and mswells.D_from_parents against tree_D.  The yardstick is numpy's own
error on the same input: e_ref = the larger error of np.linalg.solve and inv(D) @ z against the longdouble result; 16 e_ref is admitted
(tests/test_gpu_ms_wells_device.py::test_badly_scaled_rows), rows unscaled and scaled by 10^U(-4, 4).  No GPU."""
import numpy as np
import pytest

import ms_tree_shapes as shapes
from cpr_dense import solve_dense

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("name", ["chain1", "chain2", "chain5", "chain65", "chain130", "star71", "comb120", "random150"])
def test_tree_solve_against_longdouble(pkg, name, scaled):
    par = shapes.SHAPES[name]
    rng = np.random.default_rng(len(par) + (1000 if scaled else 0))
    D = pkg.mswells.D_from_parents(par, rng)
    if scaled:
        D = 10.0 ** rng.uniform(-4, 4, len(D))[:, None] * D
    z = rng.standard_normal(len(D)) * (np.abs(D).max(axis=1) if scaled else 1.0)
    x_ld = solve_dense(D, z, np.longdouble)
    e_ref = float(max(np.abs(np.linalg.solve(D, z) - x_ld).max(), np.abs(np.linalg.inv(D) @ z - x_ld).max()))
    err = float(np.abs(pkg.mswells.tree_solve(D, z, par) - x_ld).max())
    print("%s scaled %d: e_ref %.3g, error / e_ref %.3g" % (name, scaled, e_ref, err / e_ref))
    assert err <= 16 * e_ref


def test_tree_solve_300_segments_in_the_bound_of_cond(pkg):
    """M = 1200: an elimination in longdouble takes too long here, so the bound is the operator tests' term in cond_inf(D) for unscaled D"""
    par = shapes.SHAPES["random300"]
    rng = np.random.default_rng(300)
    D = pkg.mswells.D_from_parents(par, rng)
    z = rng.standard_normal(len(D))
    x = np.linalg.solve(D, z)
    assert np.abs(pkg.mswells.tree_solve(D, z, par) - x).max() <= 2 * len(D) * EPS * np.linalg.cond(D, np.inf) * np.abs(x).max()


def test_tree_solve_follows_any_rooting(pkg):
    """the same tree hung on another root is another elimination order of the same D"""
    rng = np.random.default_rng(5)
    par = [1, 2, -1, 2, 3, 0]
    D = pkg.mswells.D_from_parents(par, rng)
    z = rng.standard_normal(24)
    np.testing.assert_allclose(pkg.mswells.tree_solve(D, z, par), np.linalg.solve(D, z), rtol=0, atol=1e-13)
    np.testing.assert_allclose(pkg.mswells.tree_solve(D, z, [-1, 0, 1, 2, 3, 0]), np.linalg.solve(D, z), rtol=0, atol=1e-13)


def test_a_singular_diagonal_block_is_not_pivoted_around(pkg):
    """two block rows exchanged: D regular, its leading block singular - the block elimination stops where a pivoted one goes on"""
    rng = np.random.default_rng(6)
    D = pkg.mswells.D_from_parents(shapes.chain(3), rng)
    P = np.r_[8:12, 4:8, 0:4]
    with pytest.raises(pkg.wells.SingularWellEquations):
        pkg.mswells.tree_solve(D[P], rng.standard_normal(12), [-1, 0, 0])
    assert np.linalg.matrix_rank(D[P]) == 12


def test_D_from_parents_has_the_pattern_of_tree_D_for_a_chain(pkg):
    Mb = 9
    a = pkg.mswells.tree_D(Mb, np.random.default_rng(1), branch=0.0)
    b = pkg.mswells.D_from_parents(shapes.chain(Mb), np.random.default_rng(2))
    assert np.array_equal(a != 0, b != 0)
    # ... and its blocks: the diagonal carries +-4, the blocks beside it offd * U(-1, 1)
    d = np.abs(np.diag(b))
    assert np.all(d >= 4.0) and np.all(d <= 5.0)
    off = b - np.kron(np.eye(Mb), np.ones((4, 4))) * b
    assert 0.0 < np.abs(off).max() <= 0.6
    # a tree in any numbering: the blocks lie between a segment and its parent, both ways, and nowhere else
    par = [3, 0, 0, -1, 2]
    c = pkg.mswells.D_from_parents(par, np.random.default_rng(3)) != 0
    for i in range(5):
        for j in range(5):
            assert c[4 * i:4 * i + 4, 4 * j:4 * j + 4].all() == (i == j or par[i] == j or par[j] == i)
            assert c[4 * i:4 * i + 4, 4 * j:4 * j + 4].any() == (i == j or par[i] == j or par[j] == i)

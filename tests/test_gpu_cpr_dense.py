"""The CPR pressure stage of the device (csrc/cpr.hip) against dense algebra (tests/cpr_dense.py) at the sizes its dense coarse solve
depends on.  Every case first asserts what the other CPR tests assert - cpr_apply = oracle/cpr.hpp bit for bit, in the device's ordering,
which is also why the oracle's aggregates are the device's - and then holds the device's result against the longdouble dense form directly:

    max|v - v_ld| <= 16 max(e_ref, eps max|v_ld|)    per probe and component class (Sw, p, X),

e_ref the dense form's own float64 error (cpr_dense.assert_within).  The coarsest sizes: k_cpr_dense_solve keeps two rows per lane of one
wavefront (rows 0-63 and 64-127), broadcasts x_j from either register by v_readlane, reads its factors four columns ahead and forms the
right-hand side itself (from the finer level's residual) wherever the hierarchy has more than one level; 128 rows is the cap of the
direct solve (CPR_COARSE_DIRECT) and k_cpr_dense_lu_lds tiles the trailing block 32 x 32.  Hence: both sides of lane 64, both sides of
the cap, all four residues mod 4, as the only level and as the coarsest of two.  (Level scheduling leaves a chain in its natural order,
where the block ILU0 is an exact LU and M^-1 d = A^-1 d whatever the pressure stage returned: there the dense form checks the whole
and only the bitwise comparison sees the pressure stage; in the two colourings the ILU0 drops fill and the dense form sees both.)
And the zero pivot of that factorisation, which no
other test raises.  That these tests fail on a wrong kernel cannot be shown without breaking a kernel on the GPU; what is shown (on the
CPU, tests/test_oracle_cpr.py) is that the same criterion fails on an oracle with a wrong damping, a Galerkin sum one term short or a
substitution in the wrong column order."""
import numpy as np
import pytest

import cpr_dense
import oracle_bind

pytestmark = pytest.mark.gpu

DT = 86400.0
REORDERS = ["line_coloring", "graph_coloring", "level_scheduling"]
# mixed heterogeneous cartesian_case(nx, 1, 1) at dt = 1 day: the level sizes the chains were chosen for (found with the CPU oracle; the
# finest level is aggregated in natural visiting order, so they do not depend on the ordering).  Asserted: a change of the aggregation
# must not move the cases off their edges unnoticed.
LEVELS_QUASI = {63: [63], 64: [64], 65: [65], 127: [127], 128: [128], 129: [129, 35], 234: [234, 63], 238: [238, 64], 242: [242, 65],
                246: [246, 66], 465: [465, 126], 469: [469, 127], 472: [472, 128]}
# the same chains with true-IMPES weights handed in: another pressure matrix, other matchings on the longest chains (472: past the cap,
# a third level)
LEVELS_HANDED_IN = dict(LEVELS_QUASI)
LEVELS_HANDED_IN.update({465: [465, 127], 469: [469, 128], 472: [472, 129, 38]})


@pytest.fixture(scope="module")
def systems(pkg, orc):
    """shape -> (case, Jacobian, true-IMPES weights in natural order), assembled once per shape by the oracle"""
    made = {}

    def get(shape, dt=DT):
        if (shape, dt) not in made:
            case = pkg.decks.cartesian_case(*shape, state="mixed", heterogeneous=True)
            o = oracle_bind.OracleModel(orc, case)
            o.set_state(case["pv"], case["meaning"])
            jac, res = o.assemble(dt, 0)
            made[(shape, dt)] = (case, jac, res, o.true_impes_weights(dt))
        return made[(shape, dt)]
    return get


def _device_oracle_dense(pkg, orc, case, jac, reorder, w_nat, levels, ilu, what, seed=0):
    Nb, rp, ci = case["Nb"], case["rowptr"], case["col"]
    s = pkg.capi.HipSolver(reorder=reorder, preconditioner="cpr_quasiimpes" if w_nat is None else "cpr_trueimpes", cpr_amg_ilu_levels=ilu)
    s.set_pattern(Nb, rp, ci)
    s.upload_system(jac)
    s.ilu0_factor(want_factors=False)
    if w_nat is not None:
        s.set_cpr_weights(w_nat)
    to, fr, _ = s.ordering()
    rr, rc, rv = orc.reorder_matrix(Nb, rp, ci, jac, to, fr)
    cpr = oracle_bind.OracleCpr(orc)
    cpr.set_natural_ids(fr)
    if ilu:
        cpr.set_ilu_smoother(ilu, 1)
    if w_nat is not None:
        cpr.set_weights(w_nat[fr])
    cpr.update(Nb, rr, rc, rv)
    D = cpr_dense.probes(Nb, seed)                                     # columns, in the ordering the preconditioner sees
    D_nat = D.reshape(Nb, 3, -1)[to].reshape(3 * Nb, -1)               # the same vectors as the caller hands them over
    v_dev = np.column_stack([s.cpr_apply(np.ascontiguousarray(D_nat[:, k])).reshape(Nb, 3)[fr].reshape(-1) for k in range(D.shape[1])])
    v_orc = np.column_stack([cpr.apply(np.ascontiguousarray(D[:, k])) for k in range(D.shape[1])])
    assert np.array_equal(v_dev, v_orc)                                # first: the device applies the oracle's preconditioner, bit for bit
    n = s.cpr_levels()[0]
    assert n == [int(x) for x in cpr.levels()[0]] and n == levels, (n, levels)
    w = cpr.weights(Nb)
    assert np.array_equal(s.cpr_weights()[fr], w)
    aggs = [cpr.aggregates(l, n[l]) for l in range(len(n) - 1)]
    ref = [cpr_dense.DenseCpr(Nb, rr, rc, rv, w, aggs, dtype=t, ilu0_level0=bool(ilu)).apply(D) for t in (np.longdouble, np.float64)]
    return cpr_dense.assert_within(v_dev, ref[0], ref[1], what)


@pytest.mark.parametrize("weights", ["quasi", "handed_in"])
@pytest.mark.parametrize("reorder", REORDERS)
@pytest.mark.parametrize("nx", sorted(LEVELS_QUASI))
def test_coarsest_level_at_the_sizes_the_dense_solve_depends_on(pkg, orc, systems, nx, reorder, weights):
    case, jac, _, wt = systems((nx, 1, 1))
    levels = (LEVELS_QUASI if weights == "quasi" else LEVELS_HANDED_IN)[nx]
    _device_oracle_dense(pkg, orc, case, jac, reorder, None if weights == "quasi" else wt, levels, 0, "nx %d %s %s" % (nx, reorder, weights), seed=nx)


@pytest.mark.parametrize("reorder,weights", [(r, "quasi") for r in REORDERS] + [("line_coloring", "handed_in")])
@pytest.mark.parametrize("ilu", [0, 1], ids=["jacobi", "ilu0_level0"])
def test_three_levels(pkg, orc, systems, reorder, weights, ilu):
    """(9, 8, 7), 5-day step: three levels, Jacobi everywhere and level 0 smoothed by its scalar ILU0 in the block ILU0's ordering
    (cpr_amg_ilu_levels = 1, what the benchmark's CPR runs use)"""
    case, jac, _, wt = systems((9, 8, 7), 5 * DT)
    levels = [504, 160, 57] if weights == "quasi" else [504, 152, 44]
    _device_oracle_dense(pkg, orc, case, jac, reorder, None if weights == "quasi" else wt, levels, ilu, "9x8x7 %s %s ilu %d" % (reorder, weights, ilu))


def test_zero_pivot_of_the_coarsest_level(pkg, orc, systems):
    """Weights whose row for cell 0 is (c1, -c0, 0), c the pressure column of cell 0's diagonal block: a_p[0,0] = c0 c1 - c1 c0 is exactly
    0, cell 0 is eliminated first, and the dense LU (no pivoting) of the one-level hierarchy meets a zero pivot.  solve_system fails with
    CREATE_PRECONDITIONER_FAILED and says which factorisation it was; the same context then solves the same system with good weights to
    the bits of a fresh context."""
    case, jac, res, wt = systems((3, 2, 1))
    Nb, rp, ci = case["Nb"], case["rowptr"], case["col"]
    d0 = [k for k in range(rp[0], rp[1]) if ci[k] == 0][0]
    c = jac.reshape(-1, 3, 3)[d0][:, 1]
    bad = wt.copy()
    bad[0] = (c[1], -c[0], 0.0)
    assert c[0] != 0.0 and c[1] != 0.0 and c[0] * bad[0, 0] + c[1] * bad[0, 1] == 0.0

    def solver():
        s = pkg.capi.HipSolver(preconditioner="cpr_trueimpes")
        s.set_pattern(Nb, rp, ci)
        return s
    s = solver()
    assert s.ordering()[0][0] == 0                  # cell 0 comes first in the device's ordering: its a_p is the first pivot
    s.set_cpr_weights(bad)
    with pytest.raises(pkg.capi.OpmHipError) as e:
        s.solve_system(Nb, rp, ci, jac.copy(), res)
    assert e.value.code == pkg.capi.CREATE_PRECONDITIONER_FAILED
    assert "CPR: the dense LU of the coarsest pressure level met a zero or non-finite pivot" in str(e.value)
    s.set_cpr_weights(wt)
    r = s.solve_system(Nb, rp, ci, jac.copy(), res)
    f = solver()
    f.set_cpr_weights(wt)
    rf = f.solve_system(Nb, rp, ci, jac.copy(), res)
    assert r.converged and rf.converged and r.it == rf.it
    x = s.get_result()
    assert np.all(np.isfinite(x)) and np.array_equal(x, f.get_result())

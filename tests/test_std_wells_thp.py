"""wells.StandardWells with THP limits through VFPPROD / VFPINJ tables, on the CPU over the oracle: the stated form against the NumPy form,
the switching table of update_well_controls, and a list without limits against vfp=None.  (tests/thp_cases.py holds the case; the device
form is compared with the stated one in tests/test_gpu_std_wells_thp.py.)"""
import numpy as np
import pytest

import oracle_bind
import thp_cases

EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def setup(pkg, orc):
    case = thp_cases.make_case(pkg)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    return case, om.iq(), thp_cases.tables(pkg)


def wells(pkg, setup, arithmetic="stated", limits=True, vfp=True):
    case, iq, tabs = setup
    return pkg.wells.StandardWells(thp_cases.make_wells(pkg, case, limits=limits), case["depth"], arithmetic=arithmetic, vfp=tabs if vfp else None)


def solved(pkg, setup, **kw):
    w = wells(pkg, setup, **kw)
    w.calculate_explicit_quantities(setup[1])
    w.solve_well_equations(setup[1])
    return w


def test_stated_form_against_the_numpy_form_under_thp_control(pkg, setup):
    """The two forms differ in the order of the per-well sums (one lane's loop against pairwise) and in D^-1 (Gauss-Jordan against LAPACK);
    the THP row, like every control row, is elementwise arithmetic in both.  So at one x: the control rows and B, C are EQUAL; a sum of n
    terms carries at most (n - 1) eps sum|terms| in either order, so the two differ by at most 2 (n - 1) eps sum|terms| (n = 65 for P65);
    D^-1 of both is within 16 eps cond(D) max|D^-1| of the exact inverse (the bound test_invert4_stated holds the stated form to), so
    they differ by at most twice that."""
    case, iq, tabs = setup
    ws, wn = solved(pkg, setup), solved(pkg, setup, arithmetic="numpy")
    for w in (ws, wn):
        w.update_well_controls()
    assert [w.control[0] for w in ws.wells] == [w.control[0] for w in wn.wells] == ["thp", "thp", "rate"]
    x0 = ws.x.copy()
    x0[:, :3] *= 0.8
    x0[:, 3] += [-1e5, 2e5, -1e5]
    ws.x, wn.x = x0.copy(), x0.copy()
    (rs, Ds, Bs, Cs, src_s, _), (rn, Dn, Bn, Cn, src_n, _) = ws._assemble_wells(iq), wn._assemble_wells(iq)
    assert np.array_equal(rs[:, 3], rn[:, 3]) and np.array_equal(Ds[:, 3, :], Dn[:, 3, :]) and np.array_equal(Bs, Bn) and np.array_equal(Cs, Cn)
    assert np.array_equal(src_s, src_n)
    assert np.all(Ds[0, 3, [0, 2]] != 0.0) and Ds[0, 3, 3] == 1.0 and Ds[1, 3, 1] != 0.0 and np.all(rs[:2, 3] != 0.0)
    pr = ws._perf_rates(iq, x0[:, 3])
    for k in range(ws.nw):
        lo, hi = ws.vp[k], ws.vp[k + 1]
        bound = 2.0 * (hi - lo - 1) * EPS
        assert np.all(np.abs(rs[k, :3] - rn[k, :3]) <= bound * np.abs(pr[lo:hi, :, 0]).sum(axis=0))
        assert np.all(np.abs(Ds[k, :3, 3] - Dn[k, :3, 3]) <= bound * np.abs(pr[lo:hi, :, 4]).sum(axis=0))
        inv_s, inv_n = pkg.wells.invert4_stated(Ds[k]), np.linalg.inv(Dn[k])
        assert np.abs(inv_s - inv_n).max() <= 2 * 16 * EPS * np.linalg.cond(Dn[k]) * np.abs(inv_n).max()
    # the wells alone under THP control: both forms reach V - dp, to the stopping test's 1e-3 Pa
    for w in (ws, wn):
        w.solve_well_equations(iq)
        a = w.assemble(iq)
        assert np.all(np.abs(w.x[:2, 3] - w.bhp_from_thp[:2]) <= 2e-3) and w.converged(a["res_well"])
        assert -40.0 / thp_cases.DAY < w.x[0, 0] < 0.0 and 0.0 < w.x[1, 1] < 60.0 / thp_cases.DAY      # the limits cost both wells rate


def test_control_row_is_the_statement(pkg, setup):
    """r = bhp - (V - dp), D[3][j] = 0 - dV/dq_j in the unknowns' order (oil, water, gas), D[3][3] = 1; dp = (rho_o g) dh of the first
    perforation's cell"""
    case, iq, tabs = setup
    w = solved(pkg, setup)
    w.update_well_controls()
    W, vfp = pkg.wells, pkg.vfp
    r, g = w._control_rows()
    for k, t in ((0, tabs[0]), (1, tabs[1])):
        q = w.x[k]
        V = vfp.bhp(t, q[W.WATER], q[W.OIL], q[W.GAS], w.wells[k].thp_limit, 0.0)
        rho = iq[w.wells[k].cells[0], W.F_RHO + W.PH_O, 0]
        dp = (rho * W.GRAVITY) * (2490.0 - w.wells[k].ref_depth)
        assert w.thp_dp[k] == dp and dp < 0.0
        assert r[k] == q[3] - (V[0] - dp) and np.array_equal(g[k], [0.0 - V[7], 0.0 - V[6], 0.0 - V[8], 1.0])
    assert w.thp_dp[2] == 0.0 and np.array_equal(g[2], [1.0, 0.0, 0.0, 0.0])


def test_switching_table(pkg, setup):
    w = solved(pkg, setup)
    xs = w.x.copy()
    vfp, W = pkg.vfp, pkg.wells
    names = []
    for name, k, before, x, after in thp_cases.transitions(xs):
        w.x = xs.copy()
        w.x[k] = x
        for q in w.wells:
            q.control = q.rate_control
        w.wells[k].control = thp_cases.control_of(w.wells[k], before)
        w.update_well_controls()
        well = w.wells[k]
        assert well.control == thp_cases.control_of(well, after), name
        current = vfp.thp(w.thp_tables[k], x[W.WATER], x[W.OIL], x[W.GAS], x[3] + w.thp_dp[k], 0.0)
        assert w.thp_current[k] == current, name
        if after == before:
            assert np.array_equal(w.x[k], x), name
        elif after == "bhp":
            assert w.x[k, 3] == well.bhp_limit and np.array_equal(w.x[k, :3], x[:3]), name
        elif after == "thp":
            V = vfp.bhp(w.thp_tables[k], x[W.WATER], x[W.OIL], x[W.GAS], well.thp_limit, 0.0)[0]
            assert w.x[k, 3] == V - w.thp_dp[k] and np.array_equal(w.x[k, :3], x[:3]), name
            assert (well.thp_limit > current) if well.producer else (well.thp_limit < current), name
        else:
            assert np.array_equal(w.x[k], x), name
        names.append((before, after, k))
    for k in (0, 1):
        assert {("rate", "thp", k), ("bhp", "thp", k), ("thp", "bhp", k), ("thp", "rate", k), ("rate", "bhp", k)} <= set(names)
    assert w.wells[2].control[0] == "rate" and w.thp_current[2] == 0.0


def test_a_list_without_limits_gives_the_bits_of_vfp_none(pkg, setup):
    case, iq, tabs = setup
    runs = []
    for kw in (dict(limits=False, vfp=False), dict(limits=False, vfp=True)):
        w = solved(pkg, setup, **kw)
        w.update_well_controls()
        a = w.assemble(iq)
        runs.append((w.x.copy(), a["res_well"], a["wells"]["Dnnzs"], a["wells"]["Bnnzs"], a["wells"]["Cnnzs"], a["source_cells"], [q.control for q in w.wells]))
    for p, q in zip(*runs):
        assert np.array_equal(p, q) if not isinstance(p, list) else p == q
    # ... and the limits do change something
    w = solved(pkg, setup)
    w.update_well_controls()
    assert not np.array_equal(w.x, runs[0][0]) and [q.control[0] for q in w.wells] != [c[0] for c in runs[0][6]]


def test_state_convergence_and_events(pkg, setup):
    case, iq, tabs = setup
    w = solved(pkg, setup)
    w.update_well_controls()
    st = w.state()
    assert st[1][0] == ("thp", thp_cases.PROD_LIMIT)
    rw = np.zeros((3, 4))
    rw[0, 3] = 0.5                                         # half a pascal off on a THP row: judged with tol_bhp, like a BHP row
    assert w.converged(rw) and not w.converged(rw * 4.0)
    w.wells[0].control = w.wells[0].rate_control
    assert not w.converged(rw)                             # ... a rate row is judged in rates
    w.set_state(st)
    assert w.wells[0].control == ("thp", thp_cases.PROD_LIMIT) and np.array_equal(w.x, st[0])
    w.set_rate_target(0, 10.0 / thp_cases.DAY)             # an event puts the well under the deck's mode again
    assert w.wells[0].control == ("rate", pkg.wells.OIL, 10.0 / thp_cases.DAY) and w.x[0, 0] == -10.0 / thp_cases.DAY
    W = pkg.wells
    with pytest.raises(ValueError, match="come together"):
        W.Well("X", [0], [1.0], 0.0, True, ("rate", W.OIL, 1.0), 1e5, thp_limit=1e5)
    with pytest.raises(ValueError, match="THP control"):
        W.Well("X", [0], [1.0], 0.0, True, ("thp", 2e5), 1e5, thp_limit=1e5, vfp_table=5)
    with pytest.raises(ValueError, match="tables with the number"):
        W.StandardWells([W.Well("X", [0], [1.0], 0.0, False, ("rate", W.WATER, 1.0), 1e5, inj_phase="water", thp_limit=1e5, vfp_table=5)], np.zeros(1), vfp=tabs)

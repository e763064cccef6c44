"""Crossflow in producers (wells.Well(allow_crossflow=True)): the injecting branch of StandardWellEval::computePerfRate for a producer's
reversed perforations, in both arithmetics of wells.StandardWells, on the CPU over the oracle.

Grid: 2 x 2 x 150 (cell = i + 2 (j + 2 k)), one well per column: producers of 150, 65 and 1 completions with the switch, a 64-completion
water injector without.  The forced-reversal state: the wells alone solved, then the long producer's bottom-hole pressure at the median
of p_o - head over its completions, so that half of them are reversed while q != 0.

Measured here (numpy 2.2.6), largest relative difference; the tests assert 100 x these, and equality where the measured value is 0:

    stated rates against the scalar np.longdouble restatement (values of all 150 perforations of the long producer): 1.11e-11
        (MEASURED_FORMULA; not a few eps: the drawdown p_o - (bhp + head) of the perforation nearest the median is 125 Pa, the difference
        of two numbers of 2.5e7 whose rounding, 5e-9 Pa, is 4e-11 of it - in the producing branch as in the injecting one)

    stated against NumPy form on the forced-reversal state, every well moved off its solved state (MEASURED; tests/test_std_wells_stated.py's
    comparisons and its reasons: D^-1 relative to its row's largest |entry|, and entry by entry above the row's rounding floor):
        r_w 5.3e-16    D^-1 per row 3.2e-15    D^-1 per entry 6.5e-7 (the full D of the crossflow well has cond(D) = 3.3e10; without
        crossflow D is I plus one column and both inversions are nearly exact)    B, C, source, dsource 0    x after the wells alone 3.0e-16

    the seven derivatives against central differences: 7.2e-11 of the row's largest entry (asserted: 1e-6, the issue's bound)

The derivatives (test 2) are compared with central differences of relative step 1e-6: rounding about eps / h = 2e-10, truncation about
h^2 = 1e-12.  "1e-6 of the row's largest entry" is taken on a row whose entries have one unit: the seven derivatives of one rate of one
perforation, each times the magnitude of its variable (the magnitude its step is 1e-6 of) - d rate / d ln(variable).  Unscaled, a row
would put d/dp (1e-11) beside d/dq (1) and check only the latter."""
import numpy as np
import pytest

import oracle_bind

DAY = 86400.0
MEASURED_FORMULA = 1.12e-11
MEASURED = dict(res_well=5.3e-16, Dinv=3.2e-15, Dinv_entries=6.5e-7, B=0.0, C=0.0, source=0.0, dsource=0.0, solved_x=3.0e-16)


def column(i, j, ks):
    return [i + 2 * (j + 2 * k) for k in ks]


def make_case(pkg):
    return pkg.decks.cartesian_case(2, 2, 150, state="mixed", heterogeneous=True, dz=1.0)


def make_wells(pkg, case, crossflow=True):
    """producers of 150, 65 and 1 completions (with the switch), a 64-completion water injector (without); no cell is shared"""
    W = pkg.wells

    def well(name, cells, producer, control, limit, inj=None):
        tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return W.Well(name, cells, tw, case["depth"][cells[0]], producer, control, limit, inj_phase=inj, allow_crossflow=crossflow and producer)
    return [well("P150", column(0, 0, range(150)), True, ("rate", W.OIL, 40.0 / DAY), 150e5),
            well("W64", column(1, 0, range(64)), False, ("rate", W.WATER, 60.0 / DAY), 400e5, "water"),
            well("P65", column(0, 1, range(65)), True, ("rate", W.OIL, 20.0 / DAY), 150e5),
            well("P1", column(1, 1, [100]), True, ("rate", W.OIL, 2.0 / DAY), 150e5)]


def median_bhp(w, records):
    """the long producer's bottom-hole pressure at which half of its completions are reversed"""
    po = records[:, 4, 0] if not hasattr(records, "rows") else records.rows(w.cells)[:, 4, 0]
    return float(np.median((po[:150] - w.head[:150])))


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    d, s = np.abs(a - b), np.maximum(np.abs(a), np.abs(b))
    m = s > 0
    return float((d[m] / s[m]).max()) if m.any() else 0.0


def rel_rows(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float((np.abs(a - b) / np.abs(a).max(axis=-1, keepdims=True)).max())


def rel_entries_above_the_floor(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    m = np.abs(a) > 16 * np.finfo(float).eps * np.abs(a).max(axis=-1, keepdims=True)
    assert 3 * m.sum() > 2 * np.count_nonzero(a)
    return float((np.abs(a - b)[m] / np.abs(a)[m]).max())


def same(a, b):
    """everything assemble() returns, np.array_equal"""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            if not same(a[k], b[k]):
                return False
        elif not np.array_equal(a[k], b[k]):
            return False
    return True


@pytest.fixture(scope="module")
def setup(pkg, orc):
    case = make_case(pkg)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq().copy()
    ws = pkg.wells.StandardWells(make_wells(pkg, case), case["depth"], arithmetic="stated")
    ws.calculate_explicit_quantities(iq)
    ws.solve_well_equations(iq)
    x0 = ws.x.copy()
    x0[0, 3] = median_bhp(ws, iq[ws.cells])
    return dict(case=case, om=om, iq=iq, x0=x0, head=ws.head.copy(), solved=ws.x.copy())


def stated_at(pkg, s, x=None, crossflow=True, arithmetic="stated"):
    ws = pkg.wells.StandardWells(make_wells(pkg, s["case"], crossflow), s["case"]["depth"], arithmetic=arithmetic)
    ws.head = s["head"].copy()
    ws.x = (s["x0"] if x is None else x).copy()
    ws.initialised = True
    return ws


# ---- 1. the formula --------------------------------------------------------------------------------------------------------------------------
def longdouble_rates(W, ws, iq):
    """the module docstring's formulas for the long producer, one perforation at a time in np.longdouble"""
    L = np.longdouble
    q = iq[ws.cells]
    out = np.zeros((150, 3))
    qo, qw, qg = (L(v) for v in ws.x[0, :3])
    p = {W.OIL: max(-qo, L(0)), W.WATER: max(-qw, L(0)), W.GAS: max(-qg, L(0))}
    P = (p[W.OIL] + p[W.WATER]) + p[W.GAS]
    cmix = {c: p[c] / P for c in p}
    for k in range(150):
        val = lambda f: L(q[k, f, 0])
        dd = val(W.F_P + W.PH_O) - (L(ws.x[0, 3]) + L(ws.head[k]))
        tw = L(ws.tw[k])
        b = {ph: val(W.F_B + ph) for ph in range(3)}
        mob = {ph: val(W.F_MOB + ph) for ph in range(3)}
        rs = val(W.F_RS)
        if dd > 0:
            so, sw, sg = (b[ph] * (-tw * (mob[ph] * dd)) for ph in (W.PH_O, W.PH_W, W.PH_G))
            out[k] = [float(so), float(sw), float(sg + rs * so)]
        else:
            cqt_i = -tw * (mob[W.PH_W] + mob[W.PH_O] + mob[W.PH_G]) * dd
            ratio = cmix[W.WATER] / b[W.PH_W] + cmix[W.OIL] / b[W.PH_O] + (cmix[W.GAS] - rs * cmix[W.OIL]) / b[W.PH_G]
            assert ratio > 0
            out[k] = [float(cmix[c] * (cqt_i / ratio)) for c in (W.OIL, W.WATER, W.GAS)]
    return out


def test_formula_against_a_longdouble_restatement(pkg, setup):
    W = pkg.wells
    ws = stated_at(pkg, setup)
    iq = setup["iq"]
    assert np.all(ws.x[0, :3] < 0.0)                                      # the well has flowed: q != 0
    pr = ws._perf_rates(iq, ws.x[:, 3])
    dd = iq[ws.cells][:150, W.F_P + W.PH_O, 0] - (ws.x[0, 3] + ws.head[:150])
    reversed_ = ~(dd > 0.0)
    assert 10 <= reversed_.sum() <= 140
    assert np.all((pr[:150, :, 0][reversed_] > 0.0).any(axis=1))         # every reversed perforation injects some component
    assert np.all(pr[:150, :, 0][reversed_] >= 0.0) and np.all(pr[:150, :, 0][~reversed_] <= 0.0)
    want = longdouble_rates(W, ws, iq)
    got = rel(pr[:150, :, 0], want)
    print("stated rates against the longdouble restatement: %.2e (reversed perforations alone: %.2e)" % (got, rel(pr[:150, :, 0][reversed_], want[reversed_])))
    assert got <= 100.0 * MEASURED_FORMULA


# ---- 2. the derivatives ------------------------------------------------------------------------------------------------------------------------
def test_derivatives_against_central_differences(pkg, setup):
    """all seven derivatives (d/dSw, d/dp, d/dX of the cell, d/dbhp, d/dq_o, d/dq_w, d/dq_g) of the three rates of every perforation of the
    long producer; a second pass with q_w > 0, the clamp's flat side (d/dq_w = 0 there)"""
    W = pkg.wells
    case, om = setup["case"], setup["om"]
    pv0 = case["pv"].reshape(-1, 3)
    cells = np.asarray(column(0, 0, range(150)))
    mag = np.ones_like(pv0)                                               # saturations (and a gas saturation as X): steps of 1e-6
    mag[:, 1] = np.abs(pv0[:, 1])                                         # pressures: 1e-6 of the pressure
    mag[:, 2] = np.maximum(np.abs(pv0[:, 2]), 1.0)                        # X as Rs: 1e-6 of it
    h = 1e-6
    iqs = {}
    try:
        for v in range(3):
            for sign in (1.0, -1.0):
                pv = pv0.copy()
                pv[:, v] += sign * h * mag[:, v]
                om.set_state(pv.reshape(-1), case["meaning"])
                iqs[v, sign] = om.iq().copy()
    finally:
        om.set_state(case["pv"], case["meaning"])
    flat = setup["x0"].copy()
    flat[0, W.WATER] = 1e-6                                               # q_w >= 0: no water in the well bore's mixture
    worst = 0.0
    for name, x0 in (("q < 0", setup["x0"]), ("q_w > 0", flat)):
        ws = stated_at(pkg, setup, x0)
        pr = ws._perf_rates(setup["iq"], ws.x[:, 3])[:150]
        dq = ws._rate_dq[:150]
        dd = setup["iq"][ws.cells][:150, W.F_P + W.PH_O, 0] - (ws.x[0, 3] + ws.head[:150])
        reversed_ = ~(dd > 0.0)
        assert 10 <= reversed_.sum() <= 140 and np.abs(dd).min() > 2.0 * h * mag[cells, 1].max()      # no perforation changes side within a step
        analytic = np.concatenate([pr[:, :, 1:], dq], axis=2)             # (150, 3, 7)
        scale = np.zeros((150, 7))
        fd = np.zeros((150, 3, 7))
        for v in range(3):
            scale[:, v] = mag[cells, v]
            f = [ws._perf_rates(iqs[v, sign], ws.x[:, 3])[:150, :, 0] for sign in (1.0, -1.0)]
            fd[:, :, v] = (f[0] - f[1]) / (2.0 * h * scale[:, v, None])
        for v in range(4):                                                # bhp, q_o, q_w, q_g
            col = 3 if v == 0 else v - 1
            scale[:, 3 + v] = abs(x0[0, col])
            f = []
            for sign in (1.0, -1.0):
                ws.x = x0.copy()
                ws.x[0, col] += sign * h * abs(x0[0, col])
                f.append(ws._perf_rates(setup["iq"], ws.x[:, 3])[:150, :, 0])
            fd[:, :, 3 + v] = (f[0] - f[1]) / (2.0 * h * abs(x0[0, col]))
        a, d = analytic * scale[:, None, :], fd * scale[:, None, :]
        big = np.abs(a).max(axis=2, keepdims=True)
        err = float((np.abs(a - d) / np.where(big > 0.0, big, 1.0)).max())
        print("derivatives against central differences, %s: %.2e of the row's largest entry (reversed perforations: %d)" % (name, err, reversed_.sum()))
        worst = max(worst, err)
        # the q-derivatives are there at all, and exactly zero on the clamp's flat side and in producing perforations
        assert np.all(np.abs(dq[reversed_][:, :, W.OIL]).max(axis=1) > 0.0) and np.all(dq[~reversed_] == 0.0)
        if name == "q_w > 0":
            assert np.all(dq[:, :, W.WATER] == 0.0) and np.all(pr[reversed_][:, W.WATER, :] == 0.0) and np.all(fd[:, :, 3 + 1 + W.WATER] == 0.0)
        else:
            assert np.all(np.abs(dq[reversed_][:, :, W.WATER]).max(axis=1) > 0.0)
    assert worst <= 1e-6


# ---- 3. stated against the NumPy form ----------------------------------------------------------------------------------------------------------
def test_stated_form_against_the_numpy_form(pkg, setup):
    iq = setup["iq"]
    forms = []
    for arithmetic in ("numpy", "stated"):
        w = pkg.wells.StandardWells(make_wells(pkg, setup["case"]), setup["case"]["depth"], arithmetic=arithmetic)
        w.calculate_explicit_quantities(iq)
        w.solve_well_equations(iq)
        forms.append(w)
    wn, ws = forms
    got = dict(solved_x=rel(wn.x, ws.x))
    # one state for both: the long producer's forced reversal, and every well away from the solved state - the residuals are not zero
    x0 = setup["x0"].copy()
    x0[:, :3] *= 1.02
    x0[1:, 3] += np.where([w.producer for w in wn.wells[1:]], -2e5, 3e5)
    wn.x, ws.x = x0.copy(), x0.copy()
    an, a_s = wn.assemble(iq), ws.assemble(iq)
    Dn, Ds = an["wells"]["Dnnzs"].reshape(-1, 4, 4), a_s["wells"]["Dnnzs"].reshape(-1, 4, 4)
    got["res_well"] = rel(an["res_well"], a_s["res_well"])
    got["Dinv"], got["Dinv_entries"] = rel_rows(Dn, Ds), rel_entries_above_the_floor(Dn, Ds)
    got["B"], got["C"] = rel(an["wells"]["Bnnzs"], a_s["wells"]["Bnnzs"]), rel(an["wells"]["Cnnzs"], a_s["wells"]["Cnnzs"])
    got["source"], got["dsource"] = rel(an["source_cells"], a_s["source_cells"]), rel(an["dsource_cells"], a_s["dsource_cells"])
    print("crossflow, stated against numpy:", {k: "%.2e" % v for k, v in got.items()}, "cond(D) %.1e" % np.linalg.cond(ws._assemble_wells(iq)[1][0]))
    C = a_s["wells"]["Cnnzs"].reshape(-1, 4, 3)
    assert np.any(C[:150, :3, :] != 0.0) and np.all(C[150:214, :3, :] == 0.0) and np.any(ws.rate_dq != 0.0)
    assert 2 * np.count_nonzero(an["res_well"]) > an["res_well"].size
    for k, v in got.items():
        bound = 100.0 * MEASURED[k]
        assert v <= bound, (k, v, bound)          # a measured 0 asks for equality


# ---- 4. nothing moves when it should not -------------------------------------------------------------------------------------------------------
def rates_without_crossflow(ws):
    """the rate model as it was before the switch existed, for StandardWells._perf_rates' hook: producing perforations of producers,
    injecting perforations of injectors, every other perforation closed"""
    W = type(ws)

    def perf_rates(iq, bhp):
        from importlib import import_module
        M = import_module(W.__module__)
        q = M._rows(iq, ws.cells)
        n = len(ws.cells)
        ad = lambda f: np.concatenate([q[:, f, :], np.zeros((n, 1))], axis=1)

        def mul(a, b):
            out = np.empty_like(a)
            out[:, 0] = a[:, 0] * b[:, 0]
            out[:, 1:] = a[:, :1] * b[:, 1:] + b[:, :1] * a[:, 1:]
            return out
        dd = ad(M.F_P + M.PH_O)
        dd[:, 0] -= np.asarray(bhp)[ws.well_of_perf] + ws.head
        dd[:, 4] = -1.0
        b, mob, rs = [ad(M.F_B + ph) for ph in range(3)], [ad(M.F_MOB + ph) for ph in range(3)], ad(M.F_RS)
        tw = ws.tw[:, None]
        out = np.zeros((n, 3, 5))
        producer = np.array([w.producer for w in ws.wells])[ws.well_of_perf]
        flows = producer & (dd[:, 0] > 0.0)
        surf = [mul(b[ph], -tw * mul(mob[ph], dd)) for ph in range(3)]
        out[flows, M.OIL], out[flows, M.WATER] = surf[M.PH_O][flows], surf[M.PH_W][flows]
        out[flows, M.GAS] = (surf[M.PH_G] + mul(rs, surf[M.PH_O]))[flows]
        inj = ~producer & (dd[:, 0] < 0.0)
        vol = -tw * mul(mob[0] + mob[1] + mob[2], dd)
        for name, ph, comp in (("gas", M.PH_G, M.GAS), ("water", M.PH_W, M.WATER), ("oil", M.PH_O, M.OIL)):
            sel = inj & np.array([w.inj_phase == name for w in ws.wells])[ws.well_of_perf]
            out[sel, comp] = mul(b[ph], vol)[sel]
        return out
    return perf_rates


@pytest.mark.parametrize("arithmetic", ["stated", "numpy"])
def test_nothing_moves_when_it_should_not(pkg, setup, arithmetic):
    iq = setup["iq"]
    W = pkg.wells
    # (a) the switch off, on the state with reversed perforations: the rate model from before the switch
    off = stated_at(pkg, setup, crossflow=False, arithmetic=arithmetic)
    before = stated_at(pkg, setup, crossflow=False, arithmetic=arithmetic)
    before._perf_rates = rates_without_crossflow(before)
    a_off = off.assemble(iq)
    assert same(a_off, before.assemble(iq)) and np.all(off.rate_dq == 0.0)
    assert np.all(a_off["wells"]["Cnnzs"].reshape(-1, 4, 3)[:, :3, :] == 0.0)
    on = stated_at(pkg, setup, crossflow=True, arithmetic=arithmetic)
    assert not same(on.assemble(iq), a_off)                               # (the switch does act on this state)
    # (b) the switch on, no perforation reversed: every producer's bottom-hole pressure below all of its completions'
    x = setup["x0"].copy()
    inflow = iq[on.cells][:, W.F_P + W.PH_O, 0] - setup["head"]
    for k in (0, 2, 3):
        x[k, 3] = inflow[on.vp[k]:on.vp[k + 1]].min() - 1e5
    on, off = (stated_at(pkg, setup, x, crossflow=cf, arithmetic=arithmetic) for cf in (True, False))
    assert same(on.assemble(iq), off.assemble(iq)) and on._rate_dq is None
    # (c) P == 0: a well that has not flowed yet keeps its reversed perforations closed
    x = setup["x0"].copy()
    x[:, :3] = 0.0
    on, off = (stated_at(pkg, setup, x, crossflow=cf, arithmetic=arithmetic) for cf in (True, False))
    a_on = on.assemble(iq)
    assert same(a_on, off.assemble(iq)) and np.all(np.isfinite(a_on["wells"]["Dnnzs"]))
    rates = on._perf_rates(iq, on.x[:, 3])[:150, :, 0]
    assert 10 <= np.all(rates == 0.0, axis=1).sum() <= 140


# ---- 5. the wells alone converge ---------------------------------------------------------------------------------------------------------------
def test_the_wells_alone_converge(pkg, setup):
    iq = setup["iq"]
    runs = {}
    for cf in (True, False):
        ws = stated_at(pkg, setup, crossflow=cf)
        calls = []
        inner = ws._assemble_wells
        ws._assemble_wells = lambda iq, inner=inner, calls=calls: (calls.append(1), inner(iq))[1]
        ws.solve_well_equations(iq)
        ws._assemble_wells = inner
        # its stopping test was met inside the loop: the loop ended early, and one more step from where it stopped is below the test
        r, D, *_ = ws._assemble_wells(iq)
        dx = np.array([pkg.wells.row_times_vector(pkg.wells.invert4_stated(D[k]), r[k]) for k in range(ws.nw)])
        small = (np.abs(dx[:, :3]).max(axis=1) <= 1e-12 * np.maximum(1e-6, np.abs(ws.x[:, :3]).max(axis=1))) & (np.abs(dx[:, 3]) <= 1e-3)
        assert len(calls) < 20 and small.all(), (cf, len(calls), dx)
        wa = ws.assemble(iq)
        assert ws.converged(wa["res_well"])
        runs[cf] = (ws.x.copy(), ws._perf_rates(iq, ws.x[:, 3])[:, :, 0], len(calls))
    (x_on, rates_on, n_on), (x_off, rates_off, n_off) = runs[True], runs[False]
    injecting = (rates_on[:150] > 0.0).any(axis=1).sum()
    print("the wells alone: %d / %d iterations with / without crossflow; bhp %.6e / %.6e; %d of 150 perforations inject" % (n_on, n_off, x_on[0, 3], x_off[0, 3], injecting))
    assert x_on[0, 3] != x_off[0, 3] and abs(x_on[0, 3] - x_off[0, 3]) > 1e3
    assert injecting >= 1 and not (rates_off > 0.0)[:150].any()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_an_injector_with_the_switch_is_refused(pkg, setup):
    W = pkg.wells
    with pytest.raises(ValueError, match="injector"):
        W.Well("I", [0], [1e-12], 0.0, False, ("rate", W.WATER, 1e-4), 400e5, inj_phase="water", allow_crossflow=True)
    wells = make_wells(pkg, setup["case"])
    wells[1].allow_crossflow = True                                       # set behind the constructor's back
    for arithmetic in ("numpy", "stated"):
        with pytest.raises(ValueError, match="injector"):
            W.StandardWells(wells, setup["case"]["depth"], arithmetic=arithmetic)
    assert not W.Well("P", [0], [1e-12], 0.0, True, ("rate", W.OIL, 1e-4), 100e5).allow_crossflow       # off by default

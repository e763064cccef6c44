"""Vaporised oil in the connection rates (wells.StandardWells(vaporised_oil=True)): the rs / rv terms of StandardWellEval::computePerfRate
in both arithmetics of wells.StandardWells, on the CPU over the oracle.

Case: helpers.wetgas_case(pkg, 3, 3, 70, heterogeneous=True, dz=1.0) - gas cap (meaning 2: Sw, pg, Rv), three-phase zone, oil leg - with
decks.gas_condensate_wells: PLONG (70 completions through all three zones, crossflow allowed), PCAP (one completion in the gas cap, GRAT
target, ORAT limit), GINJ (gas injector, 5 completions).  The state of the comparisons: the wells alone solved, the controls updated
(PCAP falls to its ORAT limit: its oil is vaporised oil only), PLONG's bottom-hole pressure at the median of p_o - head, so that half of
its completions are reversed in every zone, and every rate unknown 5 % off, so that r_w is not a difference of equal numbers.

Measured here (numpy 2.2.6), largest relative difference; the tests assert 100 x these, and equality where the measured value is 0.
Every array entry by entry, except D^-1, which is taken relative to its row's largest |entry| (tests/test_std_wells_stated.py's reason):

    stated against the np.longdouble restatement below (MEASURED_FORMULA):
        rates  6.3e-13   dq  6.3e-13   B  6.3e-13   C  6.3e-13   D  5.1e-15   r_w  1.1e-11   solution rates  7.2e-15
        (not a few eps: the drawdown p_o - (bhp + head) of the two perforations nearest the median is 2650 Pa, the difference of two
        numbers of 2.5e7 whose rounding, 4e-9 Pa, is 1.4e-12 of it; the largest r_w difference is the gas injector's, whose drawdowns are
        differences of the same kind and whose r_w is the twentieth part of the sum of its rates)
    NumPy form against stated (MEASURED_NUMPY):
        rates  0   dq  0   B  0   C  0   D  3.7e-16   r_w  0   D^-1 per row  1.9e-14   solution rates  1.6e-16

Not here: a dry-gas fluid written as PVTG with Rv = 0 under both switch positions - the oracle's PVTG wants undersaturated data in its last
table (fluid.hpp's assertion), so the fixture allows no such fluid.
"""
import numpy as np
import pytest

import helpers
import oracle_bind

DAY = 86400.0
L = np.longdouble
MEASURED_FORMULA = dict(rates=6.3e-13, dq=6.3e-13, B=6.3e-13, C=6.3e-13, D=5.1e-15, rw=1.1e-11, sol=7.2e-15)
MEASURED_NUMPY = dict(rates=0.0, dq=0.0, B=0.0, C=0.0, D=3.7e-16, rw=0.0, Dinv=1.9e-14, sol=1.6e-16)


def make_case(pkg):
    return helpers.wetgas_case(pkg, 3, 3, 70, heterogeneous=True, dz=1.0)


def rel(a, b):
    a, b = np.asarray(a, L), np.asarray(b, L)
    d, s = np.abs(a - b), np.maximum(np.abs(a), np.abs(b))
    m = s > 0
    return float((d[m] / s[m]).max()) if m.any() else 0.0


def rel_rows(a, b):
    a, b = np.asarray(a, L), np.asarray(b, L)
    return float((np.abs(a - b) / np.abs(a).max(axis=-1, keepdims=True)).max())


@pytest.fixture(scope="module")
def setup(pkg, orc):
    case = make_case(pkg)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq().copy()
    assert iq.shape[1] == 19
    ws = wells_at(pkg, dict(case=case), None)
    ws.calculate_explicit_quantities(iq)
    ws.solve_well_equations(iq)
    ws.update_well_controls()
    assert [w.control[0] for w in ws.wells] == ["rate", "orat", "rate"]          # PCAP: its vaporised oil exceeds the ORAT limit
    x = ws.x.copy()
    x[:, :3] *= 1.05
    x[0, 3] = float(np.median(iq[ws.cells[:70], 4, 0] - ws.head[:70]))
    return dict(case=case, iq=iq, x=x, head=ws.head.copy(), controls=[w.control for w in ws.wells])


def wells_at(pkg, s, x, arithmetic="stated", vaporised_oil=True, crossflow=True):
    """the wells of the module's text in the state x (None: a fresh list)"""
    ws = pkg.wells.StandardWells(pkg.decks.gas_condensate_wells(s["case"], allow_crossflow=crossflow), s["case"]["depth"], arithmetic=arithmetic,
                                 vaporised_oil=vaporised_oil)
    if x is not None:
        ws.head, ws.x, ws.initialised = s["head"].copy(), x.copy(), True
        for w, c in zip(ws.wells, s["controls"]):
            w.control = c
    return ws


# ---- the np.longdouble restatement: dual numbers of 8 entries (value, d/dSw, d/dp, d/dX, d/dbhp, d/dq_o, d/dq_w, d/dq_g) written out --------
def dual(v=0.0, d=()):
    a = np.zeros(8, L)
    a[0] = L(v)
    for i, x in d:
        a[i] = L(x)
    return a


def mul(a, b):
    o = a[0] * b + b[0] * a
    o[0] = a[0] * b[0]
    return o


def div(a, b):
    o = (a - (a[0] / b[0]) * b) / b[0]
    o[0] = a[0] / b[0]
    return o


def longdouble_wells(W, ws, iq):
    """the issue's formulas, one perforation at a time -> rates (nperf, 3, 5), dq (nperf, 3, 3), B, C (nperf, 4, 3), D (nw, 4, 4), r_w (nw, 4),
    solution rates (nw, 2); the control rows are the module's own (they do not hold the rate model)"""
    OIL, WATER, GAS, PH_W, PH_O, PH_G = W.OIL, W.WATER, W.GAS, W.PH_W, W.PH_O, W.PH_G
    n, nw = len(ws.cells), ws.nw
    rates, dq, sol = np.zeros((n, 3, 5), L), np.zeros((n, 3, 3), L), np.zeros((n, 2), L)
    for k, w in enumerate(ws.wells):
        x = [L(v) for v in ws.x[k]]
        neg = [x[c] < 0 for c in range(3)]
        pc = [-x[c] if neg[c] else L(0) for c in range(3)]
        P = (pc[OIL] + pc[WATER]) + pc[GAS]
        cmix = None
        if w.allow_crossflow and P > 0:
            cmix = [dual(pc[c] / P, [(5 + j, -(((1 if c == j else 0) - pc[c] / P) / P)) for j in range(3) if neg[j]]) for c in range(3)]
        for p in range(ws.vp[k], ws.vp[k + 1]):
            rec = np.asarray(iq[ws.cells[p]], L)
            f = lambda field: dual(rec[field, 0], [(1, rec[field, 1]), (2, rec[field, 2]), (3, rec[field, 3])])
            tw = L(ws.tw[p])
            dd = f(W.F_P + PH_O)
            dd[0] = dd[0] - (x[3] + L(ws.head[p]))
            dd[4] = L(-1)
            b, mob, rs, rv = [f(W.F_B + ph) for ph in range(3)], [f(W.F_MOB + ph) for ph in range(3)], f(W.F_RS), f(W.F_RV)
            r = [dual(), dual(), dual()]
            if w.producer and dd[0] > 0:
                surf = [mul(b[ph], -tw * mul(mob[ph], dd)) for ph in range(3)]
                dis, vap = mul(rs, surf[PH_O]), mul(rv, surf[PH_G])
                r[OIL], r[GAS], r[WATER] = surf[PH_O] + vap, surf[PH_G] + dis, surf[PH_W]
                sol[p] = dis[0], vap[0]
            elif not w.producer and dd[0] < 0:
                ph = W.PHASE_BY_NAME[w.inj_phase]
                r[W.COMPONENT_OF_PHASE[ph]] = mul(b[ph], -tw * mul((mob[0] + mob[1]) + mob[2], dd))
            elif w.producer and cmix is not None:
                d = dual(1.0) - mul(rv, rs)
                tmp_oil = div(cmix[OIL] - mul(rv, cmix[GAS]), d)
                tmp_gas = div(cmix[GAS] - mul(rs, cmix[OIL]), d)
                ratio = (div(cmix[WATER], b[PH_W]) + div(tmp_oil, b[PH_O])) + div(tmp_gas, b[PH_G])
                if d[0] > 0 and ratio[0] > 0:
                    cqt_is = div(-tw * mul((mob[PH_W] + mob[PH_O]) + mob[PH_G], dd), ratio)
                    r = [mul(cmix[c], cqt_is) for c in range(3)]
                    sol[p, 1] = rv[0] * (r[GAS][0] - rs[0] * r[OIL][0]) / d[0]
                    sol[p, 0] = rs[0] * (r[OIL][0] - rv[0] * r[GAS][0]) / d[0]
            for c in range(3):
                rates[p, c], dq[p, c] = r[c][:5], r[c][5:]
    rw, D = np.zeros((nw, 4), L), np.zeros((nw, 4, 4), L)
    B, C = np.zeros((n, 4, 3), L), np.zeros((n, 4, 3), L)
    solw = np.zeros((nw, 2), L)
    cr, cg = ws._control_rows()
    for k in range(nw):
        lo, hi = ws.vp[k], ws.vp[k + 1]
        for c in range(3):
            rw[k, c] = L(ws.x[k, c]) - rates[lo:hi, c, 0].sum()
            D[k, c, 3] = -rates[lo:hi, c, 4].sum()
            for j in range(3):
                D[k, c, j] = (1 if c == j else 0) - dq[lo:hi, c, j].sum()
        rw[k, 3], D[k, 3] = cr[k], cg[k]
        solw[k] = sol[lo:hi].sum(axis=0)
    B[:, :3, :] = -rates[:, :, 1:4]
    C[:, 3, :] = -rates[:, :, 4]
    C[:, :3, :] = -dq.transpose(0, 2, 1)
    return dict(rates=rates, dq=dq, B=B, C=C, D=D, rw=rw, sol=solw)


def module_form(ws, iq):
    r, D, B, C, src, dsrc = ws._assemble_wells(iq)
    dis, vap = ws.solution_rates()
    return dict(rates=ws._perf_rates(iq, ws.x[:, 3]), dq=ws.rate_dq.copy(), B=B, C=C, D=D, rw=r, sol=np.stack([dis, vap], axis=1),
                Dinv=np.array([np.linalg.inv(d) for d in D]))


def differences(a, b, keys):
    return {k: (rel_rows if k == "Dinv" else rel)(a[k], b[k]) for k in keys}


def check(name, measured, got):
    print(name, "measured: " + "   ".join("%s %.2e" % kv for kv in got.items()))
    for k, v in got.items():
        assert v <= 100.0 * measured[k], (name, k, v, measured[k])


# ---- 1. the formula -----------------------------------------------------------------------------------------------------------------------
def test_stated_form_against_the_longdouble_restatement(pkg, setup):
    ws = wells_at(pkg, setup, setup["x"])
    got = module_form(ws, setup["iq"])
    want = longdouble_wells(pkg.wells, ws, setup["iq"])
    long_rates = got["rates"][:70, :, 0]
    reversed_ = (long_rates > 0.0).any(axis=1)
    assert 20 <= reversed_.sum() <= 50 and reversed_[:21].any() and reversed_[21:35].any() and reversed_[35:].any()      # in all three zones
    assert np.all(got["sol"][0] < 0.0) and got["sol"][1, 0] == 0.0 and got["sol"][1, 1] < 0.0 and np.all(got["sol"][2] == 0.0)   # PCAP has no oil phase to dissolve gas in; the injector: zeros
    assert np.any(got["dq"][:70] != 0.0)
    check("stated against longdouble", MEASURED_FORMULA, differences(got, want, MEASURED_FORMULA))


# ---- 2. the two arithmetics ---------------------------------------------------------------------------------------------------------------
def test_numpy_form_against_stated(pkg, setup):
    a = module_form(wells_at(pkg, setup, setup["x"], "numpy"), setup["iq"])
    b = module_form(wells_at(pkg, setup, setup["x"], "stated"), setup["iq"])
    check("numpy against stated", MEASURED_NUMPY, differences(a, b, MEASURED_NUMPY))


# ---- 3. what the switch adds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arithmetic", ["stated", "numpy"])
def test_gas_cap_perforation_gains_rv_times_the_gas_rate(pkg, setup, arithmetic):
    """PCAP's completion: meaning 2 (no oil phase: surf_o is a zero), Rv > 0, mobile gas - the oil rate with the switch is the rate without
    it plus rv * surf_g, to the bit, value and derivatives"""
    W = pkg.wells
    case, iq = setup["case"], setup["iq"]
    on, off = (wells_at(pkg, setup, setup["x"], arithmetic, vaporised_oil=v) for v in (True, False))
    p = 70
    c = on.cells[p]
    assert case["meaning"][c] == 2 and iq[c, W.F_RV, 0] > 0.0 and iq[c, W.F_MOB + W.PH_G, 0] > 0.0 and iq[c, W.F_S + W.PH_O, 0] == 0.0
    r_on, r_off = on._perf_rates(iq, on.x[:, 3])[p], off._perf_rates(iq, off.x[:, 3])[p]
    ad = lambda f: np.concatenate([iq[c, f, :], [0.0]])
    dd = ad(W.F_P + W.PH_O)
    dd[0] -= on.x[1, 3] + on.head[p]
    dd[4] = -1.0
    assert dd[0] > 0.0

    def mul5(a, b):
        return np.concatenate([[a[0] * b[0]], a[0] * b[1:] + b[0] * a[1:]])
    surf_g = mul5(ad(W.F_B + W.PH_G), -on.tw[p] * mul5(ad(W.F_MOB + W.PH_G), dd))
    vap = mul5(ad(W.F_RV), surf_g)
    assert vap[0] < 0.0 and np.all(r_off[W.OIL] == 0.0)
    assert np.array_equal(r_on[W.OIL] - r_off[W.OIL], vap)
    assert np.array_equal(r_on[W.WATER], r_off[W.WATER]) and np.array_equal(r_on[W.GAS], r_off[W.GAS])
    on._assemble_wells(iq)
    off._assemble_wells(iq)
    assert on.solution_rates()[1][1] == vap[0] and np.all(np.concatenate(off.solution_rates()) == 0.0)
    # the cell's oil row gets its sink, and the ORAT limit sees the oil
    assert on.assemble(iq)["source_cells"].reshape(-1, 3)[list(on.ucells).index(c), W.OIL] == r_on[W.OIL, 0] < 0.0


def test_switch_off_is_the_dry_gas_model(pkg, setup):
    """the default computes what it computed: no argument and vaporised_oil=False give the same arrays, and PCAP reports no oil"""
    iq = setup["iq"]
    ws0 = pkg.wells.StandardWells(pkg.decks.gas_condensate_wells(setup["case"], allow_crossflow=True), setup["case"]["depth"], arithmetic="stated")
    ws0.head, ws0.x, ws0.initialised = setup["head"].copy(), setup["x"].copy(), True
    ws1 = wells_at(pkg, setup, setup["x"], vaporised_oil=False)
    for ws in (ws0, ws1):        # (PCAP back under its gas target: without the switch no oil rate answers to an ORAT row)
        for w in ws.wells:
            w.control = w.rate_control
    a, b = module_form(ws0, iq), module_form(ws1, iq)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.all(a["rates"][70, pkg.wells.OIL] == 0.0) and np.all(a["sol"] == 0.0)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_a_17_field_record_is_refused(pkg, orc):
    case = pkg.decks.cartesian_case(3, 3, 70, state="mixed", heterogeneous=True, dz=1.0)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    assert iq.shape[1] == 17
    ws = pkg.wells.StandardWells(pkg.decks.gas_condensate_wells(case), case["depth"], arithmetic="stated", vaporised_oil=True)
    with pytest.raises(ValueError, match="19-field"):
        ws.solve_well_equations(iq)
    with pytest.raises(ValueError, match="19-field"):
        ws.assemble(iq)
    off = pkg.wells.StandardWells(pkg.decks.gas_condensate_wells(case), case["depth"], arithmetic="stated")
    off.solve_well_equations(iq)                                                     # (the default takes the record as before)
    assert np.all(np.concatenate(off.solution_rates()) == 0.0)

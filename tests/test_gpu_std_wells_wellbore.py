"""The heads from the well-bore density on the device (opmhip_set_std_wells_head_model, k_std_wells_wellbore) against
wells.StandardWells(head_model="wellbore", arithmetic="stated") over the device's own property functions (capi.HipFluid), bit for bit:
same operations in the same order, IEEE division / fabs / min, no contraction, probes equal to the bit (tests/test_gpu_equil.py).

Grid of the small tests: 2 x 2 x 70 (cell = i + 2 (j + 2 k)).  Column (0, 0): a 70-completion producer; (1, 0): a 65-completion water
injector - both longer than one pass of lanes, the carries cross the boundary at 64 upwards (the flow) and downwards (x, the head);
(0, 1): a three-completion gas injector, a three-completion water injector; (1, 1): a one-completion producer, two producers that share
a cell, a producer whose middle completion is closed and one whose bottom two are; (0, 1) again: a producer on a gas target across
the gas-oil contact.  (The wet-gas case has no oil phase in its top 21 layers.)"""
import numpy as np
import pytest

import helpers
import std_wells_harness as H
from std_wells_harness import moved, same

pytestmark = pytest.mark.gpu

DAY = 86400.0
WB = ("density", "p_avg", "mixture")


def make_case(pkg, wet):
    if wet:
        return helpers.wetgas_case(pkg, 2, 2, 70, heterogeneous=True, dz=1.0)
    return pkg.decks.cartesian_case(2, 2, 70, state="mixed", heterogeneous=True, dz=1.0)


column = H.column(2, 2)


def make_wells(pkg, case, shared=True):
    W = pkg.wells

    def well(name, cells, producer, control, limit, inj=None, tw=None, ref=None, **kw):
        if tw is None:
            tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return W.Well(name, cells, tw, case["depth"][cells[0]] - 1.5 if ref is None else ref, producer, control, limit, inj_phase=inj, **kw)
    tw3 = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in column(1, 1, [30, 31, 32])]
    out = [well("P70", column(0, 0, range(70)), True, ("rate", W.OIL, 30.0 / DAY), 150e5),
           well("W65", column(1, 0, range(65)), False, ("rate", W.WATER, 60.0 / DAY), 400e5, "water"),
           well("G3", column(0, 1, [0, 1, 2]), False, ("rate", W.GAS, 5000.0 / DAY), 400e5, "gas"),
           well("W3", column(0, 1, [40, 41, 42]), False, ("rate", W.WATER, 5.0 / DAY), 400e5, "water"),
           well("P1", column(1, 1, [50]), True, ("rate", W.OIL, 2.0 / DAY), 150e5, ref=case["depth"][column(1, 1, [50])[0]] - 11.5, preferred_phase="water"),
           well("CM", column(1, 1, [30, 31, 32]), True, ("rate", W.OIL, 2.0 / DAY), 150e5, tw=[tw3[0], 0.0, tw3[2]]),
           well("CB", column(1, 1, [22, 23, 24]), True, ("rate", W.OIL, 1.0 / DAY), 150e5, tw=[tw3[1], 0.0, 0.0], preferred_phase="gas"),
           well("GV", column(0, 1, [18, 19, 20, 21, 22]), True, ("rate", W.GAS, 20000.0 / DAY), 150e5)]      # gas with a little oil from its lowest completions
    if shared:
        out += [well("SA", column(1, 1, [25, 26, 27]), True, ("rate", W.OIL, 3.0 / DAY), 150e5),
                well("SB", column(1, 1, [27, 28]), True, ("rate", W.WATER, 0.5 / DAY), 150e5)]
    return out


def compare_heads(md, wh, what):
    """after begin_iteration(0): density, p_avg, mixture, head.  (Local: there is no assembly yet, and the harness's compare_wells always
    compares what an assembly leaves)"""
    wb, blk = md.std_wells_wellbore(), md.std_wells_blocks()
    for k in WB:
        same(wb[k], wh.wellbore[k], (what, k))
    same(blk["head"], wh.head, (what, "head"))
    assert np.all(np.isfinite(blk["head"])) and np.all(wb["density"] > 10.0) and np.all(wb["density"] < 1200.0)
    return wb, blk


# ---- 1. heads and one assembly, dry and wet gas ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wet", [False, True])
def test_heads_and_assembly(pkg, wet):
    case = make_case(pkg, wet)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case), head_model="wellbore", props="wellbore")
    W = pkg.wells
    assert md.iq().shape[1] == (19 if wet else 17) and list(np.diff(wh.vp)) == [70, 65, 3, 3, 1, 3, 3, 5, 3, 2]
    dt = 5.0 * DAY
    # the first time step: every well at rest
    wh.calculate_explicit_quantities(wh.records(mh))
    md.std_wells_begin_iteration(0)
    wb, blk = compare_heads(md, wh, "rest")
    vp, mix = wh.vp, wb["mixture"]
    rho = case["fluid"].pvt[0]["density"]
    props = pkg.capi.HipFluid(case["fluid"])
    # (a) the water injector at rest: water at the mean pressure in every segment, the heads their running sum
    s = slice(vp[3], vp[4])
    bw = props.probe(wb["p_avg"][s])[:, 0]
    dens = np.array([rho[1] / (1.0 / b) for b in bw])
    z, ref = case["depth"][wh.cells[s]], wh.wells[3].ref_depth
    dp = [(z[0] - ref) * dens[0] * W.GRAVITY, (z[1] - z[0]) * dens[1] * W.GRAVITY, (z[2] - z[1]) * dens[2] * W.GRAVITY]
    same(wb["density"][s], dens, "a density")
    same(blk["head"][s], [dp[0], dp[0] + dp[1], (dp[0] + dp[1]) + dp[2]], "a head")
    same(mix[s], [[0.0, 1.0, 0.0]] * 3, "a mixture")
    # (b) producers at rest take the mobility ratio: three components where three phases are mobile
    assert np.all(mix[vp[0]:vp[0] + 20] > 0.0) and np.allclose(mix[vp[0]:vp[1]].sum(axis=1), 1.0, rtol=1e-14)
    # (c) a closed completion passes the flow from below on; below the last open one x - not mix - is handed down
    assert np.array_equal(mix[vp[5] + 1], mix[vp[5] + 2]) and not np.array_equal(mix[vp[5]], mix[vp[5] + 1])
    same(mix[vp[6] + 1], wh.wellbore["x"][vp[6]], "c x")
    same(mix[vp[6] + 2], wh.wellbore["x"][vp[6] + 1], "c x")
    # (d) one completion: (perf_depth - ref_depth) * density * g and nothing else
    p = vp[4]
    assert blk["head"][p] == (case["depth"][wh.cells[p]] - wh.wells[4].ref_depth) * wb["density"][p] * W.GRAVITY
    # the carries cross 64 in both directions: the head still grows, the flow of the last completions arrives at the first
    assert np.all(np.diff(blk["head"][vp[0]:vp[1]]) > 0.0) and np.all(np.diff(blk["head"][vp[1]:vp[2]]) > 0.0)
    # ... then the wells alone, the controls and two assemblies
    wh.solve_well_equations(wh.records(mh))
    for it, state in ((0, None), (1, moved(case, 3))):
        if state is not None:
            for m in (md, mh):
                m.set_state(state, case["meaning"])
        iq = wh.records(mh)
        wh.update_well_controls()
        wa = wh.assemble(iq)
        mh.set_source_cells(wa["cells"], wa["source_cells"], wa["dsource_cells"])
        jh, rh = mh.assemble(dt, it)
        if it > 0:
            wd.begin_iteration(it)
        jd, rd = md.assemble(dt, it)
        blk = H.compare_wells(pkg, md, wh, wa, it, extra=("D", "source", "wellbore"), iq=iq)
        assert np.array_equal(jd, jh) and np.array_equal(rd, rh), it
    assert np.count_nonzero(blk["perf_rates"]) > 50 and np.all(np.isfinite(blk["Dinv"]))
    # the next time step starts from flowing wells: the general branch - the flow summed from below, the rs / rv corrections
    wh.calculate_explicit_quantities(wh.records(mh))
    md.std_wells_begin_iteration(0)
    wb, blk = compare_heads(md, wh, "flowing")
    m_, b_ = wh.wellbore["mixture"], wh.wellbore
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rs_binds = (m_[:, W.OIL] > 1e-12) & (m_[:, W.GAS] / m_[:, W.OIL] > b_["rsmax"])
        rs_free = (m_[:, W.OIL] > 1e-12) & (m_[:, W.GAS] > 0.0) & (m_[:, W.GAS] / m_[:, W.OIL] < b_["rsmax"])
        rv_binds = (m_[:, W.GAS] > 1e-12) & (m_[:, W.OIL] / m_[:, W.GAS] > b_["rvmax"])
        rv_free = (m_[:, W.GAS] > 1e-12) & (m_[:, W.OIL] > 0.0) & (m_[:, W.OIL] / m_[:, W.GAS] < b_["rvmax"])
    print("wet" if wet else "dry", "rs min binds / does not:", rs_binds.sum(), rs_free.sum(), " rv min binds / does not:", rv_binds.sum(), rv_free.sum())
    assert rs_binds.any() and rs_free.any()
    if wet:       # (a producing well's oil share is always above the saturated Rv here; tests_perf_state_handed_in has the other branch)
        assert rv_binds.any() and np.all(b_["rvmax"] > 0.0)
    else:
        assert np.all(b_["rvmax"] == 0.0)
    wh.solve_well_equations(wh.records(mh))
    iq = wh.records(mh)
    wh.update_well_controls()
    wa = wh.assemble(iq)
    md.assemble(dt, 0, fetch=False)
    H.compare_wells(pkg, md, wh, wa, "second step", extra=("D", "source", "wellbore"), iq=iq)


# ---- 2. the perforation state handed in ------------------------------------------------------------------------------------------------------
def handed_in_state(pkg, wh):
    """a well state no run would leave, to reach every branch: wells without an oil rate, without a gas rate, without any; a perforation
    in three without flow; in the gas producer a trace of oil in much gas (below the saturated Rv: its min() does not bind)"""
    W = pkg.wells
    rng = np.random.default_rng(5)
    n = len(wh.cells)
    pp = 250e5 + 1e5 * rng.uniform(-1.0, 1.0, n)
    rates = rng.uniform(-1e-4, 1e-4, (n, 3)) * (rng.uniform(0.0, 1.0, (n, 1)) > 0.3)
    rates[wh.vp[1]:wh.vp[2]] = np.abs(rates[wh.vp[1]:wh.vp[2]]) * [0.0, 1.0, 0.0]
    gv = slice(wh.vp[7], wh.vp[8])
    rates[gv] = -rng.uniform(0.5, 1.0, (5, 1)) * [1e-6, 1e-9, 0.1]
    x = np.zeros((wh.nw, 4))
    x[:, :3] = rng.uniform(-1e-3, 1e-3, (wh.nw, 3))
    x[2, :3] = 0.0                                       # a well without rates: the saturated curves
    x[3, W.GAS] = 0.0                                    # no gas rate: rv = 0, 1/B_o on the saturated curve
    x[4, W.OIL] = 0.0                                    # no oil rate: rs = 0, 1/B_g on the saturated curve
    x[7, :3] = [-1e-6, -1e-9, -0.1]                      # |q_o| / |q_g| below the saturated Rv
    x[5, :3] = [-1e-3, -1e-5, -1e-3 * 50.0]              # |q_g| / |q_o| below the saturated Rs
    x[:, 3] = 250e5
    return x, pp, rates


def test_perf_state_handed_in(pkg):
    """wet gas; opmhip_set_std_wells_perf_state and the read-back; the rv min() binds in some perforations and not in others"""
    case = make_case(pkg, True)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case, shared=False), head_model="wellbore", props="wellbore")
    W = pkg.wells
    x, pp, rates = handed_in_state(pkg, wh)
    st_none = wd.state()
    assert st_none[2][0] is None and not md.std_wells_wellbore()["perf_state_set"]
    wd.set_state((x, [w.control for w in wd.wells], (pp, rates)))
    wh.set_state((x, [w.control for w in wh.wells], (pp, rates)))
    assert md.std_wells_wellbore()["perf_state_set"]
    wb = md.std_wells_wellbore()
    same(wb["perf_pressure"], pp, "pp")
    same(wb["perf_rates"], rates, "rates")
    st = wd.state()
    same(st[0], x, "state x")
    same(st[2][0], pp, "state pp")
    same(st[2][1], rates, "state rates")
    md.std_wells_begin_iteration(0)                       # (the first ever: the bottom-hole pressures start from the cells on both sides)
    wh.calculate_explicit_quantities(wh.records(mh))
    compare_heads(md, wh, "handed in")
    m_, b_ = wh.wellbore["mixture"], wh.wellbore
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rv_binds = (m_[:, W.GAS] > 1e-12) & (m_[:, W.OIL] / m_[:, W.GAS] > b_["rvmax"])
        rv_free = (m_[:, W.GAS] > 1e-12) & (m_[:, W.OIL] > 0.0) & (m_[:, W.OIL] / m_[:, W.GAS] < b_["rvmax"])
        rs_binds = (m_[:, W.OIL] > 1e-12) & (m_[:, W.GAS] / m_[:, W.OIL] > b_["rsmax"])
        rs_free = (m_[:, W.OIL] > 1e-12) & (m_[:, W.GAS] > 0.0) & (m_[:, W.GAS] / m_[:, W.OIL] < b_["rsmax"])
    print("handed in: rv min binds / does not:", rv_binds.sum(), rv_free.sum(), " rs:", rs_binds.sum(), rs_free.sum())
    assert rv_binds.any() and rv_free.any() and rs_binds.any() and rs_free.any()
    assert np.any(np.abs(rates).sum(axis=1) == 0.0)
    with pytest.raises(ValueError):
        md.set_std_wells_perf_state(pp[:-1])
    # a state from before the first heads takes the pressures away again: the next begin_iteration(0) takes them from the cells
    wd.set_state(st_none)
    assert not md.std_wells_wellbore()["perf_state_set"] and wd.state()[2][0] is None
    md.set_std_wells_perf_state()                        # nothing handed in: nothing changes
    assert not md.std_wells_wellbore()["perf_state_set"]
    with pytest.raises(pkg.capi.OpmHipError) as e:
        md.set_std_wells_perf_state(None, rates)         # rates alone while no pressures exist
    assert e.value.code == pkg.capi.INVALID_ARGUMENT
    md.std_wells_begin_iteration(0)
    po = md.iq_cells(wh.cells)[:, W.F_P + W.PH_O, 0]
    second = np.array([wh.vp[k] + 1 for k in range(wh.nw) if wh.vp[k + 1] - wh.vp[k] > 1])
    assert md.std_wells_wellbore()["perf_state_set"] and np.array_equal(md.std_wells_wellbore()["p_avg"][second], (po[second] + po[second - 1]) / 2)


# ---- 3. schedule ------------------------------------------------------------------------------------------------------------------------------
def run_schedule(pkg, m, wells, schedule, device):
    model = pkg.newton.BlackoilModelHip(m, well_model=wells)
    ts = pkg.newton.AdaptiveTimeStepping(model, pkg.newton.TimeSteppingParameters(initial_dt=DAY))
    trail = []
    inner = model.nonlinear_iteration

    def recorded(iteration, dt):
        rep = inner(iteration, dt)
        x = wells.fetch().copy() if device else wells.x.copy()
        head = m.std_wells_blocks()["head"] if device else wells.head.copy()
        trail.append((x, "".join("R" if w.control[0] == "rate" else "B" for w in wells.wells), head))
        return rep
    model.nonlinear_iteration = recorded
    for length, rate in schedule:
        if rate is not None:
            for k in range(1, wells.nw):
                wells.set_rate_target(k, rate * pkg.decks.STB_PER_DAY)
        ts.advance_report_step(length)
    return ts, trail


def test_spe9_shaped_schedule(pkg):
    """two short report steps with the rate-target event between them, under the conditions of
    tests/test_gpu_std_wells_device.py::test_spe9_shaped_schedule (no cell shared by two wells): device and host-stated form agree after
    every Newton iteration in x, the controls and the heads, and in the reservoir state at the end; against the same run under
    head_model="cell_oil" the water injector's heads differ by far more than rounding"""
    from test_spe9_shaped_wells import PRODUCER_BHP_LIMIT
    case = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
    schedule = ((2 * DAY, None), (2 * DAY, 100.0))
    props = pkg.capi.HipFluid(case["fluid"])
    runs = {}
    for form in ("device", "host", "cell_oil"):
        m = pkg.capi.HipModel(case, tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
        m.set_state(case["pv"], case["meaning"])
        wl = pkg.decks.spe9_shaped_wells(case, producer_bhp_limit=PRODUCER_BHP_LIMIT).wells
        if form == "host":
            w = pkg.wells.StandardWells(wl, case["depth"], arithmetic="stated", head_model="wellbore", props=props)
        else:
            w = pkg.wells.DeviceStandardWells(wl, case["depth"], m, head_model="wellbore" if form == "device" else "cell_oil")
        ts, trail = run_schedule(pkg, m, w, schedule, form != "host")
        runs[form] = dict(ts=ts, trail=trail, m=m)
    dev, host, oil = runs["device"], runs["host"], runs["cell_oil"]
    assert dev["ts"].history == host["ts"].history and len(dev["trail"]) == len(host["trail"]) >= 6
    assert abs(dev["ts"].time - 4 * DAY) < 1.0 and len(dev["ts"].history) >= 3
    for n, ((xd, cd, hd), (xh, ch, hh)) in enumerate(zip(dev["trail"], host["trail"])):
        assert cd == ch, n
        same(xd, xh, ("x", n))
        same(hd, hh, ("head", n))
    (pd, md_), (ph, mh_) = dev["m"].get_state(), host["m"].get_state()
    assert np.array_equal(pd, ph) and np.array_equal(md_, mh_)
    # the model is in force: an injector full of water weighs far more than the oil of its cells
    hw, ho = dev["trail"][-1][2][:5], oil["trail"][-1][2][:5]
    assert np.all(hw[1:] > 1.2 * ho[1:]) and np.all(ho[1:] > 0.0), (hw, ho)


# ---- 4. chopped step -----------------------------------------------------------------------------------------------------------------------
def test_chopped_step(pkg):
    """update_failed restores the perforation pressures and the stored rates: the next begin_iteration(0) yields the heads of a context
    that never tried the failed step"""
    case = make_case(pkg, False)
    ctx = []
    for _ in range(2):
        m = pkg.capi.HipModel(case, tolerance=1e-4)
        m.set_state(case["pv"], case["meaning"])
        w = pkg.wells.DeviceStandardWells(make_wells(pkg, case, shared=False), case["depth"], m, head_model="wellbore")
        ctx.append((m, w))

    def iterations(m, w, dt, n):
        for it in range(n):
            w.begin_iteration(it)
            m.assemble(dt, it, fetch=False)
            m.std_wells_apply_residual()
            m.solve_jacobian_system()
            m.update(None, 1.0)
            w.update(1.0)
        w.begin_iteration(n)
        m.assemble(dt, n, fetch=False)
    (ma, wa), (mb, wb) = ctx
    for m, w in ctx:                                      # (a first step given up on both: test_first_step_given_up looks at what follows it)
        m.advance_time_level()
        iterations(m, w, 5.0 * DAY, 1)
        m.update_failed()
    for m, w in ctx:                                      # an accepted step on both
        iterations(m, w, DAY, 2)
        m.advance_time_level()
    ref = mb.std_wells_wellbore()
    for k in ("perf_pressure", "perf_rates"):
        same(ma.std_wells_wellbore()[k], ref[k], ("accepted", k))
    xa = ma.get_std_wells()[0]
    iterations(ma, wa, 10.0 * DAY, 2)                     # the step the caller gives up
    tried = ma.std_wells_wellbore()
    assert not np.array_equal(tried["perf_pressure"], ref["perf_pressure"]) and not np.array_equal(tried["perf_rates"], ref["perf_rates"])
    ma.update_failed()
    for k in ("perf_pressure", "perf_rates"):
        same(ma.std_wells_wellbore()[k], ref[k], ("restored", k))
    same(ma.get_std_wells()[0], xa, "x restored")
    for m, w in ctx:
        w.begin_iteration(0)
    ga, gb = ma.std_wells_wellbore(), mb.std_wells_wellbore()
    for k in WB:
        same(ga[k], gb[k], ("after the failure", k))
    same(ma.std_wells_blocks()["head"], mb.std_wells_blocks()["head"], "heads after the failure")
    # (they are also the given-up step's own: it had started from the same well state - what the restore brought back)
    same(ga["density"], tried["density"], "the given-up step's start")
    # ... and not those of the well state the given-up step left behind
    ma.set_std_wells_state(x=mb.get_std_wells()[0])
    ma.set_std_wells_perf_state(tried["perf_pressure"], tried["perf_rates"])
    for m, w in ctx:
        w.begin_iteration(0)
    assert not np.array_equal(ma.std_wells_blocks()["head"], mb.std_wells_blocks()["head"])


def test_first_step_given_up(pkg):
    """newton.AdaptiveTimeStepping's order of calls - advance_time_level, the iterations, update_failed - on the very first time step: the
    retry's begin_iteration(0) yields the density, p_avg, heads and well unknowns of a context that never tried the step - the perforation
    pressures and the bottom-hole pressures from the cells again, not the zeros the roll-back of x alone would leave - on the device and
    in the host form"""
    case = make_case(pkg, False)
    props = pkg.capi.HipFluid(case["fluid"])
    wells = lambda: make_wells(pkg, case, shared=False)
    got = []
    for tried in (True, False):
        m = pkg.capi.HipModel(case, tolerance=1e-4)
        m.set_state(case["pv"], case["meaning"])
        w = pkg.wells.DeviceStandardWells(wells(), case["depth"], m, head_model="wellbore")
        m.advance_time_level()
        if tried:
            w.begin_iteration(0)
            m.assemble(5.0 * DAY, 0, fetch=False)
            m.std_wells_apply_residual()
            m.solve_jacobian_system()
            m.update(None, 1.0)
            w.update(1.0)
            w.begin_iteration(1)
            m.assemble(5.0 * DAY, 1, fetch=False)
            assert m.std_wells_wellbore()["perf_state_set"] and np.any(m.std_wells_wellbore()["perf_rates"] != 0.0)
            m.update_failed()
            assert not m.std_wells_wellbore()["perf_state_set"] and np.all(m.get_std_wells()[0] == 0.0)
        w.begin_iteration(0)
        got.append((m.std_wells_wellbore(), m.std_wells_blocks()["head"], m.get_std_wells()[0]))
    (wa, ha, xa), (wf, hf, xf) = got
    for k in WB + ("perf_pressure", "perf_rates"):
        same(wa[k], wf[k], ("retry against fresh", k))
    same(ha, hf, "heads")
    same(xa, xf, "x")
    assert np.all(wa["p_avg"] > 200e5) and np.all(xa[:, 3] > 200e5)          # no segment at half pressure
    # the host form, through state() / set_state() as newton.BlackoilModelHip rolls it back
    mh = pkg.capi.HipModel(case)
    mh.set_state(case["pv"], case["meaning"])
    wh = pkg.wells.StandardWells(wells(), case["depth"], arithmetic="stated", head_model="wellbore", props=props)
    saved = wh.state()
    iq = H.host_begin(mh, wh, 0)
    wh.assemble(iq)
    assert wh.initialised and np.any(wh.perf_rates != 0.0)
    wh.set_state(saved)
    assert not wh.initialised
    wh.calculate_explicit_quantities(iq)
    for k in WB:
        same(wh.wellbore[k], wf[k], ("host retry against the fresh device context", k))
    same(wh.head, hf, "host heads")


# ---- 4b. two PVT regions --------------------------------------------------------------------------------------------------------------------
def two_region_case(pkg):
    """the 2 x 2 x 70 column with a second PVT region - heavier surface densities, another water - in every other layer"""
    fl = pkg.fluid.spe1_fluid()[0]
    r1 = dict(fl.pvt[0])
    r1["density"] = [1.06 * fl.pvt[0]["density"][0], 1.03 * fl.pvt[0]["density"][1], 1.2 * fl.pvt[0]["density"][2]]
    r1["pvtw"] = [fl.pvt[0]["pvtw"][0], 1.04 * fl.pvt[0]["pvtw"][1], 1.5 * fl.pvt[0]["pvtw"][2]] + list(fl.pvt[0]["pvtw"][3:])
    fl2 = pkg.fluid.Fluid([fl.pvt[0], r1], fl.sat, rock_pref=fl.rock_pref, rock_cr=fl.rock_cr)
    case = pkg.decks.cartesian_case(2, 2, 70, state="mixed", heterogeneous=True, dz=1.0, fluid=fl2)
    case["pvtnum"] = ((np.arange(case["Nb"]) // 4) % 2).astype(np.int32)
    return case


def test_two_pvt_regions(pkg):
    """the PVT region and the surface densities are the perforated cell's: device against host-stated form, and against the numbers a
    single region would give"""
    case = two_region_case(pkg)
    props = pkg.capi.HipFluid(case["fluid"])
    md = pkg.capi.HipModel(case)
    mh = pkg.capi.HipModel(case)
    for m in (md, mh):
        m.set_state(case["pv"], case["meaning"])
    wd = pkg.wells.DeviceStandardWells(make_wells(pkg, case), case["depth"], md, head_model="wellbore")
    wh = pkg.wells.StandardWells(make_wells(pkg, case), case["depth"], arithmetic="stated", head_model="wellbore", props=props, pvtnum=case["pvtnum"])
    one = pkg.wells.StandardWells(make_wells(pkg, case), case["depth"], arithmetic="stated", head_model="wellbore", props=props)
    assert set(wh.pvt_of_perf[:10]) == {0, 1} and np.all(one.pvt_of_perf == 0)
    wh.calculate_explicit_quantities(wh.records(mh))
    one.calculate_explicit_quantities(one.records(mh))
    md.std_wells_begin_iteration(0)
    wb, blk = compare_heads(md, wh, "rest, two regions")
    # the water injector at rest: the region's surface density over the region's 1/B_w, layer by layer
    s = slice(wh.vp[1], wh.vp[2])
    reg = case["pvtnum"][wh.cells[s]]
    bw = np.where(reg == 0, props.probe(wb["p_avg"][s], pvt_region=0)[:, 0], props.probe(wb["p_avg"][s], pvt_region=1)[:, 0])
    rho_w = np.array([case["fluid"].pvt[r]["density"][1] for r in reg])
    same(wb["density"][s], rho_w / (1.0 / bw), "water by region")
    odd = reg == 1
    assert odd.any() and (~odd).any() and np.all(wb["density"][s][odd] != one.wellbore["density"][s][odd]) and np.array_equal(wb["density"][s][~odd], one.wellbore["density"][s][~odd])
    # flowing wells
    wh.solve_well_equations(wh.records(mh))
    iq = wh.records(mh)
    wh.update_well_controls()
    wa = wh.assemble(iq)
    md.assemble(DAY, 0, fetch=False)
    H.compare_wells(pkg, md, wh, wa, "two regions", extra=("D", "source", "wellbore"), iq=iq)
    wh.calculate_explicit_quantities(wh.records(mh))
    md.std_wells_begin_iteration(0)
    compare_heads(md, wh, "flowing, two regions")


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    case = make_case(pkg, False)
    m = C.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    wells = dict(perf_pointers=[0, 2, 3], cell=[0, 4, 5], tw=[1e-12] * 3, dz=[0.0, 1.0, 0.0], producer=[1, 0], inj_phase=[0, 0], rate_component=[0, 1],
                 rate_target=[1e-4, 1e-4], bhp_limit=[150e5, 400e5], control=[0, 0], x=None)
    good = dict(perf_depth=case["depth"][[0, 4, 5]], ref_depth=[2499.0, 2500.0], preferred_phase=[1, 7])     # (an injector's preferred phase is not read)

    def refused(wb, code, word):
        s, keep = C.make_std_wells_wellbore(wb, 2, 3)
        rc = C.lib().opmhip_set_std_wells_head_model(m._h, s)
        msg = C.lib().opmhip_last_error(m._h).decode()
        assert rc == code and word in msg, (rc, msg)

    refused(good, C.NOT_READY, "no resident list")                       # before a list
    with pytest.raises(C.OpmHipError) as e:
        m.set_std_wells_perf_state(np.zeros(0))
    assert e.value.code == C.NOT_READY
    m.set_std_wells(wells)
    with pytest.raises(C.OpmHipError) as e:
        m.set_std_wells_perf_state(np.zeros(3))                          # a list, but not the model
    assert e.value.code == C.NOT_READY and "head model" in str(e.value)
    x0 = np.array([[0.0, 0.0, 0.0, 250e5], [0.0, 0.0, 0.0, 252e5]])
    pp0 = np.array([250e5, 250.3e5, 251e5])

    def heads(model):
        """the heads of one fixed well state"""
        m.set_std_wells_state(x=x0, control=[0, 0])
        if model:
            m.set_std_wells_perf_state(pp0, np.zeros((3, 3)))
        m.std_wells_begin_iteration(0)
        return m.std_wells_blocks()["head"]
    m.std_wells_begin_iteration(0)                                       # (the first ever: the bottom-hole pressures from the cells)
    oil_heads = heads(False)
    assert np.all(m.std_wells_wellbore()["density"] == 0.0)              # the getter is a no-op without the model
    m.set_std_wells_head_model(good)
    wb_heads = heads(True)
    assert not np.array_equal(wb_heads, oil_heads) and np.all(m.std_wells_wellbore()["density"] > 100.0)
    same(heads(True), wb_heads, "a function of the well state")
    # refused calls leave the model in force as it was
    refused(dict(good, preferred_phase=[3, 0]), C.INVALID_ARGUMENT, "unknown phase")
    refused(dict(good, preferred_phase=[-1, 0]), C.INVALID_ARGUMENT, "unknown phase")
    refused(dict(good, ref_depth=[np.nan, 2500.0]), C.INVALID_ARGUMENT, "not finite")
    for field in ("perf_depth", "ref_depth", "preferred_phase"):
        s, keep = C.make_std_wells_wellbore(good, 2, 3)
        setattr(s, field, None)
        assert C.lib().opmhip_set_std_wells_head_model(m._h, s) == C.INVALID_ARGUMENT and "null array" in C.lib().opmhip_last_error(m._h).decode()
    same(heads(True), wb_heads, "still in force")
    # NULL: back to the cell-oil head
    m.set_std_wells_head_model(None)
    same(heads(False), oil_heads, "cleared")
    # clearing or replacing the list clears the model
    m.set_std_wells_head_model(good)
    m.set_std_wells(None)
    refused(good, C.NOT_READY, "no resident list")
    m.set_std_wells(wells)
    same(heads(False), oil_heads, "a new list starts under the default model")
    with pytest.raises(C.OpmHipError) as e:
        m.set_std_wells_perf_state(np.zeros(3))
    assert e.value.code == C.NOT_READY


# ---- 6. without the model --------------------------------------------------------------------------------------------------------------------
def test_default_model_launches_and_computes_what_it_did(pkg):
    """a context that never called opmhip_set_std_wells_head_model against one that set the model and withdrew it: the launch counts of
    begin_iteration(0), an assembly and a solve, and every block they leave; with the model in force begin_iteration(0) books one launch more
    and an assembly none"""
    case = make_case(pkg, False)
    seen = []
    for touched in (False, True):
        m = pkg.capi.HipModel(case, tolerance=1e-4)
        m.set_state(case["pv"], case["meaning"])
        w = pkg.wells.DeviceStandardWells(make_wells(pkg, case, shared=False), case["depth"], m, head_model="wellbore" if touched else "cell_oil")
        if touched:
            m.set_std_wells_head_model(None)
        m.profile_enable(True)
        m.std_wells_begin_iteration(0)
        jr = m.assemble(DAY, 0)
        m.std_wells_apply_residual()
        res = m.solve_jacobian_system()
        m.update(None, 1.0)
        m.std_wells_update(1.0)
        m.synchronize()
        seen.append((H.launch_counts(m), res.it, jr, m.get_std_wells(), m.std_wells_blocks(), m.get_state()[0]))
    (ca, ita, jra, wa, ba, sa), (cb, itb, jrb, wb_, bb, sb) = seen
    assert ca == cb and ita == itb
    same(jra[0], jrb[0], "J")
    same(jra[1], jrb[1], "r")
    same(sa, sb, "state")
    for a, b in zip(wa, wb_):
        same(a, b, "get_std_wells")
    for k in ba:
        same(ba[k], bb[k], k)
    assert np.any(ba["xw"] != 0.0) and np.any(ba["head"] != 0.0)
    # with the model in force: one launch more at begin_iteration(0), none in an assembly
    counts = []
    for hm in ("cell_oil", "wellbore"):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        pkg.wells.DeviceStandardWells(make_wells(pkg, case, shared=False), case["depth"], m, head_model=hm)
        m.profile_enable(True)
        m.std_wells_begin_iteration(0)
        m.synchronize()
        n0 = m.profile()["assemble"][0]
        m.assemble(DAY, 0, fetch=False)
        m.std_wells_begin_iteration(1)
        m.assemble(DAY, 1, fetch=False)
        m.synchronize()
        counts.append((n0, m.profile()["assemble"][0] - n0))
    assert counts[1][0] == counts[0][0] + 1 and counts[1][1] == counts[0][1]

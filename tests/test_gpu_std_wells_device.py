"""Standard wells resident on the device (opmhip_set_std_wells) against wells.StandardWells(arithmetic="stated") on the same HipModel
state, bit for bit: one assembly on wells that sit on the 64-lane round boundaries, closed completions and the guard, a singular D, the
operator and the update, the SPE9-shaped schedule, a chopped step, an aquifer and a well in one cell, the refusals, and the launch counts
of a context that never saw the call.

Grid of the small tests: 2 x 2 x 150 (cell = i + 2 (j + 2 k)), one well per column: a 150-completion producer, a 64-completion water
injector, a 65-completion gas injector, a 1-completion producer, and two producers that share one cell."""
import uuid

import numpy as np
import pytest

import std_wells_harness as H
from std_wells_harness import make_case, moved, same_state

pytestmark = pytest.mark.gpu

DAY = 86400.0
column = H.column(2, 2)


def make_wells(pkg, case, shared=True, bad=False):
    W = pkg.wells
    def well(name, cells, producer, control, limit, inj=None):
        tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return W.Well(name, cells, tw, case["depth"][cells[0]], producer, control, limit, inj_phase=inj)
    out = [well("P150", column(0, 0, range(150)), True, ("rate", W.OIL, 40.0 / DAY), 150e5),
           well("W64", column(1, 0, range(64)), False, ("rate", W.WATER, 60.0 / DAY), 400e5, "water"),
           well("G65", column(0, 1, range(65)), False, ("rate", W.GAS, 5000.0 / DAY), 400e5, "gas"),
           well("P1", column(1, 1, [100]), True, ("rate", W.OIL, 2.0 / DAY), 150e5)]
    if shared:
        out += [well("SA", column(1, 1, [10, 11, 12]), True, ("rate", W.OIL, 3.0 / DAY), 150e5),
                well("SB", column(1, 1, [12, 13]), True, ("rate", W.WATER, 0.5 / DAY), 150e5)]
    if bad:   # a rate target on a component no completion of a water injector can flow: rows 0 and 3 of D are equal
        out.append(well("BAD", column(1, 1, [140, 141]), False, ("rate", W.OIL, 1.0 / DAY), 400e5, "water"))
    return out


# ---- 1. one assembly ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_one_assembly(pkg, ext):
    case = make_case(pkg, ext)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case))
    assert md.iq().shape[1] == (19 if ext else 17)
    assert list(np.diff(wh.vp)) == [150, 64, 65, 1, 3, 2] and len(wh.ucells) == len(wh.cells) - 1
    dt = 5.0 * DAY
    for it, state in ((0, None), (1, moved(case, 3))):
        if state is not None:
            for m in (md, mh):
                m.set_state(state, case["meaning"])
        wa = H.host_begin_and_assemble(mh, wh, it)
        jh, rh = mh.assemble(dt, it)
        wd.begin_iteration(it)
        jd, rd = md.assemble(dt, it)
        blk = H.compare_wells(pkg, md, wh, wa, it)
        x = blk["x"]
        assert np.array_equal(jd, jh) and np.array_equal(rd, rh), it              # the reservoir's J and r equal the host path's
        assert np.all(x[:, 3] > 100e5) and np.all(blk["head"][wh.vp[0] + 1:wh.vp[1]] > 0.0)
        assert np.count_nonzero(blk["rates"][:, :, 0]) > 50 and np.all(blk["B"][:, 3, :] == 0.0) and np.all(blk["C"][:, :3, :] == 0.0)
    # the caller's source arrays are back: without the list the assembly is that of a context that never had wells
    md.set_std_wells(None)
    plain = pkg.capi.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    plain.assemble(dt, 0, fetch=False)                                            # (the old time level's storage term, as md has it)
    plain.set_state(moved(case, 3), case["meaning"])
    (j0, r0), (jp, rp) = md.assemble(dt, 1), plain.assemble(dt, 1)
    assert np.array_equal(j0, jp) and np.array_equal(r0, rp) and not np.array_equal(r0, rd)


# ---- 2. closed completions, the guard ----------------------------------------------------------------------------------------------------------
def test_closed_completions_and_a_well_without_a_flowing_completion(pkg):
    case = make_case(pkg, False)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case))
    for m in (md, mh):
        m.set_state(moved(case, 11), case["meaning"])
    iq = H.begin(wd, mh, wh, 0)
    x0 = wh.x.copy()
    po = wh.records(mh).rows(wh.cells)[:, 4, 0]
    inflow = (po - wh.head)[:150]
    x0[0, 3] = np.median(inflow)                       # the long producer: about half of its completions would flow backwards - closed
    x0[3, 3] = po[wh.vp[3]] + 50e5                     # the one-completion producer: nothing flows, the guard keeps its equations regular
    wh.x = x0.copy()
    md.set_std_wells_state(x=x0)
    wa = H.host_assemble(mh, wh, iq)
    jh, rh = mh.assemble(DAY, 0)
    jd, rd = md.assemble(DAY, 0)
    blk = H.compare_wells(pkg, md, wh, wa, "closed")   # get_std_wells inside: no flag is reported
    assert np.array_equal(jd, jh) and np.array_equal(rd, rh)
    flowing = np.any(blk["rates"][:150, :, 0] != 0.0, axis=1)
    assert 10 < flowing.sum() < 140 and np.array_equal(flowing, inflow - x0[0, 3] > 0.0)
    assert np.all(blk["rates"][wh.vp[3]] == 0.0) and np.array_equal(blk["D"][3, 3], [0.0, 0.0, 0.0, 1.0]) and wa["res_well"].reshape(-1, 4)[3, 3] == 0.0


# ---- 3. a singular D ------------------------------------------------------------------------------------------------------------------------------
def test_singular_D_is_reported_not_divided_by(pkg):
    C = pkg.capi
    case = make_case(pkg, False)
    m = C.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    wd = pkg.wells.DeviceStandardWells(make_wells(pkg, case, bad=True), case["depth"], m)
    wd.begin_iteration(0)
    m.assemble(DAY, 0, fetch=False)
    blk = m.std_wells_blocks()
    assert all(np.all(np.isfinite(v)) for v in blk.values()) and np.all(blk["Dinv"][6] == 0.0) and np.any(blk["Dinv"][5] != 0.0)
    assert np.array_equal(blk["D"][6, 0], blk["D"][6, 3]) and blk["D"][6, 1, 3] != 0.0       # not the guard's case: the injector flows
    with pytest.raises(C.OpmHipError) as e:
        m.get_std_wells()
    assert e.value.code == C.INVALID_ARGUMENT and "singular" in str(e.value) and "well 6" in str(e.value)
    # the list is cleared: the next assemble is that of a context without wells, and the binding knows
    assert m.get_std_wells()[0].shape == (0, 4)
    plain = C.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    (j, r), (jp, rp) = m.assemble(DAY, 0), plain.assemble(DAY, 0)
    assert np.array_equal(j, jp) and np.array_equal(r, rp)
    # ... and opmhip_solve_system reports it as well when it is the first to look
    wd = pkg.wells.DeviceStandardWells(make_wells(pkg, case, bad=True), case["depth"], m)
    wd.begin_iteration(0)
    m.assemble(DAY, 0, fetch=False)
    with pytest.raises(C.OpmHipError) as e:
        m.solve_jacobian_system()
    assert e.value.code == C.INVALID_ARGUMENT and "singular" in str(e.value)
    with pytest.raises(pkg.wells.SingularWellEquations):      # the host's stated form reports the same wells
        wh = pkg.wells.StandardWells(make_wells(pkg, case, bad=True), case["depth"], arithmetic="stated")
        wh.solve_well_equations(wh.records(plain))


# ---- 4. operator and update ----------------------------------------------------------------------------------------------------------------------
def test_operator_and_update(pkg):
    """(the four wells that share no cell: where two wells meet in a cell the existing operator kernels add their two contributions
    atomically, in either order - with a host list as with the resident one)"""
    case = make_case(pkg, False)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case, shared=False), model_kw=dict(tolerance=1e-4))
    dt = 5.0 * DAY
    wa = H.host_begin_and_assemble(mh, wh, 0)
    mh.assemble(dt, 0, fetch=False)
    wd.begin_iteration(0)
    md.assemble(dt, 0, fetch=False)
    mh.wells_apply_residual(wa["wells"], wa["res_well"])
    md.std_wells_apply_residual()
    rh, rd = mh.get_rhs(), md.get_rhs()
    plain = pkg.capi.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    assert np.array_equal(rd, rh) and not np.array_equal(rd, plain.assemble(dt, 0)[1])
    sh, sd = mh.solve_jacobian_system(wells=wa["wells"]), md.solve_jacobian_system()
    assert sh.converged and sd.converged and sd.it == sh.it and sd.iterations == sh.iterations and sd.reduction == sh.reduction
    xw = mh.wells_recover_solution(wa["wells"], wa["res_well"])
    wh.update(xw, 0.7)
    md.std_wells_update(0.7)
    assert np.array_equal(md.get_result(), mh.get_result())
    assert np.array_equal(md.std_wells_blocks()["xw"].reshape(-1), xw) and np.any(xw != 0.0)
    assert np.array_equal(md.get_std_wells()[0], wh.x)


# ---- 5. schedule ----------------------------------------------------------------------------------------------------------------------------------
def run_schedule(pkg, m, wells, schedule, param=None):
    """tests/test_spe9_shaped_wells.py's run_schedule with the controls recorded after every Newton iteration"""
    model = pkg.newton.BlackoilModelHip(m, param=param, well_model=wells)
    ts = pkg.newton.AdaptiveTimeStepping(model, pkg.newton.TimeSteppingParameters(initial_dt=DAY))
    controls = lambda: "".join("R" if w.control[0] == "rate" else "B" for w in wells.wells)
    trail, steps = [], []
    inner = model.nonlinear_iteration

    def recorded(iteration, dt):
        rep = inner(iteration, dt)
        trail.append(controls())
        return rep
    model.nonlinear_iteration = recorded
    for length, rate in schedule:
        if rate is not None:
            for k in range(1, wells.nw):
                wells.set_rate_target(k, rate * pkg.decks.STB_PER_DAY)
        trail.append("|" + controls())                                   # the state an event leaves is no switch
        reps = ts.advance_report_step(length)
        steps.append((len(reps), sum(r.total_linear_iterations for r in reps), controls()))
    return ts, steps, trail


def spe9_runs(pkg, case, schedule, start_under_bhp=(), param=None):
    from test_spe9_shaped_wells import PRODUCER_BHP_LIMIT
    runs = []
    for form in ("device", "host"):
        m = pkg.capi.HipModel(case, tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
        m.set_state(case["pv"], case["meaning"])
        wl = pkg.decks.spe9_shaped_wells(case, producer_bhp_limit=PRODUCER_BHP_LIMIT).wells
        for k in start_under_bhp:
            wl[k].control = ("bhp", wl[k].bhp_limit)
        w = pkg.wells.DeviceStandardWells(wl, case["depth"], m) if form == "device" else pkg.wells.StandardWells(wl, case["depth"], arithmetic="stated")
        ts, steps, trail = run_schedule(pkg, m, w, schedule, param)
        x = w.fetch().copy() if form == "device" else w.x.copy()
        runs.append(dict(ts=ts, steps=steps, trail=trail, x=x, m=m))
    return runs


def test_spe9_shaped_schedule(pkg):
    """three report steps, device wells against host-stated wells: the same sub-steps, Newton and linear iterations, controls after every
    Newton iteration, the rate-target event; x and the reservoir state bit for bit.  Producer 2 starts under BHP control at its limit (a
    restarted well state): the limit lets it flow far more than its target, so updateWellControls takes it back to the target - the
    switch from BHP to rate - while other producers fall to their limit"""
    from test_spe9_shaped_wells import SCHEDULE
    case = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
    dev, host = spe9_runs(pkg, case, SCHEDULE, start_under_bhp=(2,))
    print("SPE9-shaped schedule, device wells: (Newton, linear, controls) per report step %r; sub-steps %r" % (dev["steps"], [round(h[0] / DAY, 2) for h in dev["ts"].history]))
    assert dev["steps"] == host["steps"] and dev["ts"].history == host["ts"].history and dev["trail"] == host["trail"]
    assert abs(dev["ts"].time - 30 * DAY) < 1.0
    assert np.array_equal(dev["x"], host["x"]) and same_state(dev["m"], host["m"])
    to_bhp = to_rate = 0
    for a, b in zip(dev["trail"], dev["trail"][1:]):
        if not b.startswith("|"):
            to_bhp += sum(p == "R" and q == "B" for p, q in zip(a.lstrip("|"), b))
            to_rate += sum(p == "B" and q == "R" for p, q in zip(a.lstrip("|"), b))
    assert to_bhp >= 3 and to_rate >= 1, (to_bhp, to_rate)
    assert dev["trail"][0][1 + 2] == "B" and dev["trail"][1][2] == "R"
    c1, c2, c3 = (s[2] for s in dev["steps"])
    assert c2[1:] == "R" * 25 and "B" in c1[1:] and "B" in c3[1:]              # the event of report step 2 put every producer back on its target


# ---- 6. chopped step ----------------------------------------------------------------------------------------------------------------------------------
def test_chopped_step(pkg):
    """a Newton method allowed four iterations fails its first, long step: update_failed restores x and the controls on both sides and the
    run that follows - chopped steps, then accepted ones - is the host's"""
    case = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
    runs = []
    from test_spe9_shaped_wells import PRODUCER_BHP_LIMIT
    for form in ("device", "host"):
        m = pkg.capi.HipModel(case, tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
        m.set_state(case["pv"], case["meaning"])
        wl = pkg.decks.spe9_shaped_wells(case, producer_bhp_limit=PRODUCER_BHP_LIMIT).wells
        w = pkg.wells.DeviceStandardWells(wl, case["depth"], m) if form == "device" else pkg.wells.StandardWells(wl, case["depth"], arithmetic="stated")
        model = pkg.newton.BlackoilModelHip(m, param=pkg.newton.ModelParameters(newton_max_iter=4), well_model=w)
        ts = pkg.newton.AdaptiveTimeStepping(model, pkg.newton.TimeSteppingParameters(initial_dt=20.0 * DAY))
        seen = []
        failed = model.update_failed

        def update_failed(m=m, w=w, failed=failed, seen=seen, form=form):
            failed()
            x = w.fetch().copy() if form == "device" else w.x.copy()
            seen.append((x, "".join(q.control[0][0] for q in w.wells), m.get_state()[0].copy()))
        model.update_failed = update_failed
        reps = ts.advance_report_step(10.0 * DAY)
        x = w.fetch().copy() if form == "device" else w.x.copy()
        runs.append(dict(history=list(ts.history), n=len(reps), x=x, m=m, seen=seen))
    dev, host = runs
    assert dev["history"] == host["history"] and dev["n"] == host["n"]
    assert any(not ok for _, _, ok in dev["history"]) and any(ok for _, _, ok in dev["history"])
    assert len(dev["seen"]) == len(host["seen"]) >= 1
    for (xd, cd, sd), (xh, ch, sh) in zip(dev["seen"], host["seen"]):
        assert np.array_equal(xd, xh) and cd == ch and np.array_equal(sd, sh)      # x, the controls and the reservoir of the step's start
    assert np.all(dev["seen"][0][0] == 0.0) and np.array_equal(dev["seen"][0][2], case["pv"])      # (the first step's start: wells not solved yet)
    assert np.any(dev["seen"][-1][0] != 0.0) and "b" in dev["seen"][-1][1]                         # (a later one: solved wells, some on their limit)
    assert np.array_equal(dev["x"], host["x"]) and same_state(dev["m"], host["m"])


# ---- 7. an aquifer and a well in one cell ------------------------------------------------------------------------------------------------------------
def test_aquifer_and_well_in_one_cell(pkg):
    case = pkg.decks.cartesian_case(4, 3, 5, state="mixed", heterogeneous=True)
    recs = pkg.decks.two_aquifers(case, None, None)
    W = pkg.wells
    def wells():
        cells = [0 + 4 * (1 + 3 * k) for k in (2, 3, 4)]                  # the I- face and, with k = 4, the bottom face: in both aquifers
        tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return [W.Well("P", cells, tw, case["depth"][cells[0]], True, ("rate", W.OIL, 5.0 / DAY), 100e5)]
    assert all(wells()[0].cells[2] in r["cells"] for r in recs)
    src = np.zeros((case["Nb"], 3))
    src[7] = [0.0, 1e-5, 0.0]                                             # a caller's rate elsewhere
    dt = 5.0 * DAY
    md, mh = (pkg.capi.HipModel(case) for _ in range(2))
    for m in (md, mh):
        m.set_state(case["pv"], case["meaning"])
    md.set_source(src.reshape(-1))
    md.set_aquifers(recs)
    md.aquifers_begin_time_step(0.0, dt)
    wd = W.DeviceStandardWells(wells(), case["depth"], md)
    wh = W.StandardWells(wells(), case["depth"], arithmetic="stated")
    ha = pkg.aquifers.HostAquifers(recs, case["depth"])
    ha.initial_solution_applied(mh)
    ha.begin_time_step(mh, 0.0, dt)
    for it, state in ((0, None), (1, moved(case, 5, dp=1e5))):
        if state is not None:
            for m in (md, mh):
                m.set_state(state, case["meaning"])
        wa = wh.assemble(H.host_begin(mh, wh, it))
        cells = np.concatenate([wa["cells"], [7]])                        # the host order: the wells' rates, then the aquifers' influx
        ha.add_to_source(mh, cells, np.vstack([wa["source_cells"].reshape(-1, 3), src[7:8]]), np.vstack([wa["dsource_cells"].reshape(-1, 9), np.zeros((1, 9))]))
        jh, rh = mh.assemble(dt, it)
        wd.begin_iteration(it)
        jd, rd = md.assemble(dt, it)
        assert np.array_equal(jd, jh) and np.array_equal(rd, rh), it
        assert np.array_equal(md.aquifer_rates(), ha.rates(mh.iq_cells(ha.cells)))
    # the caller's source arrays are back unchanged after assemble
    md.set_std_wells(None)
    md.set_aquifers(None)
    plain = pkg.capi.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    plain.set_source(src.reshape(-1))
    plain.assemble(dt, 0, fetch=False)                                    # (the old time level's storage term, as md has it)
    plain.set_state(moved(case, 5, dp=1e5), case["meaning"])
    (j0, r0), (jp, rp) = md.assemble(dt, 1), plain.assemble(dt, 1)
    assert np.array_equal(j0, jp) and np.array_equal(r0, rp) and not np.array_equal(r0, rd)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    case = make_case(pkg, False)
    good = dict(perf_pointers=[0, 2, 3], cell=[0, 4, 5], tw=[1e-12] * 3, dz=[0.0, 1.0, 0.0], producer=[1, 0], inj_phase=[0, 0], rate_component=[0, 1],
                rate_target=[1e-4, 1e-4], bhp_limit=[150e5, 400e5], control=[0, 0], x=None)

    def refused(model, w, code, word):
        sw, keep = C.make_std_wells(w)
        rc = C.lib().opmhip_set_std_wells(model._h, sw)
        msg = C.lib().opmhip_last_error(model._h).decode()
        assert rc == code and word in msg, (rc, msg)

    refused(C.HipFluid(case["fluid"]), good, C.NOT_READY, "set_static")
    m = C.HipModel(case)
    refused(m, good, C.NOT_READY, "set_state")
    m.set_state(case["pv"], case["meaning"])
    plain = C.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    jp, rp = plain.assemble(DAY, 0)
    for change, word in ((dict(cell=[0, 4, 600]), "outside"), (dict(cell=[-1, 4, 5]), "outside"), (dict(inj_phase=[0, 3]), "unknown phase"),
                         (dict(rate_component=[0, 5]), "unknown component"), (dict(control=[0, 2]), "control"), (dict(perf_pointers=[0, 3, 3]), "inconsistent pointers"),
                         (dict(perf_pointers=[1, 2, 3]), "inconsistent pointers")):
        m.set_std_wells(good)
        refused(m, dict(good, **change), C.INVALID_ARGUMENT, word)
        m.set_std_wells(None)                            # (the raw call went past the binding's record of the list's size)
        j, r = m.assemble(DAY, 0)                        # nothing is left set
        assert np.array_equal(j, jp) and np.array_equal(r, rp), word
        m.std_wells_begin_iteration(0)                   # a no-op without a list
        with pytest.raises(C.OpmHipError) as e:
            m.std_wells_apply_residual()
        assert e.value.code == C.NOT_READY
    sw, keep = C.make_std_wells(good)
    sw.tw = None
    assert C.lib().opmhip_set_std_wells(m._h, sw) == C.INVALID_ARGUMENT and "null array" in C.lib().opmhip_last_error(m._h).decode()
    # a solve before the first assembly; a host list beside a resident one
    m.assemble(DAY, 0, fetch=False)
    m.set_std_wells(good)
    with pytest.raises(C.OpmHipError) as e:
        m.solve_jacobian_system()
    assert e.value.code == C.NOT_READY and "not assembled" in str(e.value)
    m.std_wells_begin_iteration(0)
    m.assemble(DAY, 0, fetch=False)
    host = pkg.wells.StandardWells(make_wells(pkg, case, shared=False), case["depth"], arithmetic="stated")
    iq = host.records(plain)
    host.solve_well_equations(iq)
    wa = host.assemble(iq)
    for call in (lambda: m.solve_jacobian_system(wells=wa["wells"]), lambda: m.wells_apply_residual(wa["wells"], wa["res_well"])):
        with pytest.raises(C.OpmHipError) as e:
            call()
        assert e.value.code == C.INVALID_ARGUMENT and "applied twice" in str(e.value)
    assert m.solve_jacobian_system().converged           # the resident list is still in force
    m.set_std_wells(None)
    m.assemble(DAY, 0, fetch=False)
    m.wells_apply_residual(wa["wells"], wa["res_well"])  # ... and once it is cleared a host list is taken (and copied) again
    assert m.solve_jacobian_system(wells=wa["wells"]).converged
    # a second list with the producers and injectors swapped: the setters that ask which wells produce go by the list now set
    m.set_std_wells(good)
    m.set_std_wells(dict(good, producer=[0, 1]))
    with pytest.raises(ValueError, match="injector"):
        m.set_std_wells_crossflow([1, 0])
    m.set_std_wells_crossflow([0, 1])
    depths = dict(perf_depth=[2000.0, 2001.0, 2000.0], ref_depth=[2000.0, 2000.0])
    with pytest.raises(C.OpmHipError, match="unknown phase"):
        m.set_std_wells_head_model(dict(depths, preferred_phase=[1, 7]))
    m.set_std_wells_head_model(dict(depths, preferred_phase=[7, 1]))   # an injector's is not looked at
    m.set_std_wells(None)
    # a decomposed context (loopback, two ranks): out of scope
    sub = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    dd = C.HipModel(sub, comm=("loopback", 2, 0, "sw" + uuid.uuid4().hex), reorder="level_scheduling")
    dd.set_state(sub["pv"], sub["meaning"])
    refused(dd, good, C.INVALID_ARGUMENT, "decomposed")


# ---- 9. with no list set --------------------------------------------------------------------------------------------------------------------------
def test_no_list_no_launch(pkg):
    """profile_get's launch counts of an assemble + solve: a context whose list was set and cleared against one that never saw the call"""
    case = make_case(pkg, False)
    counts = []
    for touched in (True, False):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        if touched:
            pkg.wells.DeviceStandardWells(make_wells(pkg, case), case["depth"], m)
            m.std_wells_begin_iteration(0)
            m.assemble(DAY, 0, fetch=False)
            m.set_std_wells(None)
        m.profile_enable(True)
        m.std_wells_begin_iteration(0)
        m.assemble(DAY, 0, fetch=False)
        res = m.solve_jacobian_system()
        m.update(None, 1.0)
        m.synchronize()
        counts.append((H.launch_counts(m), res.it, m.get_state()[0]))
    (a, ita, sa), (b, itb, sb) = counts
    assert a == b and ita == itb and np.array_equal(sa, sb) and a["assemble"] >= 1 and a["spmv"] >= 1
    # ... and the counts do show the new launches: with a list set the same calls book the wells alone, the controls, the equations
    # with the source rows and the restore beside the assembly kernel
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    pkg.wells.DeviceStandardWells(make_wells(pkg, case), case["depth"], m)
    m.profile_enable(True)
    m.std_wells_begin_iteration(0)
    m.assemble(DAY, 0, fetch=False)
    m.synchronize()
    assert m.profile()["assemble"][0] == a["assemble"] + 4

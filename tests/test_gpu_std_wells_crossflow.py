"""Crossflow in producers on the device (opmhip_set_std_wells_crossflow, k_std_wells_eq<., true>) against
wells.StandardWells(arithmetic="stated") on the same HipModel state, bit for bit: one assembly on the forced-reversal state of
tests/test_std_wells_crossflow.py (its grid, its wells: producers of 150, 65 and 1 completions with the switch, a 64-completion water
injector without), the operator and the update with those blocks, the first report step of the SPE9-shaped schedule, the well-bore
heads from stored injecting rates, the refusals and the launch counts."""
import numpy as np
import pytest

import std_wells_harness as H
from std_wells_harness import make_case, moved, same_state
from test_std_wells_crossflow import make_wells, median_bhp

pytestmark = pytest.mark.gpu

DAY = 86400.0
INJECTED_DURING_THE_RUN = False     # test c: no perforation injected during the SPE9-shaped report step (see its docstring)


def force_reversal(md, mh, wh, iq):
    """the long producer's bottom-hole pressure at the median of p_o - head, on both sides"""
    x0 = wh.x.copy()
    x0[0, 3] = median_bhp(wh, iq)
    wh.x = x0.copy()
    md.set_std_wells_state(x=x0)
    return x0


def assembles_what_assemble_wells_forms(wh, wa, iq):
    """on the host alone: assemble's r_w and C are _assemble_wells' (the same state: the same bits as inside assemble), from which the
    comparison forms D and the rates once more"""
    r, _, _, C, _, _ = wh._assemble_wells(iq)
    assert np.array_equal(wa["res_well"].reshape(-1, 4), r) and np.array_equal(wa["wells"]["Cnnzs"].reshape(len(wh.cells), 4, 3), C)


# ---- a. one assembly -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_one_assembly(pkg, ext):
    case = make_case(pkg, ext)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case), head_model="cell_oil", props="wellbore")
    assert md.iq().shape[1] == (19 if ext else 17) and list(np.diff(wh.vp)) == [150, 64, 65, 1]
    assert [bool(f) for f in wh.allow_crossflow] == [True, False, True, True]
    dt = 5.0 * DAY
    for it, state in ((0, None), (1, moved(case, 3))):
        if state is not None:
            for m in (md, mh):
                m.set_state(state, case["meaning"])
        iq = H.begin(wd, mh, wh, it)
        if it == 0:
            assert np.array_equal(md.get_std_wells()[0], wh.x) and np.all(wh.x[[0, 2, 3], :3] < 0.0)      # the wells alone, crossflow inside their loop
            force_reversal(md, mh, wh, iq)
        wa = H.host_assemble(mh, wh, iq)
        jh, rh = mh.assemble(dt, it)
        jd, rd = md.assemble(dt, it)
        assembles_what_assemble_wells_forms(wh, wa, iq)
        got = H.compare_wells(pkg, md, wh, wa, it, extra=("D", "rates", "dq"), iq=iq, all_finite=True)
        assert np.array_equal(jd, jh) and np.array_equal(rd, rh), it              # the reservoir's J and r equal the host path's
        injecting = (got["rates"][:150, :, 0] > 0.0).any(axis=1)
        assert 10 <= injecting.sum() <= 140, (it, injecting.sum())
        assert np.any(got["C"][:150, :3, :] != 0.0) and np.all(got["C"][150:214, :3, :] == 0.0) and np.any(got["dq"][:150] != 0.0)
        assert not np.array_equal(got["D"][0, :3, :3], np.eye(3)) and np.array_equal(got["D"][1, :3, :3], np.eye(3))
        assert np.array_equal(got["C"][:, :3, :], -got["dq"].transpose(0, 2, 1))


# ---- b. operator and update --------------------------------------------------------------------------------------------------------------------------
def test_operator_and_update(pkg):
    """(wells that share no cell: where two wells meet in a cell the existing operator kernels add their two contributions atomically,
    in either order - with a host list as with the resident one)"""
    case = make_case(pkg, False)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case), head_model="cell_oil", props="wellbore", model_kw=dict(tolerance=1e-4))
    dt = 5.0 * DAY
    iq = H.begin(wd, mh, wh, 0)
    force_reversal(md, mh, wh, iq)
    wa = H.host_assemble(mh, wh, iq)
    mh.assemble(dt, 0, fetch=False)
    md.assemble(dt, 0, fetch=False)
    assert np.any(wa["wells"]["Cnnzs"].reshape(-1, 4, 3)[:, :3, :] != 0.0)
    mh.wells_apply_residual(wa["wells"], wa["res_well"])
    md.std_wells_apply_residual()
    rh, rd = mh.get_rhs(), md.get_rhs()
    assert np.array_equal(rd, rh)
    sh, sd = mh.solve_jacobian_system(wells=wa["wells"]), md.solve_jacobian_system()
    assert sh.converged and sd.converged and sd.it == sh.it and sd.iterations == sh.iterations and sd.reduction == sh.reduction
    xw = mh.wells_recover_solution(wa["wells"], wa["res_well"])
    wh.update(xw, 0.7)
    md.std_wells_update(0.7)
    assert np.array_equal(md.get_result(), mh.get_result())
    assert np.array_equal(md.std_wells_blocks()["xw"].reshape(-1), xw) and np.any(xw != 0.0)
    assert np.array_equal(md.get_std_wells()[0], wh.x)


# ---- c. a short run ------------------------------------------------------------------------------------------------------------------------------------
def test_spe9_shaped_first_report_step(pkg):
    """the first report step of tests/test_spe9_shaped_wells.py's SCHEDULE with the switch on every producer, device wells against
    host-stated wells: the same sub-steps, Newton and linear iterations, controls after every Newton iteration; x and the reservoir
    state bit for bit.  No perforation injects during this run: the producers are completed in three adjacent layers of one column,
    6 m apart, and their drawdown under the rate target is far larger than the difference between the explicit head and the reservoir's
    gradient over 12 m - the run shows that the crossflow instantiation with the switch on every producer reproduces the host through
    a whole report step (the wells alone, the controls, chopped and accepted sub-steps), and tests a, b and d cover injecting
    perforations.  The count of perforations with a non-zero d rate / d q is recorded after every Newton iteration on both sides."""
    from test_spe9_shaped_wells import PRODUCER_BHP_LIMIT, SCHEDULE
    case = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
    runs = []
    for form in ("device", "host"):
        m = pkg.capi.HipModel(case, tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
        m.set_state(case["pv"], case["meaning"])
        wl = pkg.decks.spe9_shaped_wells(case, producer_bhp_limit=PRODUCER_BHP_LIMIT).wells
        for w in wl:
            w.allow_crossflow = w.producer
        w = pkg.wells.DeviceStandardWells(wl, case["depth"], m) if form == "device" else pkg.wells.StandardWells(wl, case["depth"], arithmetic="stated")
        assert w.allow_crossflow.sum() == 25
        model = pkg.newton.BlackoilModelHip(m, well_model=w)
        ts = pkg.newton.AdaptiveTimeStepping(model, pkg.newton.TimeSteppingParameters(initial_dt=DAY))
        controls = lambda w=w: "".join("R" if q.control[0] == "rate" else "B" for q in w.wells)
        trail, injected = [], []
        inner = model.nonlinear_iteration

        def recorded(iteration, dt, inner=inner, trail=trail, injected=injected, m=m, w=w, form=form, controls=controls):
            rep = inner(iteration, dt)
            trail.append(controls())
            injected.append(int(np.count_nonzero((m.std_wells_rate_dq() if form == "device" else w.rate_dq).any(axis=(1, 2)))))
            return rep
        model.nonlinear_iteration = recorded
        reps = ts.advance_report_step(SCHEDULE[0][0])
        x = w.fetch().copy() if form == "device" else w.x.copy()
        runs.append(dict(history=list(ts.history), newton=len(reps), linear=sum(r.total_linear_iterations for r in reps), trail=trail, x=x, m=m, injected=injected,
                         time=ts.time))
    dev, host = runs
    print("SPE9-shaped first report step with crossflow: %d Newton, %d linear iterations, sub-steps %r; injecting perforations per iteration %r"
          % (dev["newton"], dev["linear"], [round(h[0] / DAY, 2) for h in dev["history"]], dev["injected"]))
    assert dev["history"] == host["history"] and (dev["newton"], dev["linear"]) == (host["newton"], host["linear"]) and dev["trail"] == host["trail"]
    assert abs(dev["time"] - SCHEDULE[0][0]) < 1.0
    assert np.array_equal(dev["x"], host["x"]) and same_state(dev["m"], host["m"])
    assert dev["injected"] == host["injected"]
    assert (max(dev["injected"]) > 0) == INJECTED_DURING_THE_RUN


# ---- d. well-bore heads ------------------------------------------------------------------------------------------------------------------------------
def test_wellbore_heads_from_stored_injecting_rates(pkg):
    """two time-step starts: the second forms the well-bore density from the rates the first assembly stored, injecting signs included"""
    case = make_case(pkg, False)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case), head_model="wellbore", props="wellbore")
    dt = 5.0 * DAY
    for start in (0, 1):
        iq = H.begin(wd, mh, wh, 0)
        wb, blk = md.std_wells_wellbore(), md.std_wells_blocks()
        for k in ("density", "p_avg", "mixture"):
            assert np.array_equal(wb[k], wh.wellbore[k]), (start, k)
        assert np.array_equal(blk["head"], wh.head) and np.array_equal(md.get_std_wells()[0], wh.x), start
        if start == 0:
            force_reversal(md, mh, wh, iq)
            heads0 = wh.head.copy()
        wa = H.host_assemble(mh, wh, iq)
        mh.assemble(dt, 0, fetch=False)
        md.assemble(dt, 0, fetch=False)
        assembles_what_assemble_wells_forms(wh, wa, iq)
        H.compare_wells(pkg, md, wh, wa, start, extra=("D", "rates", "dq"), iq=iq, all_finite=True)
        wb = md.std_wells_wellbore()
        assert np.array_equal(wb["perf_rates"], wh.perf_rates) and np.array_equal(wb["perf_pressure"], wh.perf_pressure), start
        if start == 0:
            assert np.any(wh.perf_rates[:150] > 0.0) and np.any(wh.perf_rates[:150] < 0.0)       # stored: injecting and producing perforations
    assert not np.array_equal(wh.head, heads0)


# ---- e. refusals and the no-change guarantee -----------------------------------------------------------------------------------------------------
def test_refusals_and_the_previous_flags(pkg):
    C = pkg.capi
    case = make_case(pkg, False)

    def raw(model, allow):
        a = None if allow is None else np.ascontiguousarray(allow, np.int32)
        rc = C.lib().opmhip_set_std_wells_crossflow(model._h, C._ptr(a))
        return rc, C.lib().opmhip_last_error(model._h).decode()

    m = C.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    rc, msg = raw(m, [1, 0, 1, 1])
    assert rc == C.NOT_READY and "no resident list" in msg                  # before a list
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: make_wells(pkg, case), head_model="cell_oil", props="wellbore")
    iq = H.begin(wd, mh, wh, 0)
    force_reversal(md, mh, wh, iq)
    md.assemble(DAY, 0, fetch=False)
    dq0, blk0 = md.std_wells_rate_dq(), md.std_wells_blocks()
    assert np.any(dq0 != 0.0)
    rc, msg = raw(md, [1, 0, 2, 1])
    assert rc == C.INVALID_ARGUMENT and "allow[2] = 2" in msg
    rc, msg = raw(md, [1, 1, 1, 1])
    assert rc == C.INVALID_ARGUMENT and "injector" in msg
    with pytest.raises(ValueError, match="injector"):
        md.set_std_wells_crossflow([0, 1, 0, 0])
    with pytest.raises(ValueError):
        md.set_std_wells_crossflow([1, 0, 1])                                # ragged
    wl = make_wells(pkg, case)
    wl[1].allow_crossflow = True
    with pytest.raises(ValueError, match="injector"):
        pkg.wells.DeviceStandardWells(wl, case["depth"], C.HipModel(case))
    # the previous flags are in force: the next assembly is the one before the refused calls
    md.assemble(DAY, 0, fetch=False)
    blk1 = md.std_wells_blocks()
    assert np.array_equal(md.std_wells_rate_dq(), dq0) and all(np.array_equal(blk0[k], blk1[k]) for k in blk0)
    # an accepted call makes the last assembly stale; flags off: the reversed perforations are closed again
    md.set_std_wells_crossflow([0, 0, 0, 0])
    with pytest.raises(C.OpmHipError) as e:
        md.solve_jacobian_system()
    assert e.value.code == C.NOT_READY
    md.assemble(DAY, 0, fetch=False)
    blk2 = md.std_wells_blocks()
    assert np.all(md.std_wells_rate_dq() == 0.0) and np.all(blk2["C"][:, :3, :] == 0.0) and not np.any(blk2["rates"][:150, :, 0] > 0.0)
    # replacing the list clears the flags
    md.set_std_wells_crossflow([1, 0, 0, 0])
    wd2 = pkg.wells.DeviceStandardWells(make_wells(pkg, case, crossflow=False), case["depth"], md)
    wd2.begin_iteration(0)
    md.set_std_wells_state(x=wh.x)
    md.assemble(DAY, 0, fetch=False)
    assert np.all(md.std_wells_rate_dq() == 0.0) and np.all(md.std_wells_blocks()["C"][:, :3, :] == 0.0)


def test_flags_off_launch_and_compute_what_they_did(pkg):
    """profile_get's launch counts and the bits of begin_iteration + assemble + solve + update: all-zero flags against a context that
    never saw the call; with a flag set the count is the same - the crossflow instantiation runs in place of the other"""
    case = make_case(pkg, False)
    seen = []
    for flags in (None, [0, 0, 0, 0], [1, 0, 1, 1]):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        wd = pkg.wells.DeviceStandardWells(make_wells(pkg, case, crossflow=False), case["depth"], m)
        if flags is not None:
            m.set_std_wells_crossflow(flags)
        m.profile_enable(True)
        wd.begin_iteration(0)
        j, r = m.assemble(DAY, 0)
        blk = m.std_wells_blocks()
        res = m.solve_jacobian_system()
        wd.update(1.0)
        m.update(None, 1.0)
        m.synchronize()
        seen.append(dict(counts=H.launch_counts(m), j=j, r=r, blk=blk, it=res.it, x=m.get_std_wells()[0], state=m.get_state()[0]))
    never, zeros, on = seen
    assert never["counts"] == zeros["counts"] and never["counts"]["assemble"] >= 5
    assert np.array_equal(never["j"], zeros["j"]) and np.array_equal(never["r"], zeros["r"]) and never["it"] == zeros["it"]
    assert all(np.array_equal(never["blk"][k], zeros["blk"][k]) for k in never["blk"])
    assert np.array_equal(never["x"], zeros["x"]) and np.array_equal(never["state"], zeros["state"])
    assert on["counts"]["assemble"] == never["counts"]["assemble"] + 0       # no launch is added
    assert not np.array_equal(on["blk"]["rates"], never["blk"]["rates"])     # (and the switch did act: the solved wells have reversed perforations)

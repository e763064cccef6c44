"""THP control of the device-resident standard wells (opmhip_set_vfp_tables, opmhip_set_std_wells_thp) against
wells.StandardWells(arithmetic="stated", vfp=...) on the same HipModel state, bit for bit.  tests/thp_cases.py holds the case: a
3 x 3 x 65 grid, a 65-completion producer and a water injector with THP limits that bind, a producer without one."""
import numpy as np
import pytest

import std_wells_harness as H
import thp_cases
from std_wells_harness import moved

pytestmark = pytest.mark.gpu

DAY = thp_cases.DAY
CODE = {"rate": 0, "bhp": 1, "thp": 2}


def force(wd, wh, controls, x=None):
    """the same controls (names) and, if given, well unknowns on both sides"""
    for w, c in zip(wh.wells, controls):
        w.control = thp_cases.control_of(w, c)
    if x is not None:
        wh.x = np.array(x, float)
    wd.m.set_std_wells_state(x, [CODE[c] for c in controls], None)


# ---- 1. one assembly and the wells alone under forced control 2 -------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_one_assembly_and_the_wells_alone_under_thp(pkg, ext):
    case = thp_cases.make_case(pkg, ext)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: thp_cases.make_wells(pkg, case), head_model="cell_oil", vfp=thp_cases.tables(pkg), props="wellbore")
    assert md.iq().shape[1] == (19 if ext else 17) and list(np.diff(wh.vp)) == [65, 3, 2]
    force(wd, wh, ["thp", "thp", "rate"])
    dt = 5.0 * DAY
    for it, state in ((0, None), (1, moved(case, 3))):
        if state is not None:
            for m in (md, mh):
                m.set_state(state, case["meaning"])
        wa = H.host_begin_and_assemble(mh, wh, it)
        jh, rh = mh.assemble(dt, it)
        wd.begin_iteration(it)
        jd, rd = md.assemble(dt, it)
        blk = H.compare_wells(pkg, md, wh, wa, it, extra=("D", "thp"), mh=mh)
        x = blk["x"]
        assert np.array_equal(jd, jh) and np.array_equal(rd, rh), it              # the reservoir's J and r equal the host path's
        assert [w.control[0] for w in wh.wells] == ["thp", "thp", "rate"]
        assert np.all(blk["D"][0, 3, [0, 2]] != 0.0) and blk["D"][1, 3, 1] != 0.0 and np.all(blk["D"][:2, 3, 3] == 1.0)
        if it == 0:                                      # (against the moved reservoir none of P2's two completions flows: the guard's row)
            assert np.array_equal(blk["D"][2, 3], [1.0, 0.0, 0.0, 0.0])
        assert np.count_nonzero(blk["rates"][:65, :, 0]) > 100
    # the wells alone reached V - dp (iteration 0), and at iteration 1 the moved reservoir leaves a residual on the mass balances, not on the row
    t = md.std_wells_thp()
    assert np.all(t["dp"][:2] < 0.0) and t["dp"][2] == 0.0 and np.all(np.abs(x[:2, 3] - t["bhp_from_thp"][:2]) <= 2e-3)


# ---- 2. the switching table ----------------------------------------------------------------------------------------------------------------------
def test_switching_table(pkg):
    case = thp_cases.make_case(pkg)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: thp_cases.make_wells(pkg, case), head_model="cell_oil", vfp=thp_cases.tables(pkg), props="wellbore")
    iq = wh.records(mh)
    wh.calculate_explicit_quantities(iq)
    wh.solve_well_equations(iq)
    xs = wh.x.copy()                                    # the wells alone under their rate targets
    wd.begin_iteration(0)                               # one begin_iteration: dp is set (and the controls have switched: every case sets them anew)
    assert np.array_equal(md.std_wells_thp()["dp"], wh.thp_dp) and np.all(wh.thp_dp[:2] != 0.0)
    seen = set()
    for name, k, before, xk, after in thp_cases.transitions(xs):
        x = xs.copy()
        x[k] = xk
        controls = ["rate"] * 3
        controls[k] = before
        force(wd, wh, controls, x)
        wd.begin_iteration(1)
        wh.update_well_controls()
        assert wh.wells[k].control[0] == after, name
        xd = wd.fetch()
        assert np.array_equal(xd, wh.x), name
        assert [w.control for w in wd.wells] == [w.control for w in wh.wells], name
        assert np.array_equal(md.std_wells_thp()["thp"], wh.thp_current), name
        assert wh.thp_current[k] == pkg.vfp.thp(wh.thp_tables[k], xk[1], xk[0], xk[2], xk[3] + wh.thp_dp[k], 0.0), name
        seen.add((k, before, after))
    for k in (0, 1):
        assert {(k, "rate", "thp"), (k, "bhp", "thp"), (k, "thp", "bhp"), (k, "thp", "rate"), (k, "rate", "bhp"), (k, "thp", "thp")} <= seen


# ---- 3. dp under both head models ------------------------------------------------------------------------------------------------------------------
def test_dp_under_both_head_models(pkg):
    case = thp_cases.make_case(pkg)
    dps = {}
    for hm in ("cell_oil", "wellbore"):
        (md, wd), (mh, wh) = H.pair(pkg, case, lambda: thp_cases.make_wells(pkg, case), head_model=hm, vfp=thp_cases.tables(pkg), props="wellbore")
        for it in (0, 1):
            wa = H.host_begin_and_assemble(mh, wh, it)
            mh.assemble(DAY, it, fetch=False)
            wd.begin_iteration(it)
            md.assemble(DAY, it, fetch=False)
            H.compare_wells(pkg, md, wh, wa, (hm, it), extra=("D", "thp"), mh=mh)
        assert [w.control[0] for w in wh.wells] == ["thp", "thp", "rate"]
        dps[hm] = md.std_wells_thp()["dp"]
        W = pkg.wells
        rho = wh.wellbore["density"][wh.vp[:-1]] if hm == "wellbore" else wh.records(mh).rows(wh.cells)[wh.vp[:-1], W.F_RHO + W.PH_O, 0]
        assert np.array_equal(dps[hm][:2], ((rho * W.GRAVITY) * (2490.0 - np.array([w.ref_depth for w in wh.wells])))[:2])
    # the injector's column is water under the well-bore model, oil under the other: dp differs by far more than rounding
    assert abs(dps["wellbore"][1] - dps["cell_oil"][1]) > 0.1 * abs(dps["cell_oil"][1])


# ---- 4. a report step through newton.BlackoilModelHip -----------------------------------------------------------------------------------------------
def run_step(pkg, m, wells, length, dt0):
    model = pkg.newton.BlackoilModelHip(m, well_model=wells)
    ts = pkg.newton.AdaptiveTimeStepping(model, pkg.newton.TimeSteppingParameters(initial_dt=dt0))
    controls = lambda: "".join(w.control[0][0] for w in wells.wells)
    trail = ["|" + controls()]
    inner = model.nonlinear_iteration

    def recorded(iteration, dt):
        rep = inner(iteration, dt)
        trail.append(controls())
        return rep
    model.nonlinear_iteration = recorded
    reps = ts.advance_report_step(length)
    return ts, trail, (len(reps), sum(r.total_linear_iterations for r in reps))


def test_report_step_device_wells_against_host_wells(pkg):
    case = thp_cases.make_case(pkg)
    runs = []
    for (m, w) in H.pair(pkg, case, lambda: thp_cases.make_wells(pkg, case), head_model="cell_oil", vfp=thp_cases.tables(pkg), props="wellbore",
                         model_kw=dict(tolerance=1e-2, maxit=200, ilu_relaxation=0.9)):
        ts, trail, steps = run_step(pkg, m, w, 2.0 * DAY, 0.5 * DAY)
        x = w.fetch().copy() if getattr(w, "on_device", False) else w.x.copy()
        runs.append(dict(ts=ts, trail=trail, steps=steps, x=x, m=m, w=w))
    dev, host = runs
    print("report step, device wells: (sub-steps, linear iterations) %r, controls %r" % (dev["steps"], dev["trail"]))
    assert dev["steps"] == host["steps"] and dev["ts"].history == host["ts"].history and dev["trail"] == host["trail"]
    assert abs(dev["ts"].time - 2.0 * DAY) < 1.0
    (pd, mdn), (ph, mhn) = dev["m"].get_state(), host["m"].get_state()
    assert np.array_equal(dev["x"], host["x"]) and np.array_equal(pd, ph) and np.array_equal(mdn, mhn)
    # the test shows something: a well is under THP control at the end and a well switched during the step
    assert "t" in dev["trail"][-1] and dev["trail"][0] == "|rrr" and any(a != b for a, b in zip(dev["trail"][0][1:], dev["trail"][-1]))
    t = dev["m"].std_wells_thp()
    under = [k for k, w in enumerate(dev["w"].wells) if w.control[0] == "thp"]
    assert under and np.all(np.abs(dev["x"][under, 3] - t["bhp_from_thp"][under]) <= 1.0)     # tol_bhp: the row converged


# ---- 5. update_failed --------------------------------------------------------------------------------------------------------------------------------
def test_update_failed_after_a_switch_to_thp(pkg):
    case = thp_cases.make_case(pkg)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: thp_cases.make_wells(pkg, case), head_model="cell_oil", vfp=thp_cases.tables(pkg), props="wellbore")
    dt = 5.0 * DAY
    # an accepted first step's start: solved wells under their rate targets (the controls forced back), saved as the time level
    wd.begin_iteration(0)
    H.host_begin(mh, wh, 0)
    x0 = wd.fetch().copy()
    assert np.array_equal(x0, wh.x)
    x0[:, 3] = [236e5, 255e5, 253e5]
    force(wd, wh, ["rate"] * 3, x0)
    md.advance_time_level()
    saved = wh.state()
    # the step that is given up: it switches to THP and moves x
    wd.begin_iteration(0)
    md.assemble(dt, 0, fetch=False)
    x1 = wd.fetch().copy()
    assert [w.control[0] for w in wd.wells] == ["thp", "thp", "rate"] and not np.array_equal(x1, x0)
    md.update_failed()
    assert np.array_equal(wd.fetch(), x0) and [w.control for w in wd.wells] == [w.rate_control for w in wd.wells]
    # the retry: dp is formed anew, the same switch, the host's numbers
    wh.set_state(saved)
    H.host_begin(mh, wh, 0)
    wd.begin_iteration(0)
    assert np.array_equal(wd.fetch(), wh.x) and np.array_equal(wd.x, x1) and [w.control for w in wd.wells] == [w.control for w in wh.wells]
    assert np.array_equal(md.std_wells_thp()["dp"], wh.thp_dp)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_setting_in_force(pkg):
    C = pkg.capi
    case = thp_cases.make_case(pkg)
    tabs = thp_cases.tables(pkg)
    ref_depth = [w.ref_depth for w in thp_cases.make_wells(pkg, case)]
    good = dict(vfp_table=[5, 7, 0], thp_limit=[thp_cases.PROD_LIMIT, thp_cases.INJ_LIMIT, 0.0], alq=[0.0] * 3, dh=[2490.0 - ref_depth[0], 2490.0 - ref_depth[1], 0.0])

    def refused(call, code, word):
        with pytest.raises(C.OpmHipError) as e:
            call()
        assert e.value.code == code and word in str(e.value), str(e.value)

    m = C.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    rc = C.lib().opmhip_set_std_wells_thp(m._h, None)
    assert rc == C.NOT_READY and "no resident list" in C.lib().opmhip_last_error(m._h).decode()
    wd = pkg.wells.DeviceStandardWells(thp_cases.make_wells(pkg, case, limits=False), case["depth"], m)
    refused(lambda: m.set_std_wells_thp(good), C.NOT_READY, "no VFP tables")
    refused(lambda: m.set_std_wells_state(None, [2, 0, 0], None), C.INVALID_ARGUMENT, "control")          # no limits at all: 0 / 1 as before
    m.set_vfp_tables(tabs)
    m.set_std_wells_thp(good)
    ref = C.HipModel(case)
    ref.set_state(case["pv"], case["meaning"])
    pkg.wells.DeviceStandardWells(thp_cases.make_wells(pkg, case), case["depth"], ref, vfp=tabs)
    single = pkg.vfp.VFPTable(0, 11, 2490.0, "LIQ", [[0.0, 1.0], [50e5], [0.0], [0.0], [0.0]], [200e5, 210e5], "WCT", "GOR")
    for change, word in ((dict(vfp_table=[6, 7, 0]), "does not exist"), (dict(vfp_table=[7, 7, 0]), "does not exist"), (dict(vfp_table=[5, 5, 0]), "does not exist"),
                         (dict(thp_limit=[np.nan, 15e5, 0.0]), "not finite"), (dict(alq=[0.0, np.inf, 0.0]), "not finite"), (dict(dh=[0.0, -np.inf, 0.0]), "not finite")):
        refused(lambda: m.set_std_wells_thp(dict(good, **change)), C.INVALID_ARGUMENT, word)
    refused(lambda: m.set_vfp_tables(tabs + [single]), C.INVALID_ARGUMENT, "THP limits")                  # the tables in force are named by the limits
    refused(lambda: m.set_vfp_tables(None), C.INVALID_ARGUMENT, "THP limits")
    refused(lambda: m.set_std_wells_state(None, [0, 0, 2], None), C.INVALID_ARGUMENT, "without a THP limit")
    refused(lambda: m.set_std_wells_state(None, [3, 0, 0], None), C.INVALID_ARGUMENT, "control")
    sw, keep = C.make_std_wells(dict(perf_pointers=[0, 1], cell=[0], tw=[1e-12], dz=[0.0], producer=[1], inj_phase=[0], rate_component=[0], rate_target=[1e-4],
                                     bhp_limit=[150e5], control=[2], x=None))
    other = C.HipModel(case)
    other.set_state(case["pv"], case["meaning"])
    assert C.lib().opmhip_set_std_wells(other._h, sw) == C.INVALID_ARGUMENT and "control" in C.lib().opmhip_last_error(other._h).decode()
    # the previous setting is in force: the same wells alone, the same switch, the same numbers as a context that saw the good calls only
    for mm in (m, ref):
        mm.std_wells_begin_iteration(0)
        mm.assemble(DAY, 0, fetch=False)
    (xa, ca, ra), (xb, cb, rb) = m.get_std_wells(), ref.get_std_wells()
    assert np.array_equal(xa, xb) and list(ca) == list(cb) == [2, 2, 0] and np.array_equal(ra, rb)
    assert all(np.array_equal(m.std_wells_thp()[k], ref.std_wells_thp()[k]) for k in ("thp", "dp", "bhp_from_thp"))
    # a well under THP control cannot lose its limit; under another control it can, and then the tables can be replaced
    refused(lambda: m.set_std_wells_thp(None), C.INVALID_ARGUMENT, "under THP control")
    refused(lambda: m.set_std_wells_thp(dict(good, vfp_table=[5, 0, 0])), C.INVALID_ARGUMENT, "under THP control")
    m.set_std_wells_state(None, [0, 0, 0], None)
    m.set_std_wells_thp(None)
    assert np.all(m.std_wells_thp()["dp"] == 0.0)
    m.set_vfp_tables(tabs + [single])
    refused(lambda: m.set_std_wells_thp(dict(good, vfp_table=[11, 7, 0])), C.INVALID_ARGUMENT, "fewer than two")
    m.set_std_wells_thp(good)
    m.set_std_wells(None)                                # clearing the list clears the limits
    m.set_vfp_tables(None)
    refused(lambda: m.vfp_probe(0, 5, -1e-4, -1e-4, -1e-2, 50e5), C.NOT_READY, "set_vfp_tables")


# ---- 7. launch counts ------------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_grow(pkg):
    """opmhip_profile_get's launch counts per class of one Newton iteration (begin_iteration(0), assemble, solve, update): a list without limits
    that saw opmhip_set_std_wells_thp with every vfp_table == 0 against one that never saw the call - the same counts and the same bits -,
    and a list with THP wells - the same counts"""
    case = thp_cases.make_case(pkg)
    tabs = thp_cases.tables(pkg)
    runs = []
    for kind in ("plain", "zeros", "thp"):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        pkg.wells.DeviceStandardWells(thp_cases.make_wells(pkg, case, limits=(kind == "thp")), case["depth"], m, vfp=tabs)
        if kind == "zeros":
            m.set_vfp_tables(tabs)
            m.set_std_wells_thp(dict(vfp_table=[0, 0, 0], thp_limit=[0.0] * 3, alq=[0.0] * 3, dh=[0.0] * 3))
        m.profile_enable(True)
        m.std_wells_begin_iteration(0)
        m.assemble(DAY, 0, fetch=False)
        res = m.solve_jacobian_system()
        m.std_wells_update(1.0)
        m.update(None, 1.0)
        m.synchronize()
        runs.append((H.launch_counts(m), res.it, m.get_std_wells(), m.get_state()[0]))
    (a, ita, wa, sa), (b, itb, wb, sb), (c, itc, wc, sc) = runs
    assert a == b and ita == itb and np.array_equal(sa, sb) and all(np.array_equal(p, q) for p, q in zip(wa, wb))
    assert a["assemble"] == c["assemble"] and a["assemble"] >= 5         # the wells alone, the controls, the equations, the source rows, the assembly, the restore
    if itc == ita:                                                        # (another linear system may take another number of iterations)
        assert a == c
    assert list(wc[1]) == [2, 2, 0] and not np.array_equal(wc[0], wa[0])

"""Vaporised oil in the connection rates on the device (opmhip_set_std_wells_vaporised_oil, k_std_wells_eq<., VO = true>) against
wells.StandardWells(arithmetic="stated", vaporised_oil=True) on the same HipModel state, bit for bit.

Case: helpers.wetgas_case(pkg, 3, 3, 70, heterogeneous=True, dz=1.0), with and without ROCKTAB_2 - gas cap, three-phase zone, oil leg -
and decks.gas_condensate_wells: PLONG's 70 completions cross the 64-lane boundary, PCAP's single one sits beside it (GRAT target, ORAT
limit: the list has limits, so every run here is a LIM instantiation), GINJ injects gas.  The wells share no cell, so the operator's
atomics cannot reorder."""
import numpy as np
import pytest

import helpers
import std_wells_harness as H
import thp_cases
from std_wells_harness import same

pytestmark = pytest.mark.gpu

DAY = 86400.0


def make_case(pkg, rocktab=None):
    return helpers.wetgas_case(pkg, 3, 3, 70, rocktab=rocktab, heterogeneous=True, dz=1.0)


def assemble_and_compare(pkg, md, wd, mh, wh, iq, dt, it, what):
    """one assembly on both sides: the wells' arrays, the perforated cells' source rows, the reservoir's J and r -> the device's arrays.
    (Local: the solution rates and the source rows are this feature's own)"""
    wa = H.host_assemble(mh, wh, iq)
    jh, rh = mh.assemble(dt, it)
    jd, rd = md.assemble(dt, it)
    r, _, _, C, _, _ = wh._assemble_wells(iq)                            # (the same state: the same bits as inside assemble)
    assert np.array_equal(wa["res_well"].reshape(-1, 4), r) and np.array_equal(wa["wells"]["Cnnzs"].reshape(len(wh.cells), 4, 3), C)
    got = H.compare_wells(pkg, md, wh, wa, what, extra=("D", "rates", "dq"), iq=iq, all_finite=True)
    got["dissolved_gas"], got["vaporised_oil"] = wd.solution_rates()
    same(got["dissolved_gas"], wh.solution_rates()[0], (what, "dissolved_gas"))
    same(got["vaporised_oil"], wh.solution_rates()[1], (what, "vaporised_oil"))
    # the perforated cells' source and dsource rows (every cell has one perforation here), then the reservoir's J and r, which hold them
    order = [list(wh.cells).index(c) for c in wa["cells"]]
    same(got["rates"][order, :, 0], wa["source_cells"].reshape(-1, 3), (what, "source"))
    same(got["rates"][order, :, 1:4], wa["dsource_cells"].reshape(-1, 3, 3), (what, "dsource"))
    assert np.array_equal(jd, jh) and np.array_equal(rd, rh), what
    return got


def raw(C, model, on):
    rc = C.lib().opmhip_set_std_wells_vaporised_oil(model._h, int(on))
    return rc, C.lib().opmhip_last_error(model._h).decode()


# ---- a. one assembly ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rocktab", [None, helpers.ROCKTAB_2], ids=["plain", "rocktab"])
def test_one_assembly(pkg, rocktab):
    """the wells alone at iteration 0, then one assembly.  Without crossflow PLONG's reversed perforations are closed"""
    W = pkg.wells
    case = make_case(pkg, rocktab)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: pkg.decks.gas_condensate_wells(case), vfp=None, vaporised_oil=True)
    assert md.iq().shape[1] == 19 and list(np.diff(wh.vp)) == [70, 1, 5]
    iq = H.begin(wd, mh, wh, 0)
    same(md.get_std_wells()[0], wh.x, "the wells alone")
    got = assemble_and_compare(pkg, md, wd, mh, wh, iq, 5.0 * DAY, 0, "a")
    assert [w.control[0] for w in wh.wells] == ["rate", "orat", "rate"]           # PCAP's vaporised oil exceeds its ORAT limit
    assert got["rates"][70, W.OIL, 0] < 0.0 and got["vaporised_oil"][1] == got["rates"][70, W.OIL, 0]     # ... and is all its oil
    assert np.all(got["dissolved_gas"][[0]] < 0.0) and np.all(got["vaporised_oil"][:2] < 0.0)
    assert got["dissolved_gas"][2] == 0.0 and got["vaporised_oil"][2] == 0.0      # the injector
    assert not np.any(got["rates"][:70, :, 0] > 0.0) and np.all(got["dq"] == 0.0)


# ---- b. with crossflow -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rocktab", [None, helpers.ROCKTAB_2], ids=["plain", "rocktab"])
def test_one_assembly_with_crossflow(pkg, rocktab):
    """allow_crossflow on PLONG: the device's own well solve leaves reversed perforations, in the d = 1 - rv rs branch"""
    case = make_case(pkg, rocktab)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: pkg.decks.gas_condensate_wells(case, allow_crossflow=True), vfp=None, vaporised_oil=True)
    iq = H.begin(wd, mh, wh, 0)
    same(md.get_std_wells()[0], wh.x, "the wells alone")
    got = assemble_and_compare(pkg, md, wd, mh, wh, iq, 5.0 * DAY, 0, "b")
    reversed_ = (got["rates"][:70, :, 0] > 0.0).any(axis=1)
    assert reversed_.sum() >= 1 and np.any(got["dq"][:70][reversed_] != 0.0)
    print("reversed perforations of PLONG after the device's own solve:", np.flatnonzero(reversed_))
    assert np.array_equal(got["C"][:, :3, :], -got["dq"].transpose(0, 2, 1)) and not np.array_equal(got["D"][0, :3, :3], np.eye(3))


# ---- c. beside an LRAT and a THP limit ------------------------------------------------------------------------------------------------------------
def test_lrat_and_thp_limit_in_force(pkg):
    """PLONG with crossflow, an LRAT limit below its oil target and a THP limit (tests/thp_cases.py's VFPPROD 5): k_std_wells_eq<., CF, THP,
    LIM, VO>.  The controls after the wells alone put it under LRAT; the second assembly is under THP control, set on both sides"""
    W = pkg.wells
    case = make_case(pkg)
    kw = dict(allow_crossflow=True, limits={"lrat": 30.0 / DAY}, thp_limit=97e5, vfp_table=5)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: pkg.decks.gas_condensate_wells(case, **kw), vfp=thp_cases.tables(pkg), vaporised_oil=True)
    iq = H.begin(wd, mh, wh, 0)
    assert wh.wells[0].control == ("lrat", 30.0 / DAY)
    assemble_and_compare(pkg, md, wd, mh, wh, iq, 5.0 * DAY, 0, "lrat")
    t = wd.thp()
    same(t["dp"], wh.thp_dp, "thp dp")
    same(t["bhp_from_thp"], wh.bhp_from_thp, "bhp from thp")
    wh.wells[0].control = ("thp", 97e5)
    md.set_std_wells_state(control=[W.CONTROL_CODE[w.control[0]] for w in wh.wells])
    got = assemble_and_compare(pkg, md, wd, mh, wh, iq, 5.0 * DAY, 0, "thp")
    assert got["ctl"][0] == 2 and np.any(got["D"][0, 3, :3] != 0.0) and got["D"][0, 3, 3] == 1.0


# ---- d. two Newton iterations and a round trip through advance_time_level / update_failed ----------------------------------------------------------
def test_newton_iterations_and_a_given_up_step(pkg):
    case = make_case(pkg)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: pkg.decks.gas_condensate_wells(case, allow_crossflow=True), vfp=None, vaporised_oil=True, model_kw=dict(tolerance=1e-4))
    dt = 0.2 * DAY

    def same_everything(what):
        (pd, cd), (ph, ch) = md.get_state(), mh.get_state()
        assert np.array_equal(cd, ch), (what, "meanings")
        same(pd, ph, (what, "states"))
        x, ctl, _ = md.get_std_wells()
        same(x, wh.x, (what, "x"))
        assert list(ctl) == [pkg.wells.CONTROL_CODE[w.control[0]] for w in wh.wells], what

    H.begin(wd, mh, wh, 0)                         # a time level whose wells have flowed: what a given-up step goes back to
    for m in (md, mh):
        m.advance_time_level()
    saved = wh.state()
    x_saved = md.get_std_wells()[0]
    same(x_saved, wh.x, "x at the time level")
    for it in range(2):
        iq = H.begin(wd, mh, wh, it)
        wa = H.host_assemble(mh, wh, iq)
        mh.assemble(dt, it, fetch=False)
        md.assemble(dt, it, fetch=False)
        mh.wells_apply_residual(wa["wells"], wa["res_well"])
        md.std_wells_apply_residual()
        same(md.get_rhs(), mh.get_rhs(), (it, "rhs"))
        sh, sd = mh.solve_jacobian_system(wells=wa["wells"]), md.solve_jacobian_system()
        assert sh.converged and sd.converged and sd.it == sh.it
        wh.update(mh.wells_recover_solution(wa["wells"], wa["res_well"]), 1.0)
        wd.update(1.0)
        mh.update(None, 1.0)
        md.update(None, 1.0)
        same_everything(it)
        same(wd.solution_rates()[1], wh.solution_rates()[1], (it, "vaporised oil"))
    assert np.any(md.get_std_wells()[0] != x_saved)
    for m in (md, mh):                               # the step is given up: the state of the last advance_time_level, wells included
        m.update_failed()
    wh.set_state(saved)
    same_everything("given up")
    same(md.get_std_wells()[0], x_saved, "x restored")
    iq = H.begin(wd, mh, wh, 0)                    # ... and the retry starts as the first attempt did
    assemble_and_compare(pkg, md, wd, mh, wh, iq, 0.5 * dt, 0, "retry")


# ---- e. the switch off ---------------------------------------------------------------------------------------------------------------------------
def test_switch_off_computes_and_launches_what_it_did(pkg):
    """off: every array is the host form's with vaporised_oil=False - the dry-gas rates on this wet-gas case, both solution rates zero -, and
    a context that had the switch on and off again gives the bits of one that never saw the call; profile_get's launch counts per scope are
    the same with the switch on and off"""
    case = make_case(pkg)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: pkg.decks.gas_condensate_wells(case, allow_crossflow=True), vfp=None, vaporised_oil=False)
    iq = H.begin(wd, mh, wh, 0)
    same(md.get_std_wells()[0], wh.x, "the wells alone")
    got = assemble_and_compare(pkg, md, wd, mh, wh, iq, DAY, 0, "off")
    assert np.all(got["dissolved_gas"] == 0.0) and np.all(got["vaporised_oil"] == 0.0) and np.all(got["rates"][70, pkg.wells.OIL] == 0.0)
    seen = []
    for switch in ("never", "off", "on"):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        w = pkg.wells.DeviceStandardWells(pkg.decks.gas_condensate_wells(case, allow_crossflow=True), case["depth"], m)
        if switch != "never":
            m.set_std_wells_vaporised_oil(True)
            if switch == "off":
                m.set_std_wells_vaporised_oil(False)
        m.profile_enable(True)
        w.begin_iteration(0)
        j, r = m.assemble(DAY, 0)
        m.synchronize()
        formed = H.launch_counts(m)                             # the wells alone, the controls, the assembly: no linear solve yet
        blk = m.std_wells_blocks()
        res = m.solve_jacobian_system()
        w.update(1.0)
        m.update(None, 1.0)
        m.synchronize()
        seen.append(dict(formed=formed, counts=H.launch_counts(m), j=j, r=r, blk=blk, it=res.it, x=m.get_std_wells()[0],
                         state=m.get_state()[0]))
    never, off, on = seen
    assert never["formed"] == off["formed"] == on["formed"] and never["formed"]["assemble"] >= 5
    # (after the linear solve the solver's scopes follow its iteration count, which follows the matrix: the other scopes are compared)
    assert never["counts"] == off["counts"] and all(on["counts"][k] == never["counts"][k] for k in ("assemble", "iq_update", "convergence"))
    assert np.array_equal(never["j"], off["j"]) and np.array_equal(never["r"], off["r"]) and never["it"] == off["it"]
    assert all(np.array_equal(never["blk"][k], off["blk"][k]) for k in never["blk"])
    assert np.array_equal(never["x"], off["x"]) and np.array_equal(never["state"], off["state"])
    assert np.array_equal(never["blk"]["rates"], got["rates"])
    assert not np.array_equal(on["blk"]["rates"], never["blk"]["rates"])      # (and the switch did act)


# ---- f. refusals, and what replaces the list -------------------------------------------------------------------------------------------------------
def test_refusals_and_list_replacement(pkg):
    C = pkg.capi
    case = make_case(pkg)
    m = C.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    rc, msg = raw(C, m, 1)
    assert rc == C.NOT_READY and "no resident list" in msg                  # before a list
    dis, vap = m.std_wells_solution_rates()
    assert dis.size == 0 and vap.size == 0
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: pkg.decks.gas_condensate_wells(case, allow_crossflow=True), vfp=None, vaporised_oil=True)
    iq = H.begin(wd, mh, wh, 0)
    md.assemble(DAY, 0, fetch=False)
    blk0, sol0 = md.std_wells_blocks(), wd.solution_rates()
    assert np.all(sol0[1][:2] < 0.0)
    rc, msg = raw(C, md, 2)
    assert rc == C.INVALID_ARGUMENT and "on = 2" in msg
    rc, msg = raw(C, md, -1)
    assert rc == C.INVALID_ARGUMENT and "on = -1" in msg
    # the previous state is in force: the next assembly is the one before the refused calls
    md.assemble(DAY, 0, fetch=False)
    blk1, sol1 = md.std_wells_blocks(), wd.solution_rates()
    assert all(np.array_equal(blk0[k], blk1[k]) for k in blk0) and np.array_equal(sol0, sol1)
    assert C.lib().opmhip_get_std_wells_solution_rates(md._h, None, None) == C.SUCCESS      # either pointer may be NULL
    # a fluid without PVTG: the 17-field record
    dry = pkg.decks.cartesian_case(3, 3, 70, state="mixed", heterogeneous=True, dz=1.0)
    mdry = C.HipModel(dry)
    mdry.set_state(dry["pv"], dry["meaning"])
    wdry = pkg.wells.DeviceStandardWells(pkg.decks.gas_condensate_wells(dry), dry["depth"], mdry)
    assert mdry.iq().shape[1] == 17
    rc, msg = raw(C, mdry, 1)
    assert rc == C.INVALID_ARGUMENT and "no PVTG" in msg
    with pytest.raises(ValueError, match="no PVTG"):
        mdry.set_std_wells_vaporised_oil(True)
    with pytest.raises(ValueError, match="no PVTG"):
        pkg.wells.DeviceStandardWells(pkg.decks.gas_condensate_wells(dry), dry["depth"], mdry, vaporised_oil=True)
    wdry = pkg.wells.DeviceStandardWells(pkg.decks.gas_condensate_wells(dry), dry["depth"], mdry)
    wdry.begin_iteration(0)
    mdry.assemble(DAY, 0, fetch=False)                                       # the refused calls left the default model in force
    assert np.all(np.concatenate(wdry.solution_rates()) == 0.0) and np.all(np.isfinite(mdry.std_wells_blocks()["rates"]))
    # an accepted call makes the last assembly stale
    md.set_std_wells_vaporised_oil(False)
    with pytest.raises(C.OpmHipError) as e:
        md.solve_jacobian_system()
    assert e.value.code == C.NOT_READY
    md.set_std_wells_state(control=[0, 0, 0])                                # (PCAP off its ORAT limit: without the switch no oil rate answers to that row)
    md.assemble(DAY, 0, fetch=False)
    assert np.all(md.std_wells_blocks()["rates"][70, pkg.wells.OIL] == 0.0) and np.all(np.concatenate(wd.solution_rates()) == 0.0)
    # replacing the list clears the switch
    md.set_std_wells_vaporised_oil(True)
    wd2 = pkg.wells.DeviceStandardWells(pkg.decks.gas_condensate_wells(case, allow_crossflow=True), case["depth"], md)
    wd2.begin_iteration(0)
    md.assemble(DAY, 0, fetch=False)
    assert np.all(md.std_wells_blocks()["rates"][70, pkg.wells.OIL] == 0.0) and np.all(np.concatenate(wd2.solution_rates()) == 0.0)

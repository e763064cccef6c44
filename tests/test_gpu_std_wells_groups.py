"""Group production control of the device-resident standard wells (opmhip_set_std_wells_groups: GCONPROD targets shared by guide rate,
control 8 = GRUP) against wells.StandardWells(groups=, arithmetic="stated") on a second context in the same state, bit for bit: x, the
controls, r_w, D, D^-1, B, C, the rates and the group read-back.  The host form takes its averages from that context and 1/B from the
device's probes (capi.HipFluid).  tests/groups_cases.py, tests/limits_cases.py and tests/thp_cases.py hold the wells."""
import ctypes
import uuid

import numpy as np
import pytest

import groups_cases as GC
import limits_cases as LC
import std_wells_harness as H
import thp_cases
from std_wells_harness import moved

pytestmark = pytest.mark.gpu
DAY = 86400.0


def constructor_kw(case, groups, nupcol=3, vfp=None, matrix_add=False):
    """the constructors' keywords of this file: the tables (None: none), the groups and NUPCOL to both sides, the switch to the device's, the
    device's property functions and the case's PVT regions (None: one) to the host's"""
    return dict(vfp=vfp, groups=groups, nupcol=nupcol, matrix_add=matrix_add, props="always", pvtnum=case.get("pvtnum"))


def lockstep(pkg, case, make, groups, states, **kw):
    """the harness's, with the controls told the iteration and the groups compared -> the two pairs, the device's arrays of the last
    comparison; then what is this file's own: the controls and the convergence check of both sides"""
    (md, wd), (mh, wh), wa, blk = H.lockstep(pkg, case, make, states, extra=("D", "rates", "groups", "resv"), pass_iteration=True, **constructor_kw(case, groups, **kw))
    wd.fetch()
    assert [w.control for w in wd.wells] == [w.control for w in wh.wells]
    # getWellConvergence decides alike on both sides: the read-back carries the groups' modes in force, which tell a GRUP well's rate row
    # from its BHP row (the second pair of tolerances passes every rate row and no pressure row but an exact one)
    assert wd.group_mode == wh.group_mode and any(wh.group_mode)
    for tol_rate, tol_bhp in ((1e-7, 1.0), (1e30, 0.0), (1e30, 1.0)):
        assert wd.converged(tol_rate=tol_rate, tol_bhp=tol_bhp) == wh.converged(wa["res_well"], tol_rate=tol_rate, tol_bhp=tol_bhp), (tol_rate, tol_bhp)
    return (md, wd), (mh, wh), blk


# ---- 1. the SPE9-shaped list in three groups ---------------------------------------------------------------------------------------------------
def spe9(pkg):
    case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
    groups, assign = GC.spe9_groups(pkg)
    return case, (lambda: assign(pkg.decks.spe9_shaped_wells(case).wells)), (lambda: GC.spe9_groups(pkg)[0])


def test_spe9_shaped_list_in_three_groups(pkg):
    case, make, groups = spe9(pkg)
    (md, wd), (mh, wh), blk = lockstep(pkg, case, make, groups, [moved(case, 3)])
    modes = wh.group_mode
    print("group modes", modes, "controls", [w.control[0] for w in wh.wells])
    assert sorted(modes) == [1, 4, 5]                       # ORAT, LRAT and RESV: the three groups left NONE for different modes
    assert [len(g) for g in wh.group_wells] == [12, 11, 1] and wh.group_wells[0][:3] == [1, 3, 5] and wh.wells[25].group is None and wh.wells[0].group == 0
    for g, members in enumerate(wh.group_wells):
        assert any(wh.wells[k].control == ("grup",) for k in members), g
    assert wh.wells[25].control[0] != "grup" and wh.wells[0].control[0] != "grup"
    assert np.all(wh.resv_coeff[wh.group_wells[1]] != 0.0) and np.all(wh.resv_coeff[wh.group_wells[0]] == 0.0)
    assert wh.group_rates()["voidage"][1] > 0.0


# ---- 2. 70 wells: the groups' wells straddle lane 63 / 64 of the controls kernel -------------------------------------------------------------------
def seventy(pkg):
    case = pkg.decks.cartesian_case(6, 6, 3, state="mixed", heterogeneous=True)
    return case, (lambda: GC.seventy_producers(pkg, case)), (lambda: [pkg.wells.Group("G%d" % g, {"lrat": 1e-3, "orat": 1e9}) for g in range(5)])


def test_seventy_producers_in_five_groups(pkg):
    case, make, groups = seventy(pkg)
    (md, wd), (mh, wh), blk = lockstep(pkg, case, make, groups, [moved(case, 5, 1e5)])
    assert wh.nw == 70 and all(min(g) < 63 and max(g) > 64 for g in wh.group_wells)
    late = [k for k in range(64, 70) if wh.wells[k].control == ("grup",)]
    print("wells 64 .. 69 under GRUP", late, "modes", wh.group_mode)
    assert late and wh.group_mode == [4] * 5
    assert all(w.control == ("grup",) for w in wh.wells) and wd.converged(tol_rate=1e30, tol_bhp=0.0)     # every control row is a rate row


# ---- 3. beside a THP limit, a further LRAT limit and crossflow; with the matrix-add form ------------------------------------------------------------
def test_groups_beside_thp_lrat_and_crossflow(pkg):
    case = thp_cases.make_case(pkg)
    tabs = thp_cases.tables(pkg)

    def make():
        p = LC.producer(pkg, case, None, {"lrat": 39.0 / DAY, "grat": 1.0}, thp_limit=thp_cases.PROD_LIMIT)
        p.allow_crossflow = True
        p.group, p.guide_rate = 0, np.full(5, 2.0)
        i = LC.injector(pkg, case, None, {"resv": 70.0 / DAY}, thp_limit=thp_cases.INJ_LIMIT)
        p2 = LC.producer(pkg, case, None, {}, cells=thp_cases.column(1, 1, [30, 31]), name="P2", scale=1.0, own=("rate", pkg.wells.OIL, 2.0 / DAY))
        p2.group, p2.guide_rate = 0, np.full(5, 1.0)
        return [p, i, p2]
    groups = lambda: [pkg.wells.Group("G", {"resv": 1.5 / DAY, "orat": 1e9})]
    (md, wd), (mh, wh), blk = lockstep(pkg, case, make, groups, [moved(case, 3), moved(case, 4, 4e5)], vfp=tabs)
    print("controls", [w.control[0] for w in wh.wells], "mode", wh.group_mode)
    t = md.std_wells_thp()
    assert np.array_equal(t["thp"], wh.thp_current) and np.array_equal(t["dp"], wh.thp_dp) and np.array_equal(t["bhp_from_thp"], wh.bhp_from_thp)
    assert np.array_equal(md.std_wells_rate_dq(), wh.rate_dq)
    assert wh.group_mode == [5] and any(w.control == ("grup",) for w in wh.wells)      # the RESV row under GRUP in the THP + LIM + CF instantiation


def test_groups_with_the_matrix_add_form(pkg):
    import test_gpu_std_wells_matrix_add as MA
    plain = pkg.decks.cartesian_case(6, 5, 4, state="mixed", heterogeneous=True)
    case = pkg.decks.with_well_cliques(plain, MA.make_wells(pkg, plain))

    def make():
        wells = MA.make_wells(pkg, case)
        for n, w in enumerate(wells):
            w.group, w.guide_rate = n % 2, np.full(5, 1.0 + n)
        return wells
    groups = lambda: [pkg.wells.Group("GA", {"orat": 2.5 / DAY}), pkg.wells.Group("GB", {"lrat": 1.0 / DAY})]
    (md, wd), (mh, wh), blk = lockstep(pkg, case, make, groups, [moved(case, 7, 1e5)], matrix_add=True)
    assert any(w.control == ("grup",) for w in wh.wells)
    md.std_wells_apply_residual()
    md.std_wells_add_to_matrix()
    res = md.solve_jacobian_system()
    wd.update(1.0)
    assert res.converged and md.std_wells_matrix_add_info()["in_matrix"] and np.all(np.isfinite(md.std_wells_blocks()["xw"]))


# ---- 4. a time step given up ---------------------------------------------------------------------------------------------------------------------
def test_a_given_up_time_step_restores_the_groups(pkg):
    case, make, groups = spe9(pkg)
    (md, wd), (mh, wh) = H.pair(pkg, case, make, **constructor_kw(case, groups, nupcol=2))
    dt = 2.0 * DAY

    def change(seed, dp):
        rng = np.random.default_rng(seed)
        dx = np.zeros((case["Nb"], 3))
        dx[:, 1] = dp * rng.uniform(0.0, 1.0, case["Nb"])
        dx[:, 0] = rng.uniform(-0.01, 0.01, case["Nb"])
        return np.ascontiguousarray(dx.reshape(-1))

    def both_iterations(changes, what):
        first = None
        for it, dx in enumerate(changes):
            if dx is not None:
                for m in (md, mh):
                    m.update(dx)
            wa = H.host_begin_and_assemble(mh, wh, it, pass_iteration=True)
            mh.assemble(dt, it, fetch=False)
            wd.begin_iteration(it)
            md.assemble(dt, it, fetch=False)
            blk = H.compare_wells(pkg, md, wh, wa, (what, it), extra=("D", "rates", "groups", "resv"), mh=mh)
            if it == 0:
                first = (blk["x"].copy(), blk["Dinv"].copy(), md.std_wells_groups())
        return first
    for m in (md, mh):
        m.advance_time_level()
    both_iterations([None, change(1, 1e5), change(3, 1e5), change(4, 1e5)], "step 1")       # iterations 0 .. 3 with nupcol = 2: the copy stops, then the check
    for m in (md, mh):
        m.advance_time_level()
    saved = wh.state()
    g_saved = md.std_wells_groups()
    wh.group_mode[2] = 0                                     # both sides forget a mode, so that the given-up attempt changes one again
    md.set_std_wells_group_targets(mode=wh.group_mode)
    first_try = both_iterations([None, change(2, 6e5)], "step 2, given up")
    g_try = md.std_wells_groups()
    assert not np.array_equal(g_try["nupcol_rates"], g_saved["nupcol_rates"]) and list(g_try["mode"]) != list(g_saved["mode"][:2]) + [0]
    for m in (md, mh):
        m.update_failed()
    wh.set_state(saved)
    wd.fetch()
    g_back = md.std_wells_groups()
    assert list(g_back["mode"]) == list(g_saved["mode"]) == saved[-1]["group_mode"] and np.array_equal(g_back["nupcol_rates"], g_saved["nupcol_rates"])
    assert [w.control for w in wd.wells] == [w.control for w in wh.wells] and np.array_equal(wd.x, wh.x)
    wh.group_mode[2] = 0
    md.set_std_wells_group_targets(mode=wh.group_mode)
    retry = both_iterations([None], "step 2, retry")
    assert np.array_equal(retry[0], first_try[0]) and np.array_equal(retry[1], first_try[1])
    for k in first_try[2]:
        assert np.array_equal(retry[2][k], first_try[2][k]), k


# ---- 5. every refusal through the C ABI --------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(pkg):
    case = thp_cases.make_case(pkg)
    inf = np.inf

    def fresh():
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        wells = [LC.producer(pkg, case, None, {}, cells=thp_cases.column(1, 1, [30, 31]), name="A", scale=1.0), LC.injector(pkg, case, None, {}),
                 LC.producer(pkg, case, None, {}, cells=thp_cases.column(0, 1, [30, 31]), name="B", scale=1.0),
                 LC.producer(pkg, case, None, {}, cells=thp_cases.column(2, 1, [30, 31]), name="C", scale=1.0)]
        return m, pkg.wells.DeviceStandardWells(wells, case["depth"], m)
    good = dict(num_groups=2, well_group=[0, 0, 1, -1], oil_target=[1.0, inf], liquid_target=[inf, 2.0], mode=[1, 0], guide_rate=np.ones((4, 5)),
                available=[1, 1, 0, 1], nupcol=3)
    m, wd = fresh()

    def refused(call, *words, code=pkg.capi.INVALID_ARGUMENT):
        with pytest.raises(pkg.capi.OpmHipError) as e:
            call()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
    refused(lambda: m.set_std_wells_guide_rates(np.ones((4, 5))), "no groups in force", code=pkg.capi.NOT_READY)
    refused(lambda: m.set_std_wells_state(None, [8, 1, 0, 0], None), "control[0] = 8", "without groups")
    m.set_std_wells_groups(good)
    before = m.std_wells_groups()
    for change, words in ((dict(well_group=[0, 0, 2, -1]), ["outside [-1, 2)"]), (dict(well_group=[-2, 0, 1, -1]), ["outside [-1, 2)"]),
                          (dict(oil_target=[np.nan, inf]), ["not > 0"]), (dict(liquid_target=[-inf, 2.0]), ["not > 0"]), (dict(oil_target=[0.0, inf]), ["not > 0"]),
                          (dict(mode=[4, 0]), ["has no such target"]), (dict(mode=[1, 6]), ["mode[1] = 6"]), (dict(guide_rate=-np.ones((4, 5))), ["negative or not finite"]),
                          (dict(guide_rate=np.full((4, 5), inf)), ["negative or not finite"]), (dict(available=[1, 2, 0, 1]), ["(0 / 1)"]), (dict(nupcol=-1), ["nupcol = -1"]),
                          (dict(num_groups=-1), ["num_groups = -1"])):
        t = dict(good, **change)
        if "num_groups" in change:                           # (the binding sizes the arrays by num_groups: hand the struct over directly)
            s, keep = pkg.capi.make_std_wells_groups(good, 4)
            s.num_groups = -1
            refused(lambda: m._check(pkg.capi.lib().opmhip_set_std_wells_groups(m._h, ctypes.byref(s))), *words)
        else:
            refused(lambda: m.set_std_wells_groups(t), "set_std_wells_groups", *words)
    after = m.std_wells_groups()
    assert all(np.array_equal(before[k], after[k]) for k in before)        # the previous values are in force
    m.set_std_wells_groups(dict(good, mode=[1, 4]))
    assert list(m.std_wells_groups()["mode"]) == [1, 4]
    # control 8: an available producer in a group
    for ctl, word in (([0, 8, 0, 0], "for an injector"), ([0, 0, 8, 0], "not available"), ([0, 0, 0, 8], "without a group"), ([9, 0, 0, 0], "control[0] = 9")):
        refused(lambda: m.set_std_wells_state(None, ctl, None), "set_std_wells_state", word)
    m.set_std_wells_state(None, [8, 1, 0, 0], None)
    assert list(m.get_std_wells()[1]) == [8, 1, 0, 0]
    refused(lambda: m.set_std_wells_groups(None), "cannot be removed")
    refused(lambda: m.set_std_wells_groups(dict(good, well_group=[-1, 0, 1, -1])), "under control 8")
    refused(lambda: m.set_std_wells_groups(dict(good, available=[0, 1, 0, 1])), "under control 8")
    # the events
    refused(lambda: m.set_std_wells_guide_rates(-np.ones((4, 5))), "set_std_wells_guide_rates", "negative or not finite")
    refused(lambda: m.set_std_wells_group_targets(oil=[inf, inf]), "set_std_wells_group_targets", "has no such target")
    refused(lambda: m.set_std_wells_group_targets(mode=[2, 0]), "has no such target")
    refused(lambda: m.set_std_wells_group_targets(resv=[np.nan, 1.0]), "not > 0")
    m.set_std_wells_guide_rates(2.0 * np.ones((4, 5)))
    m.set_std_wells_group_targets(water=[3.0, inf], mode=[2, 0])
    assert list(m.std_wells_groups()["mode"]) == [2, 0]
    # the list replaced: the groups are gone with it
    m.set_std_wells_state(None, [0, 1, 0, 0], None)
    m.set_std_wells_groups(None)
    refused(lambda: m.set_std_wells_state(None, [8, 1, 0, 0], None), "without groups")
    m2, wd2 = fresh()
    m2.set_std_wells_groups(good)
    assert list(m2.std_wells_groups()["mode"]) == [1, 0]
    s2, keep2 = pkg.capi.make_std_wells_groups(good, 4)
    m2.set_std_wells(None)
    refused(lambda: m2._check(pkg.capi.lib().opmhip_set_std_wells_groups(m2._h, ctypes.byref(s2))), "no resident list", code=pkg.capi.NOT_READY)
    # a decomposed context (loopback, two ranks) is refused as the list itself is, and told so rather than "no resident list"
    sub = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    dd = pkg.capi.HipModel(sub, comm=("loopback", 2, 0, "swg" + uuid.uuid4().hex), reorder="level_scheduling")
    dd.set_state(sub["pv"], sub["meaning"])
    refused(lambda: dd._check(pkg.capi.lib().opmhip_set_std_wells_groups(dd._h, ctypes.byref(s2))), "set_std_wells_groups", "decomposed context (2 ranks)")
    refused(lambda: dd._check(pkg.capi.lib().opmhip_set_std_wells_groups(dd._h, None)), "decomposed context")


# ---- 6. the launches -------------------------------------------------------------------------------------------------------------------------
def test_launch_counts_with_and_without_groups(pkg):
    """opmhip_profile_get's assembly class counts one scope per launcher.  A list without groups counts what a context built without the new
    call counts; with groups the count of an iteration depends neither on the wells nor on the groups (25 wells in 3 groups, 70 in 5)."""
    def count(case, wells, groups):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        wd = pkg.wells.DeviceStandardWells(wells, case["depth"], m, groups=groups)
        m.profile_enable(True)
        wd.begin_iteration(0)
        m.assemble(DAY, 0, fetch=False)
        m.synchronize()
        first = m.profile()["assemble"][0]
        wd.begin_iteration(1)
        m.assemble(DAY, 1, fetch=False)
        m.synchronize()
        return first, m.profile()["assemble"][0] - first
    case, make, groups = spe9(pkg)
    plain = pkg.decks.spe9_shaped_wells(case).wells
    counts = dict(never=count(case, plain, None), no_wells_named=count(case, pkg.decks.spe9_shaped_wells(case).wells, [pkg.wells.Group("G", {"orat": 1.0})]))
    lrat_only = lambda: [pkg.wells.Group("G%d" % g, {"lrat": 1e-3}) for g in range(3)]
    counts["spe9_3_groups_no_resv"] = count(case, make(), lrat_only())
    counts["spe9_3_groups"] = count(case, make(), groups())
    c70, make70, groups70 = seventy(pkg)
    counts["seventy_5_groups"] = count(c70, make70(), groups70())
    print("assembly-class scopes (time step's first iteration, a later iteration):", counts)
    assert counts["never"] == counts["no_wells_named"]
    assert counts["spe9_3_groups_no_resv"] == counts["seventy_5_groups"]
    assert counts["spe9_3_groups"][1] == counts["seventy_5_groups"][1] == counts["never"][1] + 2
    assert counts["spe9_3_groups_no_resv"][0] == counts["never"][0] + 3 and counts["spe9_3_groups"][0] == counts["never"][0] + 4

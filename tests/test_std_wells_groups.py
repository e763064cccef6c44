"""Group production control of wells.StandardWells (groups=, nupcol=; GCONPROD / GRUP) on the CPU over the oracle, the host form only:
the shares by guide rate, the reduction of a well that cannot hold its share, the order of the groups' modes, NUPCOL, the single-well
cases, and a list without groups against the arrays it gave before.

Tolerance of the closed-form shares: what converged() uses - tol_rate = 1e-7 relative to the well's largest rate - times the number of
wells in the sum (each well's control equation is met to the wells-alone solve's stopping test, far below it)."""
import numpy as np
import pytest

import limits_cases as LC
import oracle_bind
import thp_cases

TOL_RATE = 1e-7


@pytest.fixture(scope="module")
def setup(pkg, orc):
    case = thp_cases.make_case(pkg)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    return dict(case=case, iq=om.iq(), props=oracle_bind.OracleFluid(orc, case["fluid"]), model=om)


def prod(pkg, case, name, group=0, guide=1.0, scale=1.0, available=True, cells=None, grup=False):
    """a producer at its BHP limit (free flow), its own oil target out of reach; grup: it starts under GRUP"""
    cells = thp_cases.column(1, 1, [30, 31, 32]) if cells is None else cells
    w = LC.producer(pkg, case, ("bhp", thp_cases.PROD_BHP_LIMIT), {}, own=("rate", pkg.wells.OIL, LC.NEVER), cells=cells, name=name, scale=scale)
    w.group, w.guide_rate, w.available_for_group_control = group, np.full(5, float(guide)), available
    if grup:
        w.control = ("grup",)
    return w


def build(pkg, setup, wells, groups, nupcol=3):
    return pkg.wells.StandardWells(wells, setup["case"]["depth"], arithmetic="stated", groups=groups, nupcol=nupcol)


def settle(ws, iq, rounds=6):
    """time steps at a frozen reservoir: the wells alone, the controls, the wells alone again"""
    ws.calculate_explicit_quantities(iq)
    ws.solve_well_equations(iq)
    for _ in range(rounds):
        ws.update_well_controls(0)
        ws.solve_well_equations(iq)
    return ws


def free_flow(pkg, setup, scale=1.0):
    ws = build(pkg, setup, [prod(pkg, setup["case"], "F", group=None, scale=scale)], None)
    ws.calculate_explicit_quantities(setup["iq"])
    ws.solve_well_equations(setup["iq"])
    assert ws.x[0, pkg.wells.OIL] < 0.0
    return -ws.x[0, pkg.wells.OIL]


# ---- 1. the shares ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guides", [(1.0, 1.0), (1.0, 3.0)], ids=["even", "uneven"])
def test_two_equal_producers_share_the_target_by_guide_rate(pkg, setup, guides):
    W, case = pkg.wells, setup["case"]
    q = free_flow(pkg, setup)
    target = 0.5 * (2.0 * q)
    ws = settle(build(pkg, setup, [prod(pkg, case, "A", guide=guides[0]), prod(pkg, case, "B", guide=guides[1])], [W.Group("G", {"orat": target})]), setup["iq"])
    assert [w.control for w in ws.wells] == [("grup",), ("grup",)] and ws.group_mode == [W.GROUP_MODES.index("orat")]
    got = -ws.x[:, W.OIL]
    want = target * np.array(guides) / sum(guides)
    print("shares", got, "want", want)
    for k in range(2):
        assert abs(got[k] - want[k]) <= TOL_RATE * np.abs(ws.x[k, :3]).max(), k
    assert abs(got.sum() - target) <= 2 * TOL_RATE * np.abs(ws.x[:, :3]).max()
    rec = ws.group_rates()
    assert rec["guide_sum"][0] == sum(guides) and np.all(rec["reduction"] == 0.0) and rec["mode"][0] == 1
    assert ws.converged(ws._assemble_wells(setup["iq"])[0])


def test_a_bhp_limited_well_keeps_its_rate_and_the_other_takes_the_rest(pkg, setup):
    W, case = pkg.wells, setup["case"]
    q1, q2 = free_flow(pkg, setup), free_flow(pkg, setup, scale=0.1)
    target = 0.6 * q1
    assert q2 < 0.75 * target and q1 + q2 > target              # the second well cannot hold its share of 3/4
    ws = settle(build(pkg, setup, [prod(pkg, case, "A", guide=1.0), prod(pkg, case, "B", guide=3.0, scale=0.1)], [W.Group("G", {"orat": target})]), setup["iq"])
    assert ws.wells[0].control == ("grup",) and ws.wells[1].control == ("bhp", thp_cases.PROD_BHP_LIMIT)
    got = -ws.x[:, W.OIL]
    print("rates", got, "free flow of the second", q2, "target", target)
    assert abs(got[1] - q2) <= TOL_RATE * np.abs(ws.x[1, :3]).max()
    assert abs(got[0] - (target - got[1])) <= 2 * TOL_RATE * np.abs(ws.x[:, :3]).max()       # the reduction at work
    rec = ws.group_rates()
    assert rec["guide_sum"][0] == 1.0 and rec["reduction"][0, W.OIL] == -ws.nupcol_rates[1, W.OIL] == got[1]


# ---- 2. the order of the modes ---------------------------------------------------------------------------------------------------------------
def test_of_two_violated_group_targets_the_earlier_mode_wins(pkg, setup):
    W, case = pkg.wells, setup["case"]
    modes = W.GROUP_MODES
    for start, targets, winner in (("none", {"orat": LC.ALWAYS, "lrat": LC.ALWAYS, "wrat": LC.NEVER}, "orat"),
                                   ("orat", {"orat": LC.ALWAYS, "wrat": LC.ALWAYS, "lrat": LC.ALWAYS}, "wrat"),
                                   ("none", {"grat": LC.ALWAYS, "lrat": LC.ALWAYS, "orat": LC.NEVER, "wrat": LC.NEVER}, "grat"),
                                   ("lrat", {"lrat": LC.ALWAYS, "orat": LC.NEVER}, "lrat")):
        ws = build(pkg, setup, [prod(pkg, case, "A", available=False)], [W.Group("G", targets, mode=start)])
        ws.calculate_explicit_quantities(setup["iq"])
        ws.solve_well_equations(setup["iq"])
        assert np.all(ws.x[0, :3] < 0.0)
        ws.update_well_controls(0)
        assert modes[ws.group_mode[0]] == winner, (start, targets)


def test_a_switching_group_scales_its_wells_under_grup(pkg, setup):
    W, case = pkg.wells, setup["case"]
    ws = build(pkg, setup, [prod(pkg, case, "A", grup=True), prod(pkg, case, "B", available=False)], [W.Group("G", {"lrat": 1e-4})])
    ws.x[:] = [[-3e-4, -1e-4, -2e-2, 2e7], [-1e-4, -1e-4, -1e-2, 3e7]]
    before = ws.x.copy()
    ws._group_check(0)
    current = (3e-4 + 1e-4) + (1e-4 + 1e-4)
    assert ws.group_mode == [4]
    assert np.array_equal(ws.x[0, :3], before[0, :3] * (1e-4 / current)) and np.array_equal(ws.x[1], before[1]) and ws.x[0, 3] == before[0, 3]


# ---- 3. NUPCOL -------------------------------------------------------------------------------------------------------------------------------
def test_nupcol(pkg, setup):
    W, case = pkg.wells, setup["case"]
    ws = build(pkg, setup, [prod(pkg, case, "A", available=False)], [W.Group("G", {"orat": LC.ALWAYS})], nupcol=2)
    x0 = np.array([-3e-4, -1e-5, -2e-2, 3e7])
    ws.x[0] = x0
    ws.update_well_controls(3)                                  # iteration > nupcol: the group's check does not run
    assert ws.group_mode == [0] and np.all(ws.nupcol_rates == 0.0)
    ws.update_well_controls(1)                                  # iteration < nupcol: the rates are copied
    assert ws.group_mode == [1] and np.array_equal(ws.nupcol_rates[0], x0[:3])
    ws.group_mode = [0]
    ws.x[0, :3] = 2.0 * x0[:3]
    ws.update_well_controls(2)                                  # iteration == nupcol: the check still runs, the copy has stopped
    assert ws.group_mode == [1] and np.array_equal(ws.nupcol_rates[0], x0[:3])
    assert np.array_equal(ws.group_rates()["reduction"][0], -x0[:3]) and np.array_equal(ws.group_rates()["rates"][0], -2.0 * x0[:3])
    with pytest.raises(ValueError, match="nupcol"):
        build(pkg, setup, [prod(pkg, case, "A")], [W.Group("G", {})], nupcol=-1)


# ---- 4. single wells -------------------------------------------------------------------------------------------------------------------------
def test_a_well_under_grup_in_a_group_without_a_mode_gets_the_bhp_row(pkg, setup):
    W, case = pkg.wells, setup["case"]
    ws = build(pkg, setup, [prod(pkg, case, "A", grup=True)], [W.Group("G", {"orat": LC.NEVER})])
    ws.calculate_explicit_quantities(setup["iq"])
    ws.x[0] = [-3e-4, -1e-5, -2e-2, 2.1e7]
    r, g = ws._control_rows()
    assert r[0] == 2.1e7 - thp_cases.PROD_BHP_LIMIT and np.array_equal(g[0], [0.0, 0.0, 0.0, 1.0])
    assert ws.converged(np.array([[0.0, 0.0, 0.0, 0.5]])) and not ws.converged(np.array([[0.0, 0.0, 0.0, 2.0]]))       # in the pressure's unit


def test_an_unavailable_well_never_goes_under_grup(pkg, setup):
    W, case = pkg.wells, setup["case"]
    ws = settle(build(pkg, setup, [prod(pkg, case, "A", available=False), prod(pkg, case, "B")], [W.Group("G", {"orat": LC.ALWAYS})]), setup["iq"], rounds=3)
    assert ws.wells[0].control[0] == "bhp" and ws.wells[1].control == ("grup",) and ws.group_mode == [1]
    with pytest.raises(ValueError, match="GRUP"):
        build(pkg, setup, [prod(pkg, case, "A", available=False, grup=True)], [W.Group("G", {})])
    with pytest.raises(ValueError, match="GRUP"):
        build(pkg, setup, [prod(pkg, case, "A", group=None, grup=True)], [W.Group("G", {})])
    with pytest.raises(ValueError, match="outside"):
        build(pkg, setup, [prod(pkg, case, "A", group=1)], [W.Group("G", {})])


def test_a_guide_rate_sum_of_zero_gives_the_target_rate_zero(pkg, setup):
    W, case = pkg.wells, setup["case"]
    ws = build(pkg, setup, [prod(pkg, case, "A", guide=0.0, grup=True)], [W.Group("G", {"orat": 1e-4}, mode="orat")])
    ws.calculate_explicit_quantities(setup["iq"])
    ws.x[0] = [-3e-4, -1e-5, -2e-2, 2.1e7]
    with np.errstate(all="raise"):
        ws._group_data(0)
        r, g = ws._control_rows()
        assert ws.group_rates()["guide_sum"][0] == 0.0
        assert r[0] == -3e-4 + 0.0 and np.array_equal(g[0], [1.0, 0.0, 0.0, 0.0])
        ws.wells[0].control = ("bhp", ws.wells[0].bhp_limit)     # ... and the well's group check: fraction 0, target_rate 1e-12
        ws._group_data(0)
        assert ws._well_group_check(0) and ws.wells[0].control == ("grup",)
    assert np.array_equal(ws.x[0, :3], np.array([-3e-4, -1e-5, -2e-2]) * (1e-12 / 3e-4))


def test_group_and_well_arguments_are_checked(pkg, setup):
    W = pkg.wells
    for bad in ({"orat": 0.0}, {"lrat": -1.0}, {"resv": float("nan")}, {"crat": 1.0}):
        with pytest.raises(ValueError):
            W.Group("G", bad)
    with pytest.raises(ValueError, match="mode"):
        W.Group("G", {"orat": 1.0}, mode="lrat")
    assert W.Group("G", {"orat": np.inf, "lrat": 2.0}).targets == {"lrat": 2.0}
    for bad in (-1.0, np.inf, [1.0, 2.0]):
        with pytest.raises(ValueError, match="guide_rate"):
            W.Well("A", [0], [1.0], 0.0, True, ("bhp", 1e7), 1e7, rate_control=("rate", 0, 1.0), group=0, guide_rate=bad)
    assert W.GRUP_CODE == 8 and W.control_code(("grup",)) == 8 and W.control_code(("lrat", 1.0)) == 6 and "grup" not in W.CONTROL_CODE


# ---- 5. a list without groups ----------------------------------------------------------------------------------------------------------------
def test_without_groups_the_spe9_shaped_list_gives_the_arrays_of_before(pkg, orc):
    case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    W = pkg.wells
    plain = pkg.decks.spe9_shaped_wells(case)
    assert plain.groups == [] and all(w.group is None for w in plain.wells)
    lists = dict(plain=W.StandardWells(plain.wells, case["depth"], arithmetic="stated"),
                 empty=W.StandardWells(pkg.decks.spe9_shaped_wells(case).wells, case["depth"], arithmetic="stated", groups=[]))
    inert = pkg.decks.spe9_shaped_wells(case, groups=dict(count=3, kind="lrat", target_stb_day=1e12))     # groups whose targets nothing reaches
    lists["inert"] = W.StandardWells(inert.wells, case["depth"], arithmetic="stated", groups=inert.groups, nupcol=inert.nupcol)
    assert [w.group for w in inert.wells[:5]] == [None, 0, 1, 2, 0] and inert.group_wells[0][:3] == [1, 4, 7]
    out = {}
    for name, ws in lists.items():
        ws.calculate_explicit_quantities(iq)
        ws.solve_well_equations(iq)
        ws.update_well_controls(0)
        a = ws.assemble(iq)
        out[name] = (ws.x.copy(), [w.control for w in ws.wells], a["res_well"], a["wells"]["Dnnzs"], a["wells"]["Bnnzs"], a["wells"]["Cnnzs"], a["source_cells"], ws.state())
    assert len(out["plain"][-1]) == 2                           # the state of a list without groups has the entries it had
    for name in ("empty", "inert"):
        for k in range(7):
            assert out[name][k] == out["plain"][k] if k == 1 else np.array_equal(out[name][k], out["plain"][k]), (name, k)
    st = lists["inert"].state()
    assert st[-1]["group_mode"] == [0, 0, 0] and np.array_equal(st[-1]["nupcol_rates"][1:], lists["inert"].x[1:, :3]) and np.all(st[-1]["nupcol_rates"][0] == 0.0)
    lists["inert"].group_mode = [4, 0, 0]
    lists["inert"].set_state(st)
    assert lists["inert"].group_mode == [0, 0, 0]

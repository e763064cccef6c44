"""Several rate limits per device-resident standard well (opmhip_set_std_wells_limits: ORAT, WRAT, GRAT, LRAT, RESV) against
wells.StandardWells(arithmetic="stated") on a second context in the same state, bit for bit.  The host form takes its averages from
that context (HipModel.reservoir_averages: the device's own, read back) and 1/B from the device's probes (capi.HipFluid).
tests/limits_cases.py and tests/thp_cases.py hold the wells."""
import numpy as np
import pytest

import limits_cases as LC
import std_wells_harness as H
import thp_cases
from std_wells_harness import moved

pytestmark = pytest.mark.gpu
DAY = 86400.0


def constructor_kw(case, head_model="cell_oil", vfp=None):
    """the constructors' keywords of this file: the head model and the tables (None: none) to both sides, the device's property functions
    and the case's PVT regions (None: one) to the host's"""
    return dict(head_model=head_model, vfp=vfp, props="always", pvtnum=case.get("pvtnum"))


def lockstep(pkg, case, make, states, **kw):
    """the harness's, with this file's keywords and compared keys -> the two pairs, the device's arrays of the last comparison"""
    (md, wd), (mh, wh), wa, blk = H.lockstep(pkg, case, make, states, extra=("D", "resv", "resv_current"), **constructor_kw(case, **kw))
    return (md, wd), (mh, wh), blk


# ---- 1. one producer per mode, an injector under RESV, a well of 65 completions ----------------------------------------------------------------
def per_mode_wells(pkg, case):
    P = lambda name, ij, ks, control, limits, **kw: LC.producer(pkg, case, control, limits, use_list_target=False, cells=thp_cases.column(*ij, ks), name=name, **kw)
    q = 40.0 / DAY
    return [P("P65", (0, 0), range(65), ("resv", 45.0 / DAY), {"resv": 45.0 / DAY, "lrat": 1.0}),
            P("PO", (1, 0), [20, 21, 22], ("orat", 0.05 * q), {"orat": 0.05 * q}, scale=1.0),
            P("PW", (2, 0), [20, 21, 22], ("wrat", 1e-12), {"wrat": 1e-12, "grat": 1.0}, scale=1.0),
            P("PG", (0, 1), [30, 31, 32], ("grat", 10.0 * q), {"grat": 10.0 * q}, scale=1.0),
            P("PL", (1, 1), [30, 31], ("lrat", 0.04 * q), {"lrat": 0.04 * q, "resv": 1.0}, scale=1.0),
            LC.injector(pkg, case, ("resv", 55.0 / DAY), {"resv": 55.0 / DAY}, use_list_target=False)]


def test_one_producer_per_mode_and_an_injector_under_resv(pkg):
    case = thp_cases.make_case(pkg)
    lockstep(pkg, case, lambda: per_mode_wells(pkg, case), [moved(case, 3), moved(case, 4, 0.5e5)])     # (against the moved reservoir some wells stop flowing: the guard's row)
    (md, wd), (mh, wh), blk = lockstep(pkg, case, lambda: per_mode_wells(pkg, case), [])
    modes = [w.control[0] for w in wh.wells]
    assert modes == ["resv", "orat", "wrat", "grat", "lrat", "resv"] and [w.control for w in wd.wells] == [w.control for w in wh.wells]
    assert list(np.diff(wh.vp)) == [65, 3, 3, 3, 2, 3]
    D, c = blk["D"], md.std_wells_resv()["coeff"]
    assert np.array_equal(D[0, 3, :3], c[0]) and np.all(c[0] != 0.0) and D[0, 3, 3] == 0.0
    assert np.array_equal(D[1, 3], [1, 0, 0, 0]) and np.array_equal(D[2, 3], [0, 1, 0, 0]) and np.array_equal(D[3, 3], [0, 0, 1, 0]) and np.array_equal(D[4, 3], [1, 1, 0, 0])
    assert np.array_equal(D[5, 3], [0, c[5, 1], 0, 0]) and c[5, 1] > 0.0
    assert np.all(c[[1, 2, 3]] == 0.0) and np.all(c[4] != 0.0)       # coefficients for the wells that have a RESV limit, whatever their control


def test_the_wells_alone_reach_their_limits_on_the_device(pkg):
    case = thp_cases.make_case(pkg)
    (md, wd), (mh, wh) = H.pair(pkg, case, lambda: per_mode_wells(pkg, case), **constructor_kw(case))
    H.host_begin(mh, wh, 0)
    wd.begin_iteration(0)
    x = wd.fetch()
    assert np.array_equal(x, wh.x)
    W = pkg.wells
    c = md.std_wells_resv()["coeff"]
    lim = [w.control[1] for w in wh.wells]
    combo = [-((c[0, 1] * x[0, 1] + c[0, 0] * x[0, 0]) + c[0, 2] * x[0, 2]), -x[1, W.OIL], -x[2, W.WATER], -x[3, W.GAS], -(x[4, W.OIL] + x[4, W.WATER]), c[5, 1] * x[5, 1]]
    print("controlled combinations", combo, "limits", lim)
    for k in range(6):
        assert abs(combo[k] - lim[k]) <= 1e-7 * max(np.abs(x[k, :3]).max(), 1e-9) * max(1.0, np.abs(c[k]).max()), k


# ---- 2. two wells in one cell, two PVT regions, crossflow and a THP limit beside the limits ------------------------------------------------------------
def test_two_wells_in_one_cell(pkg):
    """the two wells' shared cells are compared in what the non-atomic kernels form: the wells' blocks and the assembled J and r"""
    case = thp_cases.make_case(pkg)
    q = 40.0 / DAY

    def make():
        return [LC.producer(pkg, case, ("lrat", 0.03 * q), {"lrat": 0.03 * q}, use_list_target=False, cells=thp_cases.column(1, 1, [30, 31, 32]), name="A", scale=1.0),
                LC.producer(pkg, case, ("resv", 2.0 / DAY), {"resv": 2.0 / DAY}, use_list_target=False, cells=thp_cases.column(1, 1, [31, 32, 33]), name="B", scale=1.0)]
    lockstep(pkg, case, make, [moved(case, 5)])


def test_two_pvt_regions_the_first_perforation_in_the_second(pkg):
    fl = pkg.fluid.spe1_fluid()[0]
    r1 = dict(fl.pvt[0])
    r1["density"] = [1.06 * fl.pvt[0]["density"][0], 1.03 * fl.pvt[0]["density"][1], 1.2 * fl.pvt[0]["density"][2]]
    r1["pvtw"] = [fl.pvt[0]["pvtw"][0], 1.04 * fl.pvt[0]["pvtw"][1], 1.5 * fl.pvt[0]["pvtw"][2]] + list(fl.pvt[0]["pvtw"][3:])
    fl2 = pkg.fluid.Fluid([fl.pvt[0], r1], fl.sat, rock_pref=fl.rock_pref, rock_cr=fl.rock_cr)
    case = pkg.decks.cartesian_case(3, 3, 65, state="mixed", heterogeneous=True, dz=1.0, fluid=fl2)
    case["pvtnum"] = ((np.arange(case["Nb"]) // 9) % 2).astype(np.int32)          # layers alternate

    def make():
        return [LC.producer(pkg, case, ("resv", 3.0 / DAY), {"resv": 3.0 / DAY}, use_list_target=False, cells=thp_cases.column(1, 1, [31, 32, 33]), name="B", scale=1.0),
                LC.producer(pkg, case, ("resv", 3.0 / DAY), {"resv": 3.0 / DAY}, use_list_target=False, cells=thp_cases.column(0, 1, [30, 31, 32]), name="A", scale=1.0),
                LC.injector(pkg, case, ("resv", 55.0 / DAY), {"resv": 55.0 / DAY}, use_list_target=False)]
    (md, wd), (mh, wh), blk = lockstep(pkg, case, make, [])
    assert list(case["pvtnum"][[w.cells[0] for w in wh.wells]]) == [1, 0, 0] and list(wh.pvt_of_well) == [1, 0, 0]
    c = md.std_wells_resv()["coeff"]
    assert c[0, 1] != c[1, 1] and c[0, 0] == c[1, 0]                                 # the second region's water, the same oil tables


def test_limits_beside_crossflow_and_a_thp_limit(pkg):
    case = thp_cases.make_case(pkg)
    tabs = thp_cases.tables(pkg)

    def make():
        p = LC.producer(pkg, case, None, {"lrat": 39.0 / DAY, "resv": 80.0 / DAY, "grat": 1.0}, thp_limit=thp_cases.PROD_LIMIT)
        p.allow_crossflow = True
        i = LC.injector(pkg, case, None, {"resv": 70.0 / DAY}, thp_limit=thp_cases.INJ_LIMIT)
        return [p, i, LC.producer(pkg, case, None, {}, cells=thp_cases.column(1, 1, [30, 31]), name="P2", scale=1.0, own=("rate", pkg.wells.OIL, 2.0 / DAY))]
    for hm in ("cell_oil", "wellbore"):
        (md, wd), (mh, wh), blk = lockstep(pkg, case, make, [moved(case, 3), moved(case, 4, 4e5)], vfp=tabs, head_model=hm)
        print(hm, "controls", [w.control[0] for w in wh.wells])
        t = md.std_wells_thp()
        assert np.array_equal(t["thp"], wh.thp_current) and np.array_equal(t["dp"], wh.thp_dp) and np.array_equal(t["bhp_from_thp"], wh.bhp_from_thp)
        assert np.array_equal(md.std_wells_rate_dq(), wh.rate_dq)
        assert wh.wells[0].control[0] != "rate"


# ---- 3. the order of the checks --------------------------------------------------------------------------------------------------------------
def pairs(order):
    return [(order, order[i], order[i + 1]) for i in range(len(order) - 1)]


@pytest.mark.parametrize("order,first,second", pairs(LC.PRODUCER_ORDER) + pairs(LC.INJECTOR_ORDER),
                         ids=lambda v: v if isinstance(v, str) else ("producer" if v is LC.PRODUCER_ORDER else "injector"))
def test_of_two_violated_limits_the_earlier_wins(pkg, order, first, second):
    case = thp_cases.make_case(pkg)
    tabs = thp_cases.tables(pkg)
    is_prod = order is LC.PRODUCER_ORDER
    own = "orat" if is_prod else "rate"
    name = lambda k: "rate" if k == own else k
    x_flow = np.array([-4.6e-4, -2.0e-6, -0.12, 0.0]) if is_prod else np.array([0.0, 6.9e-4, 0.0, 0.0])
    bystander = [k for k in order if k not in (first, second)][-1 if first == "bhp" else 0]
    for in_force, winner in ((bystander, first), (first, second), (second, first)):
        made = [LC.ordered_pair_well(pkg, case, order, first, second, in_force) for _ in range(2)]
        bhp = made[0][1]
        it = iter(made)
        (md, wd), (mh, wh) = H.pair(pkg, case, lambda: [next(it)[0]], **constructor_kw(case, vfp=tabs))
        H.host_begin(mh, wh, 0)
        wd.begin_iteration(0)                      # dp, the averages and the coefficients of this time step on both sides
        x = x_flow.copy()
        x[3] = bhp
        for w in (wh.wells[0], wd.wells[0]):
            w.control = LC.control_of(w, name(in_force))
        wh.x[0] = x
        md.set_std_wells_state(x, [pkg.wells.CONTROL_CODE[wh.wells[0].control[0]]], None)
        wh.update_well_controls()
        wd.begin_iteration(1)
        xd = wd.fetch()
        got = "rate" if wh.wells[0].control == wh.wells[0].rate_control else wh.wells[0].control[0]
        assert got == name(winner), (in_force, got, winner)
        assert wd.wells[0].control == wh.wells[0].control and np.array_equal(xd, wh.x), (in_force, wd.wells[0].control, wh.wells[0].control)
        r = md.std_wells_resv()
        assert np.array_equal(r["resv_current"], wh.resv_current) and r["resv_current"][0] > 0.0
        assert np.array_equal(md.std_wells_thp()["thp"], wh.thp_current)


# ---- 4. what the C ABI refuses -----------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(pkg):
    capi = pkg.capi
    case = thp_cases.make_case(pkg)
    m = capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    assert capi.lib().opmhip_set_std_wells_limits(m._h, None) == capi.NOT_READY and b"no resident list" in capi.lib().opmhip_last_error(m._h)
    wd = pkg.wells.DeviceStandardWells([LC.producer(pkg, case, None, {"lrat": 1.0, "resv": 2.0}), LC.injector(pkg, case, None, {"resv": 1.0})], case["depth"], m)
    inf = np.inf
    good = dict(liquid_rate=[1.0, inf], resv_rate=[2.0, 1.0])

    def refused(limits, text):
        with pytest.raises(capi.OpmHipError) as e:
            m.set_std_wells_limits(limits)
        assert e.value.code == capi.INVALID_ARGUMENT and text in str(e.value), (text, str(e.value))
        # ... and the previous values are in force: control 6 is still accepted, 3 still refused
        m.set_std_wells_state(None, [6, 0], None)
        with pytest.raises(capi.OpmHipError):
            m.set_std_wells_state(None, [3, 0], None)
        m.set_std_wells_state(None, [0, 0], None)
    refused(dict(liquid_rate=[np.nan, inf]), "not > 0")
    refused(dict(liquid_rate=[-inf, inf]), "not > 0")
    refused(dict(gas_rate=[0.0, inf]), "not > 0")
    refused(dict(resv_rate=[-1.0, 1.0]), "not > 0")
    refused(dict(oil_rate=[1.0, inf]), "already names")
    refused(dict(liquid_rate=[1.0, 1.0]), "producer's limit")
    refused(dict(liquid_rate=[1.0, inf], use_list_target=[0, 1]), "under control 0")
    refused(dict(liquid_rate=[1.0, inf], use_list_target=[1, 2]), "use_list_target")
    m.set_std_wells_state(None, [6, 7], None)
    for bad in (dict(resv_rate=[2.0, 1.0]), dict(liquid_rate=[1.0, inf]), None):
        with pytest.raises(capi.OpmHipError) as e:
            m.set_std_wells_limits(bad)
        assert e.value.code == capi.INVALID_ARGUMENT and "cannot be taken away" in str(e.value)
    assert list(m.get_std_wells()[1]) == [6, 7]
    with pytest.raises(capi.OpmHipError) as e:
        m.set_std_wells_state(None, [8, 0], None)
    assert "control[0] = 8" in str(e.value)
    with pytest.raises(capi.OpmHipError) as e:
        m.set_std_wells_state(None, [5, 0], None)
    assert "without that limit" in str(e.value)
    m.set_std_wells_state(None, [1, 0], None)
    m.set_std_wells_limits(dict(oil_rate=[3.0, inf], use_list_target=[0, 1]))      # the own target out, ORAT in its place
    with pytest.raises(capi.OpmHipError) as e:
        m.set_std_wells_state(None, [0, 0], None)
    assert "use_list_target = 0" in str(e.value)
    m.set_std_wells_limits(None)                                                    # off: the new codes are gone
    with pytest.raises(capi.OpmHipError):
        m.set_std_wells_state(None, [3, 0], None)
    # opmhip_set_std_wells itself keeps to 0 / 1, and replacing the list clears the limits
    m.set_std_wells_limits(good)
    wd2 = pkg.wells.DeviceStandardWells([LC.producer(pkg, case, None, {})], case["depth"], m)
    with pytest.raises(capi.OpmHipError):
        m.set_std_wells_state(None, [6], None)
    assert np.all(m.std_wells_resv()["coeff"] == 0.0)


# ---- 5. two time steps with a given-up one, and the launches -------------------------------------------------------------------------------------
def spe9(pkg, limits):
    case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
    kw = dict(liquid_rate_stb_day=1500.00065, resv_rate=4000.0 * pkg.decks.STB_PER_DAY) if limits else {}
    return case, (lambda: pkg.decks.spe9_shaped_wells(case, **kw).wells)


def test_two_time_steps_with_a_given_up_one(pkg):
    """device and host in lock step over the wells' part of two time steps (begin_iteration(0), a second iteration after a reservoir change);
    the first attempt at step 2 is given up: opmhip_update_failed restores the controls and the retry forms the same averages"""
    case, make = spe9(pkg, True)
    (md, wd), (mh, wh) = H.pair(pkg, case, make, **constructor_kw(case))
    dt = 2.0 * DAY

    def change(seed, dp):
        """a Newton update's worth of change, the same on both sides (set_state would forget the old time level)"""
        rng = np.random.default_rng(seed)
        dx = np.zeros((case["Nb"], 3))
        dx[:, 1] = dp * rng.uniform(0.0, 1.0, case["Nb"])
        dx[:, 0] = rng.uniform(-0.01, 0.01, case["Nb"])
        return np.ascontiguousarray(dx.reshape(-1))

    def both_iterations(changes, what):
        for it, dx in enumerate(changes):
            if dx is not None:
                for m in (md, mh):
                    m.update(dx)
            wa = H.host_begin_and_assemble(mh, wh, it)
            mh.assemble(dt, it, fetch=False)
            wd.begin_iteration(it)
            md.assemble(dt, it, fetch=False)
            H.compare_wells(pkg, md, wh, wa, (what, it), extra=("D", "resv", "resv_current"), mh=mh)
    for m in (md, mh):
        m.advance_time_level()
    both_iterations([None, change(1, 1e5)], "step 1")
    modes1 = [w.control[0] for w in wh.wells]
    assert {"lrat", "resv"} <= set(modes1), modes1
    avg1 = md.std_wells_resv()["averages"]
    # step 2 begins; its first attempt moves the state and the controls, then is given up
    for m in (md, mh):
        m.advance_time_level()
    saved = wh.state()
    both_iterations([None, change(2, 6e5)], "step 2, given up")
    avg2 = md.std_wells_resv()["averages"]
    assert not np.array_equal(avg1, avg2)
    x_try = wd.fetch().copy()
    for m in (md, mh):
        m.update_failed()
    wh.set_state(saved)
    wd.fetch()
    assert [w.control for w in wd.wells] == [w.control for w in wh.wells] and np.array_equal(wd.x, wh.x) and not np.array_equal(wd.x, x_try)
    both_iterations([None], "step 2, retry")
    assert np.array_equal(md.std_wells_resv()["averages"], avg2)


def test_launch_counts_with_and_without_limits(pkg):
    """opmhip_profile_get's assembly class counts one scope per launcher: a Newton iteration's count is the same with and without limits; a
    time step (begin_iteration(0)) has one more only with a RESV limit - the scope of the averages' two kernels and the coefficients'"""
    counts = {}
    for name, kw in (("none", None), ("lrat", dict(liquid_rate_stb_day=1500.00065)), ("resv", dict(resv_rate=4000.0))):
        case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        wd = pkg.wells.DeviceStandardWells(pkg.decks.spe9_shaped_wells(case, **(kw or {})).wells, case["depth"], m)
        m.profile_enable(True)
        wd.begin_iteration(0)
        m.assemble(DAY, 0, fetch=False)
        m.synchronize()
        first = m.profile()["assemble"][0]
        wd.begin_iteration(1)
        m.assemble(DAY, 1, fetch=False)
        m.synchronize()
        counts[name] = (first, m.profile()["assemble"][0] - first)
    print("assembly-class scopes (time step's first iteration, a later iteration):", counts)
    assert counts["none"][1] == counts["lrat"][1] == counts["resv"][1]
    assert counts["none"][0] == counts["lrat"][0] and counts["resv"][0] == counts["none"][0] + 1

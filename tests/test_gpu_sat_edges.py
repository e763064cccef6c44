"""Saturation end-point scaling and relative-permeability hysteresis of the per-cell kernels on their end points, table nodes and
turning points.  The states are the labelled ones of tests/sat_states.py, one per cell of an N x 1 x 1 grid (N above 256 and no
multiple of it: the 256-thread kernels end on a partial block); the CPU side of every statement here is in tests/test_sat_states.py.

  scaling      per fluid (Corey pair, plateau, degenerate, piston) and configuration (two- / three-point map, vertical mode 0 | 1 | 2
               per curve, pcw / pcg on and off, vertical scaling without saturation scaling): sat_probe and iq() the oracle's bit for
               bit, the device within 4 x the oracle's measured distance of the exact statement, the end values on the end points,
               Jacobian and residual of one assembly bit for bit, three Newton updates (+d, -2 d, a large seeded one: every member of
               a triple crosses its edge) with state, meanings, switch count and iq() the oracle's
  hysteresis   kr_model 0 | 1 x (no scaling, the imbibition tables' own points, scaled imbibition points): after
               set_hysteresis_params with the states' turning points hysteresis() and iq() bit for bit, hysteresis() within the
               bound of the exact (turning point, shift); one assembly bit for bit; one begin_time_step moves the turning points of
               exactly the rows whose label says so; the three updates
  refusals     end points that would make a kernel divide by zero are refused on the host, naming the cell, before anything is
               uploaded: the context assembles bit for bit as before"""
import numpy as np
import pytest

import oracle_bind
import sat_states as ss
from test_gpu_table_edges import same, steps_of, updates_agree
from test_sat_states import hyst_cases, hyst_setup

pytestmark = pytest.mark.gpu
DT = 86400.0


@pytest.fixture(scope="module")
def fluids(pkg):
    return ss.sat_fluids(pkg)


def two(pkg, orc, case):
    m = pkg.capi.HipModel(case)
    o = oracle_bind.OracleModel(orc, case)
    for q in (m, o):
        q.set_state(case["pv"], case["meaning"])
    return m, o


def assembled_alike(m, o, what):
    jm, rm = m.assemble(DT, 0)
    jo, ro = o.assemble(DT, 0)
    same(rm, ro, (what, "residual"))
    same(jm, jo, (what, "jacobian"))
    assert np.isfinite(jm).all() and np.isfinite(rm).all()
    return jm, rm


SCALING_CASES = [(f, c) for f in ("corey", "plateau", "degenerate", "piston") for c in ss.CONFIGS
                 if f != "piston" or 2 not in (ss.CONFIGS[c]["krw"], ss.CONFIGS[c]["kro"], ss.CONFIGS[c]["krg"])]


@pytest.mark.parametrize("fname,cn", SCALING_CASES)
def test_scaling_states(pkg, orc, fluids, fname, cn):
    fl, dr, im, cfgs = fluids[fname]
    assert cn in cfgs
    es = ss.CONFIGS[cn]
    st = ss.states(fl, dr, es)
    N = len(st["rows"])
    assert N > 256 and N % 256 != 0
    case = ss.case_of(pkg, fl, st["rows"])
    case["endscale"] = ss.endscale_dict(pkg, es, st["pts"])
    m, o = two(pkg, orc, case)
    iq = m.iq()
    assert iq.shape[1] == 19 and np.isfinite(iq).all()
    same(iq, o.iq(), "iq")
    assembled_alike(m, o, "scaling")
    sd = ss.sat_probe_by_set(pkg.capi.HipFluid(fl), st, es, dr)
    so = ss.sat_probe_by_set(oracle_bind.OracleFluid(orc, fl), st, es, dr)
    same(sd, so, "sat_probe")
    ex = ss.exact_sat(fl, st, es)
    for what, (d, where) in zip(("sat_probe", "cache"), ss.distances(fl, st, ex, sd, iq)):
        print("%-11s %-16s %-10s %.3e  %s" % (fname, cn, what, d, st["labels"][where[0]] if where else ""))
        assert d <= ss.BOUND, (what, d, where, st["labels"][where[0]])
    n, nbit, wrong = ss.end_value_checks(fl, st, es, sd)
    assert not wrong and (not (ss.cfg_of(es) & 1) or (n >= 20 and nbit >= 5)), (n, nbit, wrong[:4])
    assert updates_agree([m, o], steps_of(st["rows"])) >= 8


@pytest.mark.parametrize("fname,cname,model", hyst_cases())
def test_hysteresis_states(pkg, orc, fluids, fname, cname, model):
    fl, es, st, case, imb = hyst_setup(pkg, fluids, fname, cname)
    N = len(st["rows"])
    assert N > 256 and N % 256 != 0
    m, o = two(pkg, orc, case)
    for q in (m, o):
        q.set_hysteresis(model, st["imbnum"], imb)
        q.set_hysteresis_params(st["mdc_ow"], st["mdc_go"])
    h, ho = m.hysteresis(), o.hysteresis()
    for k in range(4):
        same(h[k], ho[k], ("hysteresis", k))
    iq = m.iq()
    same(iq, o.iq(), "iq")
    assert np.isfinite(iq).all() and all(np.isfinite(a).all() for a in h)
    ex = ss.exact_sat(fl, st, es, hyst=dict(model=model))
    for what, (d, where) in zip(("cache", "turning"), ss.distances(fl, st, ex, None, iq, h)):
        print("%-11s %-7s %d %-8s %.3e  %s" % (fname, cname, model, what, d, st["labels"][where[0]] if where else ""))
        assert d <= ss.BOUND, (what, d, where, st["labels"][where[0]])
    same(h[0], st["mdc_ow"], "the turning points handed in, oil-water")
    same(h[2], st["mdc_go"], "the turning points handed in, gas-oil")
    assembled_alike(m, o, "hysteresis")
    # one change of time step: the turning points move exactly where the labels say - stated from the states, not by the oracle
    for q in (m, o):
        q.begin_time_step(DT)
    h2, ho2 = m.hysteresis(), o.hysteresis()
    for k in range(4):
        same(h2[k], ho2[k], ("hysteresis after begin_time_step", k))
    for q, (sys_, seen, move) in enumerate((("ow", st["sOw"], st["move_ow"]), ("go", st["sGo"], st["move_go"]))):
        same(h2[2 * q], np.where(move, seen, h[2 * q]), ("turning points after begin_time_step", sys_))
        same(h2[2 * q + 1][~move], h[2 * q + 1][~move], ("shifts of the rows that did not move", sys_))
        for c, l in enumerate(st["labels"]):
            if l.startswith("upd:%s:" % sys_) or (sys_ == "go" and l.startswith("clamp:")):
                assert bool(move[c]) == l.endswith(":below"), (l, c)
                assert (h2[2 * q][c] != h[2 * q][c]) == l.endswith(":below"), (l, c)
    same(m.iq(), o.iq(), "iq after begin_time_step")
    assert updates_agree([m, o], steps_of(st["rows"])) >= 8
    for k in range(4):      # an update leaves the turning points alone
        same(m.hysteresis()[k], h2[k], ("hysteresis after the updates", k))


@pytest.mark.parametrize("fname", ["corey", "plateau"])
def test_a_turning_point_met_exactly_keeps_its_shift(pkg, orc, fluids, fname):
    """k_hyst_update compares with `<`: a saturation EQUAL to the stored turning point recomputes nothing.  With a shift that is
    consistent with its turning point a recomputation would give the same double and `<=` could not be told from `<`; so the
    drainage end points change between set_hysteresis_params and the change of time step - the shift of a row that does not move
    is then the OLD one to the bit, while a recomputed one would differ (the statement's own doubles say so)."""
    fl, es, st, case, imb = hyst_setup(pkg, fluids, fname, "own")
    m, o = two(pkg, orc, case)
    for q in (m, o):
        q.set_hysteresis(0, st["imbnum"], imb)
        q.set_hysteresis_params(st["mdc_ow"], st["mdc_go"])
    h = m.hysteresis()
    other = np.array([ss.point_sets(st["u"])[2]] * len(st["rows"]))       # another SOWCR and SWU: the drainage krow moves
    other[:, ss.SGCR] = 0.125                                             # and another SGCR: the drainage krg too
    assert ss.interval_ok(other[0])
    for q in (m, o):
        q.set_endpoint_scaling(ss.endscale_dict(pkg, es, other))
    for k in range(4):
        same(m.hysteresis()[k], h[k], ("new end points leave the hysteresis state alone", k))
    for q in (m, o):
        q.begin_time_step(DT)
    h2, ho2 = m.hysteresis(), o.hysteresis()
    for k in range(4):
        same(h2[k], ho2[k], ("hysteresis after begin_time_step", k))
    T = ss.tables(fl)["sat"]
    cfg = ss.cfg_of(es)
    told = 0
    for q, (sys_, kind, seen, move) in enumerate((("ow", ss.KRN_OW, st["sOw"], st["move_ow"]), ("go", ss.KRN_GO, st["sGo"], st["move_go"]))):
        same(h2[2 * q], np.where(move, seen, h[2 * q]), ("turning points", sys_))
        same(h2[2 * q + 1][~move], h[2 * q + 1][~move], ("shifts of the rows that did not move", sys_))
        for c, l in enumerate(st["labels"]):
            if l == "upd:%s:equal" % sys_:
                Si = T[int(st["imbnum"][c])]
                uI = ss.table_end_points(Si)
                Sv = ss.K(float(seen[c]), float)
                k = ss.sat_curve(T[st["region"]], kind, Sv, True, cfg, st["u"], list(other[c]), float)
                again = (ss.sat_curve_inv(Si, kind, k, True, cfg, uI, uI, float) - Sv).f
                told += int(again != h[2 * q + 1][c])
    assert told >= 4, told      # rows at which `<=` would have been seen


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def refused(pkg, call, *words):
    with pytest.raises(pkg.capi.OpmHipError) as e:
        call()
    assert e.value.code == pkg.capi.INVALID_ARGUMENT
    assert all(w in str(e.value) for w in words), (str(e.value), words)


def small_case(pkg, fl, region, n=40):
    rows = np.zeros((n, 6))
    rows[:, 0] = 0.3 + 0.01 * np.arange(n) % 0.4
    rows[:, 1] = ss.P_STATE
    rows[:, 2] = 0.05 + 0.005 * np.arange(n) % 0.2
    rows[:, 5] = region
    return ss.case_of(pkg, fl, rows)


def test_imbibition_end_points_without_an_interval_are_refused(pkg, orc, fluids):
    """opmhip_set_hysteresis puts the imbibition points through the check opmhip_set_endpoint_scaling puts the drainage points
    through: SWCR == SWU in one cell makes eps_sat_two_point divide by zero in k_iq_update, SWL + SGL == 1 - SOWCR in k_hyst_update
    (tests/test_sat_states.py shows the oracle's cache with such points: not finite)"""
    fl, dr, im, _ = fluids["corey"]
    case = small_case(pkg, fl, dr)
    n = case["Nb"]
    u = ss.table_end_points(ss.tables(fl)["sat"][dr])
    es = ss.CONFIGS["two_v2"]
    case["endscale"] = ss.endscale_dict(pkg, es, np.array([ss.point_sets(u)[0]] * n))
    m, o = two(pkg, orc, case)
    imbnum = np.full(n, im, np.int32)
    uI = ss.table_end_points(ss.tables(fl)["sat"][im])
    good = ss.endscale_dict(pkg, {}, np.array([ss.imb_point_set(uI)] * n))
    for q in (m, o):
        q.set_hysteresis(1, imbnum, good)
        q.set_hysteresis_params(np.full(n, 0.5), np.full(n, 0.7))
    before = assembled_alike(m, o, "before the refusals")
    hb = m.hysteresis()
    for cell, field, other in ((7, "swl", "swu"), (11, "sgl", "sgu"), (3, "swcr", "swu"), (n - 1, "sgcr", "sgu")):
        bad = {k: v.copy() for k, v in good.items()}
        bad[field][cell] = bad[other][cell]
        refused(pkg, lambda: m.set_hysteresis(1, imbnum, bad), "cell %d" % cell, "no saturation interval", "imbibition")
    bad = {k: v.copy() for k, v in good.items()}
    bad["sowcr"][5] = 1.0 - bad["swl"][5] - bad["sgl"][5]
    refused(pkg, lambda: m.set_hysteresis(0, imbnum, bad), "cell 5", "no saturation interval")
    bad = {k: v.copy() for k, v in good.items()}
    bad["sogcr"][9] = 1.0 - bad["swl"][9] - bad["sgl"][9]
    refused(pkg, lambda: m.set_hysteresis(0, imbnum, bad), "cell 9", "no saturation interval")
    # the previous settings are still in force, kr_model included
    for k in range(4):
        same(m.hysteresis()[k], hb[k], ("hysteresis after the refusals", k))
    after = assembled_alike(m, o, "after the refusals")
    same(after[0], before[0], "jacobian as before")
    same(after[1], before[1], "residual as before")


def test_vertical_scaling_by_a_table_value_of_zero_is_refused(pkg, orc, fluids):
    """mode 1 divides by the table's maximum, mode 2 by the table's value at the displacing phase's critical saturation: a region
    with an immobile phase, or one whose curve is still zero there, would give 0 x inf = NaN in the cached mobilities"""
    deg, _, _, _ = fluids["degenerate"]      # region 1: the piston - KRWR = KRORW = KRGR = KRORG = 0, positive maxima
    pla, _, _, _ = fluids["plateau"]         # region 3: krow and krg zero everywhere
    # -- the drainage region, opmhip_set_endpoint_scaling --
    case = small_case(pkg, deg, 1)
    n = case["Nb"]
    u = ss.table_end_points(ss.tables(deg)["sat"][1])
    pts = np.array([ss.point_sets(u)[0]] * n)
    ok = ss.CONFIGS["three_v1"]
    case["endscale"] = ss.endscale_dict(pkg, ok, pts)
    m, o = two(pkg, orc, case)
    before = assembled_alike(m, o, "piston, mode 1")
    for curve, kw in (("krw", dict(krw=2)), ("krow", dict(kro=2)), ("krg", dict(krg=2))):
        refused(pkg, lambda: m.set_endpoint_scaling(ss.endscale_dict(pkg, ss.config(three=1, **kw), pts)), "cell ", "saturation region 1", "scale %s vertically (mode 2)" % curve)
    refused(pkg, lambda: m.set_endpoint_scaling(ss.endscale_dict(pkg, ss.config(sat_scaling=0, krw=2), pts)), "cell ", "scale krw vertically (mode 2)")
    after = assembled_alike(m, o, "piston, after the refusals")
    same(after[0], before[0], "jacobian as before")
    same(after[1], before[1], "residual as before")
    # a mixed grid: the one cell of the piston region is named
    case = small_case(pkg, deg, 0)
    case["satnum"][17] = 1
    pts = np.array([ss.point_sets(ss.table_end_points(ss.tables(deg)["sat"][0]))[0]] * n)
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    refused(pkg, lambda: m.set_endpoint_scaling(ss.endscale_dict(pkg, ss.CONFIGS["three_v2"], pts)), "cell 17", "saturation region 1", "mode 2")
    # an immobile phase: the maximum itself is 0
    case = small_case(pkg, pla, 3)
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    for curve, kw in (("krow", dict(kro=1)), ("krg", dict(krg=1)), ("krow", dict(kro=2)), ("krg", dict(krg=2))):
        refused(pkg, lambda: m.set_endpoint_scaling(dict(ss.config(sat_scaling=0, **kw))), "cell ", "saturation region 3", "scale %s vertically" % curve)
    m.set_endpoint_scaling(dict(ss.config(sat_scaling=0, krw=1)))      # (the water curve has a maximum: accepted)
    assert np.isfinite(m.iq()).all()
    # -- the imbibition region, opmhip_set_hysteresis and, with hysteresis in force, opmhip_set_endpoint_scaling --
    case = small_case(pkg, deg, 0)
    u = ss.table_end_points(ss.tables(deg)["sat"][0])
    pts = np.array([ss.point_sets(u)[0]] * n)
    case["endscale"] = ss.endscale_dict(pkg, ss.CONFIGS["three_v2"], pts)
    m, o = two(pkg, orc, case)
    imbnum = np.zeros(n, np.int32)
    imbnum[23] = 1
    refused(pkg, lambda: m.set_hysteresis(0, imbnum), "cell 23", "saturation region 1", "imbibition", "mode 2")
    with pytest.raises(pkg.capi.OpmHipError):      # refused as a whole: hysteresis is not in force
        m.hysteresis()
    before = assembled_alike(m, o, "degenerate, no hysteresis")
    for q in (m, o):
        q.set_endpoint_scaling(ss.endscale_dict(pkg, ss.CONFIGS["three_v1"], pts))
        q.set_hysteresis(0, imbnum)
    mid = assembled_alike(m, o, "degenerate, mode 1, the piston as imbibition region of one cell")
    refused(pkg, lambda: m.set_endpoint_scaling(ss.endscale_dict(pkg, ss.CONFIGS["three_v2"], pts)), "cell 23", "imbibition", "mode 2")
    after = assembled_alike(m, o, "after the refusal")
    same(after[0], mid[0], "jacobian as before")
    same(after[1], mid[1], "residual as before")

"""The labelled states of tests/sat_states.py - saturation end-point scaling and relative-permeability hysteresis on their end points,
nodes and turning points - and the CPU oracle at them (no GPU).

  census          every kind of edge sat_states.KINDS / HYST_KINDS names has a row, for every fluid and configuration; the generator
                  is deterministic; the cell count is above 256 and no multiple of it
  exactness       the oracle (OracleFluid.sat_probe with the row's end points, OracleModel.iq(), .hysteresis()) against exact_sat
                  (fractions.Fraction) on EVERY row - none is left out, every oracle value is finite - within the recorded distance;
                  the doubles of the same statement (the .f side of sat_states.Dual) are the oracle's bit for bit
  end values      on a scaled end point the curve takes its scaled end value, to the bit where nothing rounds; the neighbours one ulp
                  away lie on the stated side
  pwlin_inv       inverts pwlin exactly on strictly monotone segments (Fraction); plateaus, nodes, both ends, a curve that is zero
                  everywhere, the decreasing and the increasing form as the module states them
  update          one change of time step moves the turning points of exactly the rows whose label says so

Measured here (oracle to exact, the largest table_states.relative_distance over all rows of all fluids and configurations): 5.16e-16
(sat_states.ORACLE_TO_EXACT; test_the_recorded_bound_is_the_measured_one prints it and where)."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import oracle_bind
import sat_states as ss
import table_states as ts

DT = 86400.0


@pytest.fixture(scope="module")
def fluids(pkg):
    return ss.sat_fluids(pkg)


def hyst_cases():
    """(fluid, configuration of sat_states.HYST_CONFIGS - which also says whose imbibition points: the tables' own or scaled ones -,
    kr_model)"""
    return [(f, c, m) for f in ("corey", "plateau", "degenerate") for c in ("none", "own", "scaled") for m in (0, 1)
            if not (f == "degenerate" and c == "scaled")]     # (the piston's KRORW = 0: mode 2 is refused, tests/test_gpu_sat_edges.py)


def hyst_setup(pkg, fluids, fname, cname):
    fl, dr, im, _ = fluids[fname]
    es = ss.HYST_CONFIGS[cname]
    regions = [im]
    if fname == "plateau":
        regions = [1, 2] + ([3] if cname == "none" else [])      # (the zero curves have no scaled interval and no denominators)
    st = ss.hyst_states(fl, dr, es, cname == "scaled", regions)
    case = ss.case_of(pkg, fl, st["rows"])
    if es is not None:
        case["endscale"] = ss.endscale_dict(pkg, es, st["pts"])
    imb = None if st["pts_imb"] is None else {k: v for k, v in ss.endscale_dict(pkg, {}, st["pts_imb"]).items()}
    return fl, es, st, case, imb


MEASURED = {}      # case -> the largest distance oracle to exact there; every measurement runs once a session


def test_census_of_the_scaling_states(pkg, fluids):
    for name, (fl, dr, im, cfgs) in fluids.items():
        for cn in cfgs:
            st = ss.states(fl, dr, ss.CONFIGS[cn])
            again = ss.states(fl, dr, ss.CONFIGS[cn])
            assert np.array_equal(st["rows"], again["rows"]) and st["labels"] == again["labels"]
            N = len(st["rows"])
            assert 256 < N < 1000 and N % 256 != 0, N
            kinds, full = ss.census(st["labels"])
            missing = [k for k in ss.KINDS if not kinds.get(k)]
            assert not missing, (name, cn, missing)
            # both sides of every scaled point, and the point itself
            for k in ss.KINDS[:16]:
                assert full.get(k + "0") and (full.get(k + "-") or full.get(k + "~-")) and (full.get(k + "+") or full.get(k + "~+")), (name, cn, k)
            assert full.get("blend:eps-") and full.get("blend:eps+") and full.get("blend:half_eps-") and full.get("blend:half_eps+")
            assert set(st["sets"].tolist()) == set(range(len(ss.SET_NAMES)))
    print(ss.census(ss.states(fluids["plateau"][0], 0, ss.CONFIGS["three_v2"])["labels"])[0])


def test_census_of_the_hysteresis_states(pkg, fluids):
    for fname, cname, model in hyst_cases():
        if model:
            continue
        fl, es, st, case, imb = hyst_setup(pkg, fluids, fname, cname)
        N = len(st["rows"])
        assert 256 < N < 1000 and N % 256 != 0, N
        kinds, full = ss.census(st["labels"])
        want = list(ss.HYST_KINDS)
        if cname == "none":
            want += ss.HYST_KINDS_UNSCALED + (ss.HYST_KINDS_GO_MAX if fname != "corey" else [])
        if fname == "plateau" and cname == "none":
            want += ss.HYST_KINDS_PLATEAU + ss.HYST_KINDS_FLAT
        missing = [k for k in want if not kinds.get(k)]
        assert not missing, (fname, cname, missing)
        assert all(full.get("scan:%s%s" % (a, b)) for a in ("ow", "go") for b in "-0+")
        if fname == "plateau":     # the inversion's other forms are met under every configuration
            assert any(k.startswith("inv:ow:inc:") for k in kinds) and any(k.startswith("inv:go:inc:") for k in kinds)
    print(ss.census(ss.hyst_states(fluids["plateau"][0], 0, None, False, [1, 2, 3])["labels"])[0])


SCALING_FLUIDS = ["corey", "plateau", "degenerate", "piston"]


@pytest.mark.parametrize("fname", SCALING_FLUIDS)
def test_oracle_against_the_exact_statement_scaling(pkg, orc, fluids, fname):
    assert scaling_distance(pkg, orc, fluids, fname) <= ss.ORACLE_TO_EXACT


def scaling_distance(pkg, orc, fluids, fname):
    if fname in MEASURED:
        return MEASURED[fname]
    fl, dr, im, cfgs = fluids[fname]
    of = oracle_bind.OracleFluid(orc, fl)
    worst = 0.0
    for cn in cfgs:
        es = ss.CONFIGS[cn]
        st = ss.states(fl, dr, es)
        case = ss.case_of(pkg, fl, st["rows"])
        case["endscale"] = ss.endscale_dict(pkg, es, st["pts"])
        o = oracle_bind.OracleModel(orc, case)
        o.set_state(case["pv"], case["meaning"])
        iq = o.iq()
        jac, res = o.assemble(DT, 0)
        sat = ss.sat_probe_by_set(of, st, es, dr)
        # no row is left out: the oracle alone is finite everywhere
        assert np.isfinite(iq).all() and np.isfinite(sat).all() and np.isfinite(jac).all() and np.isfinite(res).all(), (fname, cn)
        ex = ss.exact_sat(fl, st, es)
        assert all(v is not None for v in ex["sat"].reshape(-1)) and all(v is not None for v in ex["iq"].reshape(-1))
        for what, (d, where) in zip(("sat_probe", "cache"), ss.distances(fl, st, ex, sat, iq)):
            print("%-11s %-16s %-10s %.3e  %s" % (fname, cn, what, d, st["labels"][where[0]] if where else ""))
            worst = max(worst, d)
        # the doubles of the same statement are the oracle's
        fx = ss.exact_sat(fl, st, es, num=float)
        assert np.array_equal(np.array(fx["sat"], np.float64), sat), (fname, cn)
        # on the end points: the end values
        n, nbit, wrong = ss.end_value_checks(fl, st, es, sat)
        assert not wrong, (fname, cn, wrong[:4])
        assert not (ss.cfg_of(es) & 1) or (n >= 20 and nbit >= 5), (n, nbit)
    MEASURED[fname] = worst
    return worst


@pytest.mark.parametrize("fname,cname,model", hyst_cases())
def test_oracle_against_the_exact_statement_hysteresis(pkg, orc, fluids, fname, cname, model):
    assert hyst_distance(pkg, orc, fluids, fname, cname, model) <= ss.ORACLE_TO_EXACT


def hyst_distance(pkg, orc, fluids, fname, cname, model):
    key = "%s/%s/%d" % (fname, cname, model)
    if key in MEASURED:
        return MEASURED[key]
    fl, es, st, case, imb = hyst_setup(pkg, fluids, fname, cname)
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    o.set_hysteresis(model, st["imbnum"], imb)
    o.set_hysteresis_params(st["mdc_ow"], st["mdc_go"])
    h, iq = o.hysteresis(), o.iq()
    jac, res = o.assemble(DT, 0)
    assert all(np.isfinite(a).all() for a in h) and np.isfinite(iq).all() and np.isfinite(jac).all() and np.isfinite(res).all()
    ex = ss.exact_sat(fl, st, es, hyst=dict(model=model))
    assert all(v is not None for v in ex["iq"].reshape(-1)) and all(v is not None for v in ex["hyst"].reshape(-1))
    worst = 0.0
    for what, (d, where) in zip(("cache", "turning"), ss.distances(fl, st, ex, None, iq, h)):
        print("%-11s %-7s %d %-8s %.3e  %s" % (fname, cname, model, what, d, st["labels"][where[0]] if where else ""))
        worst = max(worst, d)
    assert np.array_equal(ex["hyst_f"], np.stack(h, axis=1))          # the doubles of the statement are the oracle's
    assert np.array_equal(h[0], st["mdc_ow"]) and np.array_equal(h[2], st["mdc_go"])
    # one change of time step: the turning points move exactly where the labels say - from the states, not from the oracle
    o.begin_time_step(DT)
    h2 = o.hysteresis()
    for q, (sys_, seen, move) in enumerate((("ow", st["sOw"], st["move_ow"]), ("go", st["sGo"], st["move_go"]))):
        assert np.array_equal(h2[2 * q], np.where(move, seen, h[2 * q]))
        assert np.array_equal(h2[2 * q + 1][~move], h[2 * q + 1][~move])
        for c, l in enumerate(st["labels"]):
            if l.startswith("upd:%s:" % sys_) or (sys_ == "go" and l.startswith("clamp:")):
                assert bool(move[c]) == l.endswith(":below"), (l, c)
    assert st["move_ow"].sum() >= 8 and st["move_go"].sum() >= 8 and (~st["move_ow"]).sum() >= 16
    MEASURED[key] = worst
    return worst


def test_the_recorded_bound_is_the_measured_one(pkg, orc, fluids):
    """the largest of the distances measured above is the recorded constant, not a looser one"""
    for fname in SCALING_FLUIDS:
        scaling_distance(pkg, orc, fluids, fname)
    for fname, cname, model in hyst_cases():
        hyst_distance(pkg, orc, fluids, fname, cname, model)
    worst = max(MEASURED.values())
    print("largest distance oracle to exact: %.17g (recorded: %.17g), at %s" % (worst, ss.ORACLE_TO_EXACT, max(MEASURED, key=MEASURED.get)))
    assert worst <= ss.ORACLE_TO_EXACT and worst >= ss.ORACLE_TO_EXACT / 4.0


def test_neighbours_of_a_scaled_point_lie_on_their_side(pkg, fluids):
    """the three-point map one ulp either side of its points: below and on a point the piece on its left, above it the next"""
    fl, dr, _, _ = fluids["corey"]
    st = ss.states(fl, dr, ss.CONFIGS["three_v2"])
    u, n = st["u"], 0
    for kind in ("krw_ow", "krn_ow", "krw_go", "krn_go"):
        ut = ss.eps_triples(u)[kind]
        for s in ss.point_sets(u):
            sc = ss.eps_triples(s)[kind]
            img = lambda v: ss.three_point(ss.K(v, Fr), ut, sc, Fr).n
            assert img(ts.below(sc[0])) == img(sc[0]) == Fr(ut[0]) and (img(ts.above(sc[0])) > Fr(ut[0]) or sc[0] == sc[1])
            assert img(sc[2]) <= Fr(ut[2]) + Fr(1, 2 ** 60) and img(ts.above(sc[2])) == Fr(ut[2])
            if sc[0] < sc[1] < sc[2]:
                # on s1 the first segment's formula (exact: u1), one ulp above the second's
                assert img(sc[1]) == Fr(ut[1])
                slope2 = (Fr(ut[2]) - Fr(ut[1])) / (Fr(sc[2]) - Fr(sc[1]))
                assert img(ts.above(sc[1])) == Fr(ut[1]) + (Fr(ts.above(sc[1])) - Fr(sc[1])) * slope2
                n += 1
    assert n >= 8


def test_pwlin_inv_inverts_pwlin_and_keeps_its_conventions(pkg, fluids):
    fl = fluids["plateau"][0]
    T = ss.tables(fl)["sat"]
    inv = lambda x, y, v: ss.pwlin_inv(x, y, ss.Dual(float(v), Fr(v)), Fr).n
    n = 0
    for r, xk, yk in ((0, "sw", "krow"), (0, "so", "krg"), (1, "sw", "krow"), (1, "so", "krg"), (2, "sw", "krow"), (2, "so", "krg")):
        x, y = T[r][xk], T[r][yk]
        for j in range(len(x) - 1):
            if y[j] == y[j + 1]:
                continue
            strict = (j == 0 or y[j - 1] != y[j]) and (j + 2 == len(x) or y[j + 2] != y[j + 1])
            for f in (Fr(1, 3), Fr(1, 2), Fr(7, 8)):
                xv = Fr(x[j]) + f * (Fr(x[j + 1]) - Fr(x[j]))
                yv = Fr(y[j]) + (xv - Fr(x[j])) * (Fr(y[j + 1]) - Fr(y[j])) / (Fr(x[j + 1]) - Fr(x[j]))
                # (decisions on the nearest double, arithmetic exact: inside a segment the two agree)
                assert inv(x, y, yv) == xv, (r, yk, j)
                n += 1
    assert n >= 60
    # the conventions, on the drainage krow of the plateau fluid: 0.8 0.8 0.6 0.4 0.4 0.4 0.2 0 0 0 over ten nodes
    x, y = T[0]["sw"], T[0]["krow"]
    assert y == [0.8, 0.8, 0.6, 0.4, 0.4, 0.4, 0.2, 0.0, 0.0, 0.0]
    assert inv(x, y, 0.0) == Fr(x[-1]) and inv(x, y, -1.0) == Fr(x[-1])          # 0: the LAST node, not the critical saturation x[7]
    assert inv(x, y, 0.8) == Fr(x[0]) and inv(x, y, 0.9) == Fr(x[0])             # the maximum and beyond: the first node
    assert inv(x, y, 0.6) == Fr(x[2])                                            # on a node: the node
    assert inv(x, y, 0.4) == Fr(x[5])                                            # on a plateau: its right end
    assert inv(x, y, ts.above(0.4)) < Fr(x[3]) and inv(x, y, ts.below(0.4)) > Fr(x[5])
    # increasing form (region 2): 0.1 0.1 0.2 0.4 0.4 0.4 0.6 0.7 0.8 0.8
    x, y = T[2]["sw"], T[2]["krow"]
    assert inv(x, y, 0.1) == Fr(x[0]) and inv(x, y, 0.05) == Fr(x[0]) and inv(x, y, 0.8) == Fr(x[-1]) and inv(x, y, 1.0) == Fr(x[-1])
    assert inv(x, y, 0.4) == Fr(x[5]) and inv(x, y, 0.6) == Fr(x[6])
    # zero everywhere (region 3): y[0] == y[n-1] takes the increasing form - 0 gives the first node, anything above the last
    x, y = T[3]["sw"], T[3]["krow"]
    assert inv(x, y, 0.0) == Fr(x[0]) and inv(x, y, 1e-300) == Fr(x[-1]) and inv(x, y, -1.0) == Fr(x[0])


def test_inverse_three_point_map_puts_a_point_on_its_right_piece(pkg, fluids):
    """sat_curve_inv with `<`: Su on u1 is mapped with the SECOND segment's formula (to s1 exactly), Su on u2 to s2; the forward
    map's `<=` takes a value on s1 with the first segment - both give the same point, the derivatives differ"""
    fl, dr, im, _ = fluids["plateau"]
    S = ss.tables(fl)["sat"][im]
    u = ss.table_end_points(S)
    s = ss.imb_point_set(u)
    cfg = ss.cfg_of(ss.CONFIGS["three_v0"])
    for kind, name in ((ss.KRN_OW, "krn_ow"), (ss.KRN_GO, "krn_go")):
        ut, st = ss.eps_triples(u)[name], ss.eps_triples(s)[name]
        x, y = S[ss._XY[kind][0]], S[ss._XY[kind][1]]
        for i in (1, 2):
            if ut[i] in x and 0 < x.index(ut[i]) < len(x) - 1 and y[x.index(ut[i])] not in (y[x.index(ut[i]) - 1], y[x.index(ut[i]) + 1]):
                k = ss.K(y[x.index(ut[i])], Fr)
                assert ss.sat_curve_inv(S, kind, k, True, cfg, u, s, Fr).n == Fr(st[i]), (name, i)


def test_what_the_refused_end_points_would_give(pkg, orc, fluids):
    """the oracle makes the same statements as the kernels and has no set-up check: with the inputs the device refuses
    (tests/test_gpu_sat_edges.py, end_points_refusal in csrc/fluid_tables.cpp) its cache is not finite"""
    from test_gpu_sat_edges import small_case
    # imbibition end points without an interval: SWCR == SWU in one cell - the two-point map of the imbibition krw divides by
    # SWU - SWCR: (S - SWCR) x inf, which pwlin clamps to an end of the table (krw jumps from 0 to its maximum at SWCR) and which is
    # 0 x inf = NaN at S == SWCR itself
    fl, dr, im, _ = fluids["corey"]
    case = small_case(pkg, fl, dr)
    n = case["Nb"]
    T = ss.tables(fl)["sat"]
    case["endscale"] = ss.endscale_dict(pkg, ss.CONFIGS["two_v2"], np.array([ss.point_sets(ss.table_end_points(T[dr]))[0]] * n))
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    bad = ss.endscale_dict(pkg, {}, np.array([ss.imb_point_set(ss.table_end_points(T[im]))] * n))
    bad["swcr"][7] = bad["swu"][7]
    pv = case["pv"].reshape(-1, 3).copy()
    pv[7, 0], pv[7, 2] = bad["swu"][7], 0.0
    o.set_state(np.ascontiguousarray(pv.reshape(-1)), case["meaning"])
    assert not ss.interval_ok([bad[k][7] for k in pkg.capi.EPS_FIELDS])
    with np.errstate(all="ignore"):
        o.set_hysteresis(1, np.full(n, im, np.int32), bad)
        o.set_hysteresis_params(np.full(n, 0.5), np.full(n, 0.7))
        finite = np.isfinite(o.iq()).reshape(n, -1).all(axis=1)
    assert not finite[7] and finite[np.arange(n) != 7].all()
    # vertical scaling by a table value of 0: the piston region in mode 2, the plateau fluid's immobile oil and gas in mode 1
    for fl, region, es in ((fluids["degenerate"][0], 1, ss.config(sat_scaling=0, krw=2, kro=2, krg=2)), (fluids["plateau"][0], 3, ss.config(sat_scaling=0, kro=1, krg=1))):
        case = small_case(pkg, fl, region)
        u = ss.table_end_points(ss.tables(fl)["sat"][region])
        case["endscale"] = ss.endscale_dict(pkg, es, np.array([u] * n))
        o = oracle_bind.OracleModel(orc, case)
        with np.errstate(all="ignore"):
            o.set_state(case["pv"], case["meaning"])
            mob = o.iq()[:, 9:12, 0]
        assert np.isnan(mob).any(), region

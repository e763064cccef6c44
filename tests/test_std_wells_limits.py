"""wells.StandardWells with several rate limits per well - ORAT, WRAT, GRAT, LRAT, RESV beside the well's own target, the BHP and the THP
limit - on the CPU over the oracle: the control rows and the rate converter against np.longdouble restatements, the stated form against
the NumPy form, the wells alone converging onto every kind of limit, the order of update_well_controls, and a list without limits against
the statements the class had before.  (tests/limits_cases.py holds the wells.)

Measured here (numpy 2.2.6), largest relative difference, stated against NumPy form on the SPE9-shaped list with LRAT + RESV limits; the
test asserts 100 x these, and equality where the measured value is 0: see MEASURED below.

Bounds against the np.longdouble restatements (64-bit mantissa: its own error is 2^-11 of a double's): a control row is at most five
roundings of terms of one sign pattern, the converter at most eight, each at most eps/2 of the largest intermediate; the tests hold them to
8 eps of the sum of the terms' magnitudes."""
import numpy as np
import pytest

import helpers
import limits_cases as LC
import oracle_bind
import thp_cases

EPS = np.finfo(float).eps
LD = np.longdouble
DAY = 86400.0

# (resv_current: the voidage rates are elementwise in both forms, but taken at each form's own solved x)
MEASURED = dict(solved_x=3.95e-16, coeff=0.0, resv_current=4.01e-16, control_row=0.0, D_control_row=0.0, res_well=2.76e-15, Dinv=4.11e-16, B=0.0, C=0.0,
                source=0.0, dsource=0.0)


@pytest.fixture(scope="module")
def setup(pkg, orc):
    case = thp_cases.make_case(pkg)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    return dict(case=case, iq=iq, tabs=thp_cases.tables(pkg), props=oracle_bind.OracleFluid(orc, case["fluid"]), model=om,
                avg=pkg.wells.reservoir_averages(iq, case["volume"]))


def build(pkg, setup, wells, arithmetic="stated"):
    w = pkg.wells.StandardWells(wells, setup["case"]["depth"], arithmetic=arithmetic, props=setup["props"], vfp=setup["tabs"], volume=setup["case"]["volume"])
    w.set_reservoir_averages(setup["avg"])
    return w


def solved(pkg, setup, wells, arithmetic="stated"):
    w = build(pkg, setup, wells, arithmetic)
    w.calculate_explicit_quantities(setup["iq"])
    w.solve_well_equations(setup["iq"])
    return w


# ---- 1. the control rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["orat", "wrat", "grat", "lrat", "resv", "resv_injector"])
def test_control_row_against_a_longdouble_restatement(pkg, setup, kind):
    W = pkg.wells
    O, Wa, G = W.OIL, W.WATER, W.GAS
    limit = 3.7e-4
    if kind == "resv_injector":
        well = LC.injector(pkg, setup["case"], ("resv", limit), {"resv": limit})
    else:
        well = LC.producer(pkg, setup["case"], (kind, limit), {kind: limit}, use_list_target=False)
    ws = build(pkg, setup, [well])
    ws.calculate_explicit_quantities(setup["iq"])
    x = np.array([-3.1e-4, -1.7e-5, -8.3e-2, 231.5e5]) if well.producer else np.array([0.0, 6.9e-4, 0.0, 262e5])
    ws.x[0] = x
    r, g = ws._control_rows()
    c = ws.resv_coeff[0]
    xl, cl, L = [LD(v) for v in x], [LD(v) for v in c], LD(limit)
    want_g = np.zeros(4)
    if kind in ("orat", "wrat", "grat"):
        comp = dict(orat=O, wrat=Wa, grat=G)[kind]
        want, mag = xl[comp] + L, abs(xl[comp]) + L
        want_g[comp] = 1.0
    elif kind == "lrat":
        want, mag = (xl[O] + xl[Wa]) + L, abs(xl[O]) + abs(xl[Wa]) + L
        want_g[[O, Wa]] = 1.0
    elif kind == "resv":
        want = ((cl[Wa] * xl[Wa] + cl[O] * xl[O]) + cl[G] * xl[G]) + L
        mag = abs(cl[Wa] * xl[Wa]) + abs(cl[O] * xl[O]) + abs(cl[G] * xl[G]) + L
        want_g[:3] = c
        assert np.array_equal(c, W.calc_coeff(setup["props"], setup["avg"], 0)) and np.all(c != 0.0)
    else:
        want, mag = cl[Wa] * xl[Wa] - L, abs(cl[Wa] * xl[Wa]) + L
        want_g[Wa] = c[Wa]
        assert np.array_equal(c, W.calc_inj_coeff(setup["props"], setup["avg"], 0)) and c[Wa] > 0.0
    assert abs(LD(r[0]) - want) <= 8 * EPS * mag and r[0] != 0.0
    assert np.array_equal(g[0], want_g)
    # ... and the row is where _assemble_wells puts it
    rw, D, *_ = ws._assemble_wells(setup["iq"])
    assert rw[0, 3] == r[0] and np.array_equal(D[0, 3], want_g)


# ---- 2. the rate converter -------------------------------------------------------------------------------------------------------------------
def longdouble_coeff(bw, bo, bg, Rs, Rv):
    bw, bo, bg, Rs, Rv = (LD(v) for v in (bw, bo, bg, Rs, Rv))
    detR = 1 - Rs * Rv
    return np.array([1 / (bo * detR) - Rs / (bg * detR), 1 / bw, 1 / (bg * detR) - Rv / (bo * detR)]), \
        np.array([1 / (bo * detR) + Rs / (bg * detR), 1 / bw, 1 / (bg * detR) + Rv / (bo * detR)])


@pytest.fixture(scope="module")
def wet(pkg, orc):
    return oracle_bind.OracleFluid(orc, helpers.wetgas_fluid(pkg))


def test_calc_coeff_and_calc_inj_coeff_against_longdouble(pkg, wet):
    W = pkg.wells
    avg = np.array([231.0e5, 95.0, 1.1e-4, 1.0, 1.0])
    p = avg[:1]
    bw, bo = wet.probe(p)[0, W.INVBW], wet.probe(p, avg[1])[0, W.INVBO]
    bg = wet.probe_gas(p, avg[2])[0, W.G_INVB]
    want, mag = longdouble_coeff(bw, bo, bg, avg[1], avg[2])
    got = W.calc_coeff(wet, avg, 0)
    assert np.all(np.abs(got.astype(LD) - want) <= 8 * EPS * mag) and np.all(got != 0.0)
    assert got[W.OIL] < 1.0 / bo            # the gas that leaves solution is taken off the oil's coefficient
    bo0, bg0 = wet.probe(p, 0.0)[0, W.INVBO], wet.probe_gas(p, 0.0)[0, W.G_INVB]
    assert np.array_equal(W.calc_inj_coeff(wet, avg, 0), [1.0 / bo0, 1.0 / bw, 1.0 / bg0])


@pytest.mark.parametrize("q,sides", [((-1.0, -0.2, -200.0), ("average", "average")), ((-1.0, -0.2, -50.0), ("ratio", "average")),
                                     ((-1.0e-6, -0.2, -1.0), ("average", "ratio")), ((0.0, 0.5, 0.0), ("ratio", "ratio"))])
def test_calc_reservoir_voidage_rates_against_longdouble(pkg, wet, q, sides):
    """q = (oil, water, gas) surface rates; sides: which argument of min() the state takes for Rs and for Rv (the last state, an injector of
    water alone, has both ratios 0)"""
    W = pkg.wells
    avg = np.array([231.0e5, 95.0, 1.1e-4, 1.0, 1.0])
    qo, qw, qg = q
    ratio_s, ratio_v = qg / (qo + 1.0e-15), qo / (qg + 1.0e-15)
    assert (("ratio" if ratio_s < avg[1] else "average"), ("ratio" if ratio_v < avg[2] else "average")) == sides
    Rs, Rv = min(avg[1], ratio_s), min(avg[2], ratio_v)
    p = avg[:1]
    bw, bo, bg = wet.probe(p)[0, W.INVBW], wet.probe(p, Rs)[0, W.INVBO], wet.probe_gas(p, Rv)[0, W.G_INVB]
    l = lambda v: LD(v)
    detR = 1 - l(Rs) * l(Rv)
    want = np.array([(l(qo) - l(Rv) * l(qg)) / (l(bo) * detR), l(qw) / l(bw), (l(qg) - l(Rs) * l(qo)) / (l(bg) * detR)])
    mag = np.array([(abs(l(qo)) + abs(l(Rv) * l(qg))) / (l(bo) * detR), abs(l(qw)) / l(bw), (abs(l(qg)) + abs(l(Rs) * l(qo))) / (l(bg) * detR)])
    got = W.calc_reservoir_voidage_rates(wet, avg, q, 0)
    assert np.all(np.abs(got.astype(LD) - want) <= 8 * EPS * mag)
    assert np.all(np.sign(got) == np.sign(want.astype(float)))


# ---- 3. the stated form against the NumPy form ------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, float).ravel(), np.asarray(b, float).ravel()
    s = np.maximum(np.abs(a), np.abs(b))
    return float(np.max(np.where(s > 0.0, np.abs(a - b) / np.where(s > 0.0, s, 1.0), 0.0))) if a.size else 0.0


def rel_rows(a, b):
    """largest difference of a row of 4 x 4 matrices relative to the row's largest entry (the entries of one row of D^-1 have one unit)"""
    a, b = np.asarray(a, float).reshape(-1, 4), np.asarray(b, float).reshape(-1, 4)
    return float((np.abs(a - b).max(axis=1) / np.maximum(np.abs(a).max(axis=1), 1e-300)).max())


# Under their oil target of 1500 stb/day the producers give 0.0004 - 0.0009 stb/day of water (S_w is near connate) and take 3600 - 4700 stb/day
# of reservoir volume: a liquid limit a hair above the oil target binds for those with the most water, a voidage limit of 4000 for the larger
# of the others, the rest keep their oil target - all three kinds of row in one list
LRAT_STB_DAY, RESV_STB_DAY = 1500.00065, 4000.0


def test_stated_form_against_the_numpy_form_on_the_spe9_shaped_list(pkg, orc):
    case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    props = oracle_bind.OracleFluid(orc, case["fluid"])
    forms = {}
    for a in ("numpy", "stated"):
        lst = pkg.decks.spe9_shaped_wells(case, liquid_rate_stb_day=LRAT_STB_DAY, resv_rate=RESV_STB_DAY * pkg.decks.STB_PER_DAY).wells
        w = pkg.wells.StandardWells(lst, case["depth"], arithmetic=a, props=props, volume=case["volume"])
        iqr = w.records(om)                      # the averages: the model has no reservoir_averages of its own - the sequential loop
        w.calculate_explicit_quantities(iqr)
        w.solve_well_equations(iqr)
        w.update_well_controls()
        w.solve_well_equations(iqr)
        forms[a] = w
    wn, ws = forms["numpy"], forms["stated"]
    modes = [w.control[0] for w in ws.wells]
    assert modes == [w.control[0] for w in wn.wells] and {"rate", "lrat", "resv"} <= set(modes), modes
    got = dict(solved_x=rel(wn.x, ws.x), coeff=rel(wn.resv_coeff, ws.resv_coeff), resv_current=rel(wn.resv_current, ws.resv_current))
    x0 = ws.x.copy()
    x0[:, :3] *= 1.03
    x0[:, 3] += np.where([w.producer for w in ws.wells], -2e5, 3e5)
    wn.x, ws.x = x0.copy(), x0.copy()
    rn, Dn, *_ = wn._assemble_wells(iq)
    rs, Ds, *_ = ws._assemble_wells(iq)
    got["control_row"], got["D_control_row"] = rel(rn[:, 3], rs[:, 3]), rel(Dn[:, 3], Ds[:, 3])
    an, a_s = wn.assemble(iq), ws.assemble(iq)
    got["res_well"] = rel(an["res_well"], a_s["res_well"])
    got["Dinv"] = rel_rows(an["wells"]["Dnnzs"], a_s["wells"]["Dnnzs"])
    got["B"], got["C"] = rel(an["wells"]["Bnnzs"], a_s["wells"]["Bnnzs"]), rel(an["wells"]["Cnnzs"], a_s["wells"]["Cnnzs"])
    got["source"], got["dsource"] = rel(an["source_cells"], a_s["source_cells"]), rel(an["dsource_cells"], a_s["dsource_cells"])
    print("limits, stated against numpy:", {k: "%.2e" % v for k, v in got.items()}, "controls", sorted(set(modes)))
    assert np.all(rs[:, 3] != 0.0)
    for k, v in got.items():
        bound = 100.0 * MEASURED[k]
        assert v <= bound, (k, v, bound)          # a measured 0 asks for equality


# ---- 4. the wells alone converge onto every kind of limit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["orat", "wrat", "grat", "lrat", "resv", "resv_injector"])
@pytest.mark.parametrize("arithmetic", ["stated", "numpy"])
def test_the_wells_alone_converge_onto_the_limit(pkg, setup, kind, arithmetic):
    W = pkg.wells
    free = solved(pkg, setup, [LC.producer(pkg, setup["case"], None, {})])           # under its own oil target: what the well gives
    q = -free.x[0, :3]
    value = dict(orat=0.7 * q[W.OIL], wrat=0.7 * q[W.WATER], grat=0.7 * q[W.GAS], lrat=0.7 * (q[W.OIL] + q[W.WATER]), resv=40.0 / DAY, resv_injector=50.0 / DAY)[kind]
    assert value > 0.0
    if kind == "resv_injector":
        well = LC.injector(pkg, setup["case"], ("resv", value), {"resv": value}, use_list_target=False)
    else:
        well = LC.producer(pkg, setup["case"], (kind, value), {kind: value}, use_list_target=False)
    ws = solved(pkg, setup, [well], arithmetic)
    x, c = ws.x[0], ws.resv_coeff[0]
    combination = dict(orat=-x[W.OIL], wrat=-x[W.WATER], grat=-x[W.GAS], lrat=-(x[W.OIL] + x[W.WATER]),
                       resv=-((c[W.WATER] * x[W.WATER] + c[W.OIL] * x[W.OIL]) + c[W.GAS] * x[W.GAS]), resv_injector=c[W.WATER] * x[W.WATER])[kind]
    scale = max(np.abs(x[:3]).max(), 1e-9)
    print(kind, arithmetic, "combination %.17g limit %.17g" % (combination, value))
    assert abs(combination - value) <= 1e-7 * scale * max(1.0, np.abs(c).max())     # getWellConvergence's tolerance on the control equation
    r, *_ = ws._assemble_wells(setup["iq"])
    assert ws.converged(r) and np.all(x[:3] <= 0.0 if well.producer else x[:3] >= 0.0) and np.abs(x[:3]).max() > 0.0


# ---- 5. the order of the checks ---------------------------------------------------------------------------------------------------------------
def pairs(order):
    return [(order, order[i], order[i + 1]) for i in range(len(order) - 1)]


@pytest.mark.parametrize("order,first,second", pairs(LC.PRODUCER_ORDER) + pairs(LC.INJECTOR_ORDER),
                         ids=lambda v: v if isinstance(v, str) else ("producer" if v is LC.PRODUCER_ORDER else "injector"))
def test_of_two_violated_limits_the_earlier_wins(pkg, setup, order, first, second):
    is_prod = order is LC.PRODUCER_ORDER
    x_flow = np.array([-4.6e-4, -2.0e-6, -0.12, 0.0]) if is_prod else np.array([0.0, 6.9e-4, 0.0, 0.0])
    bystander = [k for k in order if k not in (first, second)][-1 if first == "bhp" else 0]     # a control in force whose own limit holds

    def switched(in_force):
        well, bhp = LC.ordered_pair_well(pkg, setup["case"], order, first, second, in_force)
        ws = build(pkg, setup, [well])
        ws.calculate_explicit_quantities(setup["iq"])
        ws.x[0] = x_flow
        ws.x[0, 3] = bhp
        ws.update_well_controls()
        return "rate" if well.control == well.rate_control else well.control[0], ws

    own = "orat" if is_prod else "rate"
    name = lambda k: "rate" if k == own else k
    got, ws = switched(bystander)
    assert got == name(first), (got, first, second)
    if "resv" in (first, second):
        assert ws.resv_current[0] > 0.0
    # a violated limit that is the control in force does not count: the later one of the pair wins
    got, _ = switched(first)
    assert got == name(second), (got, first, second)
    # ... and with the later one in force the earlier still wins
    got, _ = switched(second)
    assert got == name(first)


def test_nothing_violated_nothing_switches_and_the_state_stays(pkg, setup):
    lim = {k: LC.NEVER for k in ("wrat", "grat", "lrat", "resv")}
    well = LC.producer(pkg, setup["case"], ("lrat", LC.NEVER), lim, thp_limit=1.0)
    ws = build(pkg, setup, [well])
    ws.calculate_explicit_quantities(setup["iq"])
    ws.x[0] = [-4.6e-5, -2.0e-6, -0.012, thp_cases.PROD_BHP_LIMIT + 40e5]
    before = ws.x.copy()
    ws.update_well_controls()
    assert well.control == ("lrat", LC.NEVER) and np.array_equal(ws.x, before)
    # a switch to a rate-type mode leaves the state as it is (updateWellStateWithTarget's rescaling is left out)
    well.limits["grat"] = LC.ALWAYS
    ws.update_well_controls()
    assert well.control == ("grat", LC.ALWAYS) and np.array_equal(ws.x, before)


# ---- 6. what is refused ---------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, setup):
    W, case = pkg.wells, setup["case"]
    P = lambda **kw: LC.producer(pkg, case, kw.pop("control", None), kw.pop("limits", {}), **kw)
    for bad, text in ((dict(limits={"lrat": 0.0}), "not > 0"), (dict(limits={"lrat": -1.0}), "not > 0"), (dict(limits={"resv": float("nan")}), "not > 0"),
                      (dict(limits={"resv": -np.inf}), "not > 0"), (dict(limits={"orat": 1.0}), "same component"), (dict(limits={"crat": 1.0}), "unknown limit"),
                      (dict(limits={"lrat": 1.0}, use_list_target=False), "use_list_target=False for a well under its own rate target"),
                      (dict(control=("lrat", 1.0), limits={"grat": 1.0}), "LRAT control needs that limit"),
                      (dict(control=("lrat", 2.0), limits={"lrat": 1.0}), "LRAT control needs that limit")):
        with pytest.raises(ValueError, match=text):
            P(**bad)
    with pytest.raises(ValueError, match="producer's"):
        LC.injector(pkg, case, None, {"lrat": 1.0})
    assert P(limits={"lrat": np.inf, "resv": None}).limits == {}                # +infinity / None: no such limit
    assert P(limits={"orat": 1.0}, control=("orat", 1.0), use_list_target=False).limits == {"orat": 1.0}
    # a RESV limit needs the property functions and the averages
    ws = W.StandardWells([P(limits={"resv": 1.0})], case["depth"], arithmetic="stated")
    with pytest.raises(ValueError, match="RESV limit needs props"):
        ws.calculate_explicit_quantities(setup["iq"])
    ws = W.StandardWells([P(limits={"resv": 1.0})], case["depth"], arithmetic="stated", props=setup["props"])
    with pytest.raises(ValueError, match="volumes"):
        ws.records(setup["model"])
    assert W.CONTROL_CODE == {"rate": 0, "bhp": 1, "thp": 2, "orat": 3, "wrat": 4, "grat": 5, "lrat": 6, "resv": 7}


def test_the_averages_come_from_the_model_and_are_frozen_with_the_coefficients(pkg, setup):
    W, case = pkg.wells, setup["case"]

    class WithAverages:
        """a model that has reservoir_averages(), as capi.HipModel"""
        def __init__(self, om, avg):
            self.om, self.avg, self.asked = om, avg, 0

        def iq(self):
            return self.om.iq()

        def reservoir_averages(self):
            self.asked += 1
            return self.avg

    other = setup["avg"] * [1.02, 0.9, 1.0, 1.0, 1.0]
    m = WithAverages(setup["model"], other)
    ws = W.StandardWells([LC.producer(pkg, case, None, {"resv": 40.0 / DAY})], case["depth"], arithmetic="stated", props=setup["props"])
    iq = ws.records(m)
    assert m.asked == 1 and np.all(ws.resv_coeff == 0.0)
    ws.calculate_explicit_quantities(iq)
    assert np.array_equal(ws.resv_averages, other) and np.array_equal(ws.resv_coeff[0], W.calc_coeff(setup["props"], other, 0))
    frozen = ws.resv_coeff.copy()
    m.avg = setup["avg"]
    ws.records(m)                                 # a Newton iteration's records: the next time step's averages wait
    ws.solve_well_equations(iq)
    assert np.array_equal(ws.resv_coeff, frozen) and np.array_equal(ws.resv_averages, other)
    ws.calculate_explicit_quantities(iq)
    assert np.array_equal(ws.resv_averages, setup["avg"]) and not np.array_equal(ws.resv_coeff, frozen)
    # a list without a RESV limit asks the model for nothing more than before
    m2 = WithAverages(setup["model"], other)
    W.StandardWells([LC.producer(pkg, case, None, {"lrat": 1.0})], case["depth"]).records(m2)
    assert m2.asked == 0


# ---- 7. a list without limits computes what it computed --------------------------------------------------------------------------------------
def statements_before_limits(ws):
    """StandardWells._control_rows and update_well_controls as they were before Well(limits=) existed, bound to ws"""
    import importlib
    M = importlib.import_module(type(ws).__module__)
    vfp_mod, OIL, WATER, GAS = M.vfp_mod, M.OIL, M.WATER, M.GAS

    def control_rows():
        r, g = np.zeros(ws.nw), np.zeros((ws.nw, 4))
        for k, (w, x) in enumerate(zip(ws.wells, ws.x)):
            if ws.thp_tables[k] is not None:
                V = ws._bhp_at_thp_limit(k)
                ws._from_thp[k] = V[0] - ws.thp_dp[k]
            if w.control[0] == "thp":
                r[k] = x[3] - ws._from_thp[k]
                g[k, OIL], g[k, WATER], g[k, GAS], g[k, 3] = 0.0 - V[7], 0.0 - V[6], 0.0 - V[8], 1.0
            elif w.control[0] == "bhp":
                r[k], g[k, 3] = x[3] - w.control[1], 1.0
            else:
                comp, target = w.control[1], w.control[2]
                r[k], g[k, comp] = x[comp] - (-1.0 if w.producer else 1.0) * target, 1.0
        return r, g

    def update_well_controls():
        for k, (w, x) in enumerate(zip(ws.wells, ws.x)):
            sign = -1.0 if w.producer else 1.0
            t = ws.thp_tables[k]
            if t is not None:
                ws.thp_current[k] = vfp_mod.thp(t, float(x[WATER]), float(x[OIL]), float(x[GAS]), float(x[3] + ws.thp_dp[k]), w.alq)
            if w.control[0] != "bhp" and ((w.producer and x[3] < w.bhp_limit) or (not w.producer and x[3] > w.bhp_limit)):
                w.control = ("bhp", w.bhp_limit)
                x[3] = w.bhp_limit
            elif w.control[0] != "rate" and sign * x[w.rate_control[1]] > w.rate_control[2]:
                w.control = w.rate_control
            elif t is not None and w.control[0] != "thp" and (w.thp_limit > ws.thp_current[k] if w.producer else w.thp_limit < ws.thp_current[k]):
                w.control = ("thp", w.thp_limit)
                x[3] = ws._bhp_at_thp_limit(k)[0] - ws.thp_dp[k]

    ws._control_rows, ws.update_well_controls = control_rows, update_well_controls
    return ws


@pytest.mark.parametrize("arithmetic", ["stated", "numpy"])
def test_a_list_without_limits_gives_the_arrays_it_gave(pkg, setup, arithmetic):
    """the THP case's wells through its switching table (every branch of the three old controls), once with the class as it is and once
    with the two methods this change touched put back as they were: equal arrays, equal controls"""
    case, iq = setup["case"], setup["iq"]

    def run(old):
        ws = pkg.wells.StandardWells(thp_cases.make_wells(pkg, case), case["depth"], arithmetic=arithmetic, vfp=setup["tabs"])
        if old:
            statements_before_limits(ws)
        ws.calculate_explicit_quantities(iq)
        ws.solve_well_equations(iq)
        out = [ws.x.copy()]
        x_solved = ws.x.copy()
        for name, k, before, xk, after in thp_cases.transitions(x_solved):
            ws.x = x_solved.copy()
            ws.x[k] = xk
            ws.wells[k].control = thp_cases.control_of(ws.wells[k], before)
            ws.update_well_controls()
            assert ws.wells[k].control[0] == after, name
            a = ws.assemble(iq)
            out += [ws.x.copy(), a["res_well"], a["wells"]["Bnnzs"], a["wells"]["Cnnzs"], a["wells"]["Dnnzs"], a["source_cells"], a["dsource_cells"],
                    np.array([pkg.wells.CONTROL_CODE[w.control[0]] for w in ws.wells])]
            for w in ws.wells:
                w.control = w.rate_control
        return out

    new, old = run(False), run(True)
    assert len(new) == len(old) and all(np.array_equal(a, b) for a, b in zip(new, old))


def test_spe9_shaped_wells_defaults_give_the_list_of_before(pkg):
    case = pkg.decks.cartesian_case(24, 25, 15, state="mixed", heterogeneous=True)
    a = pkg.decks.spe9_shaped_wells(case)
    assert all(w.limits == {} and w.use_list_target for w in a.wells) and not a.has_resv
    b = pkg.decks.spe9_shaped_wells(case, liquid_rate_stb_day=1800.0, resv_rate=3e-3)
    assert all(w.limits == {"lrat": 1800.0 * pkg.decks.STB_PER_DAY, "resv": 3e-3} for w in b.wells[1:]) and b.wells[0].limits == {} and b.has_resv
    for wa, wb in zip(a.wells, b.wells):
        assert np.array_equal(wa.cells, wb.cells) and np.array_equal(wa.tw, wb.tw) and wa.control == wb.control and wa.bhp_limit == wb.bhp_limit

"""Open boundaries resident on the device (opmhip_set_boundary_conditions: FREE and RATE faces of the BC keyword) against their CPU form
boundary.HostBoundary and the CPU oracle, bit for bit: the rates of the faces, the assembled Jacobian and residual, three time steps of
the Newton loop, a chopped step, the refusals, the absence of a list - and, independent of any restatement, the balance of the fluids in
place against what the boundary and the sources moved.

Grids: 9 x 9 x 2 with all six sides listed (234 faces, 162 distinct cells: more than two waves, not a multiple of 64, corner cells with
three faces; the I- side RATE, the rest FREE, so the I- column's cells have both kinds), 3 x 1 x 1 (five faces per end cell) and a list
of one face; the base record and the extended one (PVTG: Rv and the transmissibility multiplier's field)."""
import uuid

import numpy as np
import pytest

import helpers
import oracle_bind

pytestmark = pytest.mark.gpu

DAY = 86400.0
SIDES = ("I-", "I+", "J-", "J+", "K-", "K+")
INFLUX = [0.0, -2.0e-4, 0.0]          # kg / (m^2 s) of water, negative: into the domain


def make_case(pkg, ext, dims=(9, 9, 2)):
    """ext: a fluid with PVTG - the extended intensive-quantity record (Rv; helpers.hysteresis_case would be refused with FREE faces)"""
    if ext:
        return helpers.wetgas_case(pkg, *dims, heterogeneous=True)
    return pkg.decks.cartesian_case(*dims, state="mixed", heterogeneous=True)


def whole(case):
    return (0, case["nx"] - 1, 0, case["ny"] - 1, 0, case["nz"] - 1)


def make_records(pkg, case, kind="all"):
    B = pkg.boundary
    if kind == "one":
        return [B.free(B.faces(case, (case["nx"] - 1, case["nx"] - 1, 0, 0, 0, 0), "I+"))]
    if kind == "sector":          # the lateral sides alone: a prescribed water influx through I-, the other three held at the initial state
        return [B.rate(B.faces(case, whole(case), "I-"), INFLUX)] + [B.free(B.faces(case, whole(case), f)) for f in SIDES[1:4]]
    if kind == "lateral_free":
        return [B.free(B.faces(case, whole(case), f)) for f in SIDES[:4]]
    return [B.rate(B.faces(case, whole(case), "I-"), INFLUX)] + [B.free(B.faces(case, whole(case), f)) for f in SIDES[1:]]


def host_form(pkg, case, recs, **kw):
    return pkg.boundary.HostBoundary(recs, case["depth"], case["fluid"], **kw)


def sink(case, rate_sm3_per_day=4.0):
    """a rate sink of oil (with dissolved gas at the saturated Rs) and water in the middle of the top layer"""
    import importlib
    decks = importlib.import_module("opm-autodiff_amd").decks
    src = np.zeros((case["Nb"], 3))
    c = 4 + 9 * 4
    q = rate_sm3_per_day / DAY
    src[c] = [-q, -0.25 * q, -q * float(decks.rs_sat(case["fluid"], case["pv"][3 * c + 1]))]
    return src


def same_state(a, b):
    pa, ma = a.get_state()
    pb, mb = b.get_state()
    return np.array_equal(ma, mb) and np.array_equal(pa, pb)


def moved(case, seed, sign=-1.0, dp=2.0e5):
    """the aquifer test's iterate away from the state of the step's start; sign: pressure below (-1) or above (+1) it"""
    rng = np.random.default_rng(seed)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 1] += sign * dp * rng.uniform(0.5, 1.0, len(pv))
    pv[:, 0] += rng.uniform(-0.01, 0.01, len(pv))
    return pv.reshape(-1)


# ---- 1. rates ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("grid", ["9x9x2", "3x1x1", "one"])
def test_rates_equal_the_host_form(pkg, ext, grid):
    """the twelve numbers of every face at the capture state, at an iterate below and one above the captured pressure (both upwind
    branches, both compositions) and after a second capture"""
    case = make_case(pkg, ext, (3, 1, 1) if grid == "3x1x1" else (9, 9, 2))
    recs = make_records(pkg, case, "one" if grid == "one" else "all")
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_boundary_conditions(recs)
    h = host_form(pkg, case, recs)
    h.initial_solution_applied(m)
    nf = {"9x9x2": 234, "3x1x1": 14, "one": 1}[grid]
    assert len(h.cells) == nf and len(np.unique(h.cells)) == {"9x9x2": 162, "3x1x1": 3, "one": 1}[grid]
    if grid == "3x1x1":
        assert list(np.bincount(h.cells)) == [5, 4, 5]
    if grid != "one":
        both = np.intersect1d(h.cells[h.free], h.cells[~h.free])
        assert len(both) > 0                                           # cells with a RATE and a FREE face
    assert m.boundary_rates().shape == (nf, 12) and np.all(m.boundary_rates() == 0.0)
    dt = 5.0 * DAY
    seen_up, seen_comp = set(), set()

    def compare(tag):
        m.assemble(dt, 0, fetch=False)
        q = m.boundary_rates()
        want = h.rates_now(m)
        assert np.array_equal(q, want), (tag, np.abs(q - want).max())
        seen_up.update(np.unique(h.upwind_exterior[h.free]).tolist())
        seen_comp.update(np.unique(h.composition[h.free]).tolist())
        return q

    q = compare("capture")
    lateral = h.free & (h.direction < 4)
    assert np.all(q[lateral] == 0.0)                                   # no flux at equilibrium, to the bit
    assert np.all(q[~h.free, :3] == (h.mass_rate / h.rho_ref * h.area[:, None])[~h.free]) and np.all(q[~h.free, 3:] == 0.0)
    for step, sign in enumerate((-1.0, 1.0)):
        m.set_state(moved(case, step, sign), case["meaning"])
        q = compare("moved %+d" % sign)
        assert np.all(np.any(q[h.free, :3] != 0.0, axis=1)) and np.all(np.any(q[h.free, 3:] != 0.0, axis=1))
        assert np.all(h.upwind_exterior[lateral] == (sign < 0)) and np.all(h.composition[h.free] == (1 if sign < 0 else -1))
    assert seen_up == {False, True} and seen_comp >= {-1, 1}           # both upwind branches, both compositions occurred
    # a second call captures again: the moved state is now the exterior one
    m.set_boundary_conditions(recs)
    h.initial_solution_applied(m)
    q = compare("second capture")
    assert np.all(q[lateral] == 0.0)
    m.set_state(case["pv"], case["meaning"])
    q = compare("back at the first state")
    assert np.all(np.any(q[h.free, :3] != 0.0, axis=1))


# ---- 2. assembly --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_assembly_equals_the_rates_handed_in_as_source(pkg, ext):
    """J and r with the list = J and r with HostBoundary's numbers handed in as source; a boundary cell also sits in an aquifer and carries
    a caller's source and derivative; the caller's arrays are unchanged afterwards"""
    case = make_case(pkg, ext)
    recs = make_records(pkg, case)
    A = pkg.aquifers
    under = A.connections(case, (0, 8, 0, 8, 1, 1), "K+")
    aq = [A.fetkovich(1, under, 2.0e6, 5.0e-8, 1.0e-9, 1.0e8, 1010.0, float(case["depth"].max()) + 2.5, initial_pressure=255.0e5)]
    Nb = case["Nb"]
    src = sink(case)
    src[81] = [1e-5, 3e-4, -2e-5]                    # a caller's rate on a cell with a RATE face, two FREE faces and an aquifer connection ...
    dsrc = np.zeros((Nb, 9))
    dsrc[81] = [1e-4, -3e-10, 2e-5, 1e-3, -2e-9, 5e-4, 0.0, 4e-10, -1e-5]      # ... with a full derivative block
    src[40 + 81] = [0.0, 1e-4, 0.0]                  # ... and on an interior cell of the bottom layer (K+ face, aquifer)
    dt = 5.0 * DAY
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src.reshape(-1), dsrc.reshape(-1))
    m.set_aquifers(aq)
    m.set_boundary_conditions(recs)
    h = host_form(pkg, case, recs)
    h.initial_solution_applied(m)
    assert 81 in h.cells[h.free] and 81 in h.cells[~h.free] and 81 in under["cells"]
    m.aquifers_begin_time_step(10.0 * DAY, dt)
    m.set_state(moved(case, 5), case["meaning"])
    j1, r1 = m.assemble(dt, 0)
    q, qa = m.boundary_rates(), m.aquifer_rates()
    assert np.array_equal(q, h.rates_now(m))
    j1b, r1b = m.assemble(dt, 1)                         # every assemble forms the rates again, from the arrays the caller left
    m.set_boundary_conditions(None)
    ja, ra = m.assemble(dt, 0)                           # the aquifer alone
    m.set_aquifers(None)
    j0, r0 = m.assemble(dt, 0)
    plain = pkg.capi.HipModel(case)                      # a context that never had either
    plain.set_state(moved(case, 5), case["meaning"])
    plain.set_source(src.reshape(-1), dsrc.reshape(-1))
    jp, rp = plain.assemble(dt, 0)
    assert np.array_equal(j0, jp) and np.array_equal(r0, rp)         # the caller's arrays were not disturbed
    assert not np.array_equal(r1, ra) and not np.array_equal(j1, ja) and not np.array_equal(ra, r0)
    s, d = src.copy(), dsrc.copy()
    s[under["cells"], 1] += qa[:, 0]                     # the aquifer first (the device's order) ...
    d[under["cells"], 3:6] += qa[:, 1:]
    for f, c in enumerate(h.cells):                      # ... then the faces, one after the other in list order
        s[c] = s[c] - q[f, :3]
        d[c] = d[c] - q[f, 3:]
    m.set_source(s.reshape(-1), d.reshape(-1))
    j2, r2 = m.assemble(dt, 0)
    assert np.array_equal(j1, j2) and np.array_equal(r1, r2)
    j3, r3 = m.assemble(dt, 1)
    assert np.array_equal(j1b, j3) and np.array_equal(r1b, r3)


# ---- 3. lock step ---------------------------------------------------------------------------------------------------------------------------
def two_forms(pkg, case, recs, src):
    ms, bms = [], []
    for form in ("device", "host"):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        if form == "device":
            m.set_source(src)
            b = pkg.boundary.DeviceBoundary(recs)
        else:
            b = host_form(pkg, case, recs, base_source=src)
        ms.append(m)
        bms.append(pkg.newton.BlackoilModelHip(m, boundary_model=b))
    return ms, bms


def test_three_time_steps_device_form_against_host_form(pkg):
    """a sector: a box with open lateral sides and a producer's sink, through newton.BlackoilModelHip with the boundary resident on the
    device - the same sub-steps, iteration counts and states as with the host form.  (The lateral sides only: a FREE top or bottom face
    holds the cell centre's pressure at the face's depth, so a hydrostatic column is never at rest against it and the loop's time steps
    of ten and twenty days do not converge - DESIGN.md section 5)"""
    case = make_case(pkg, False)
    recs = make_records(pkg, case, "sector")
    ms, bms = two_forms(pkg, case, recs, sink(case).reshape(-1))
    time = 0.0
    for dt in (2.0 * DAY, 10.0 * DAY, 20.0 * DAY):
        reps = []
        for bm in bms:
            bm.advance_time_level()
            bm.begin_time_step(dt, time=time)
            reps.append(bm.step(dt))
            bm.end_time_step(dt)
        assert reps[0].converged and reps[1].converged
        assert reps[0].total_newton_iterations == reps[1].total_newton_iterations >= 2
        assert reps[0].total_linear_iterations == reps[1].total_linear_iterations
        assert same_state(ms[0], ms[1])
        assert np.array_equal(bms[0].boundary.rates(ms[0]), bms[1].boundary.Q)
        time += dt
    q = ms[0].boundary_rates()
    assert np.all(np.any(q[:, :3] != 0.0, axis=1))


def test_chopped_step(pkg):
    """advance_time_level, two iterations of dt, update_failed, then dt / 2 to the end: the captured state is not the step's, so both forms
    go on in lock step and the first rates after the roll-back are those of the rolled-back records"""
    case = make_case(pkg, False)
    recs = make_records(pkg, case, "sector")
    ms, bms = two_forms(pkg, case, recs, sink(case).reshape(-1))
    dt = 20.0 * DAY
    start = ms[0].get_state()
    for m, bm in zip(ms, bms):
        bm.advance_time_level()
        bm.begin_time_step(dt)
        for it in range(2):
            bm.nonlinear_iteration(it, dt)
        assert not np.array_equal(m.get_state()[0], start[0])
        m.update_failed()
        assert np.array_equal(m.get_state()[0], start[0])
        bm.begin_time_step(0.5 * dt)
    h = bms[1].boundary
    ms[0].assemble(0.5 * dt, 0, fetch=False)
    assert np.array_equal(ms[0].boundary_rates(), h.rates_now(ms[0]))
    reps = [bm.step(0.5 * dt) for bm in bms]
    assert reps[0].converged and reps[0].total_newton_iterations == reps[1].total_newton_iterations >= 2
    assert same_state(ms[0], ms[1]) and not np.array_equal(ms[0].get_state()[0], start[0])


@pytest.mark.parametrize("ext", [False, True])
def test_three_time_steps_against_the_oracle(pkg, orc, ext):
    """the comparison of tests/test_gpu_aquifers.py: Jacobian, residual and state bit for bit at every iteration, the oracle's solution
    applied on both sides; the oracle's model carries HostBoundary"""
    case = make_case(pkg, ext)
    recs = make_records(pkg, case)
    src = sink(case).reshape(-1)
    m = pkg.capi.HipModel(case, reorder="line_coloring")
    o = oracle_bind.OracleModel(orc, case)
    for q in (m, o):
        q.set_state(case["pv"], case["meaning"])
    m.set_source(src)
    m.set_boundary_conditions(recs)
    h = host_form(pkg, case, recs, base_source=src)
    h.initial_solution_applied(o)
    for step, dt in enumerate([2.0 * DAY, 10.0 * DAY, 20.0 * DAY]):
        m.begin_time_step(dt)
        o.begin_time_step(dt)
        for it in range(4):
            h.add_to_source(o)
            jm, rm = m.assemble(dt, it)
            jo, ro = o.assemble(dt, it)
            assert np.array_equal(jm, jo) and np.array_equal(rm, ro), (step, it)
            assert np.array_equal(m.boundary_rates(), h.Q), (step, it)
            x, res = o.solve(tol=1e-6, maxit=200, w=0.9, mode="post_scale", reorder="none")
            m.update(x, 1.0)
            o.update(x)
            assert same_state(m, o)
        h.add_to_source(o)
        jm, rm = m.assemble(dt, 4)
        jo, ro = o.assemble(dt, 4)
        assert np.array_equal(jm, jo) and np.array_equal(rm, ro), step
        for q in (m, o):
            q.end_time_step(dt)
    assert np.any(h.Q[h.free, :3] != 0.0)


# ---- 4. balance -----------------------------------------------------------------------------------------------------------------------------
STEPS = (1.0 * DAY, 3.0 * DAY, 8.0 * DAY, 15.0 * DAY, 30.0 * DAY)
FIP_OIL, FIP_WATER, FIP_GAS = 10, 9, 11                 # fip.TERMS: the rows of fluid_in_place
FIP_OF_EQ = (FIP_OIL, FIP_WATER, FIP_GAS)               # equation order: oil, water, gas


def run_balance(pkg, case, recs, src, steps=STEPS):
    """five steps; -> change of oil, water, gas in place, the time integral of -boundary_rates, of the sources, and the allowed mismatch per
    equation: what the Newton loop converged to - per step MB_e = |B_avg,e R_sum,e| dt / pvSum <= tolerance_mb, i.e. a surface volume of
    tolerance_mb * pvSum / B_avg,e - summed over the steps (test_water_balance_of_a_closed_box)"""
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src.reshape(-1))
    m.set_drift_compensation(False)
    m.set_fip_regions({"FIPNUM": np.ones(case["Nb"], np.int32)})
    bm = pkg.newton.BlackoilModelHip(m, boundary_model=pkg.boundary.DeviceBoundary(recs))
    first = m.fluid_in_place()["field"][list(FIP_OF_EQ)]
    time, allowed, from_sources, from_boundary = 0.0, np.zeros(3), np.zeros(3), np.zeros(3)
    for dt in steps:
        bm.advance_time_level()
        bm.begin_time_step(dt, time=time)
        assert bm.step(dt).converged
        c = m.convergence(dt, bm.param.tolerance_cnv)
        assert np.all(c[14:17] <= bm.param.tolerance_mb)
        allowed += bm.param.tolerance_mb * c[9] / c[6:9]
        from_boundary -= m.boundary_rates()[:, :3].sum(axis=0) * dt      # implicit Euler: the converged rates of a step times its length
        bm.end_time_step(dt)
        from_sources += src.sum(axis=0) * dt
        time += dt
    change = m.fluid_in_place()["field"][list(FIP_OF_EQ)] - first
    return change, from_boundary, from_sources, allowed


def test_water_balance_with_a_rate_influx(pkg):
    """independent of any restatement: with a RATE water influx on the I- side the water in place changes by -sum rate / rho_ref area dt
    plus the sources"""
    case = make_case(pkg, False)
    B = pkg.boundary
    west = B.faces(case, whole(case), "I-")
    recs = [B.rate(west, INFLUX)]
    src = sink(case)
    change, from_boundary, from_sources, allowed = run_balance(pkg, case, recs, src)
    rho_w = case["fluid"].pvt[0]["density"][1]
    stated = -(INFLUX[1] / rho_w) * float(west["area"].sum()) * sum(STEPS)
    mismatch = change - (from_boundary + from_sources)
    print("water in place: change %.6f m3, boundary %.6f (stated %.6f), sources %.6f, mismatch %.3e, allowed %.3e"
          % (change[1], from_boundary[1], stated, from_sources[1], mismatch[1], allowed[1]))
    assert abs(from_boundary[1] - stated) <= 1e-12 * stated and from_boundary[0] == 0.0 and from_boundary[2] == 0.0
    assert stated > 100.0 * allowed[1]                   # the influx is what the balance is about
    assert abs(change[1] - (stated + from_sources[1])) <= allowed[1]


def mobile_water_case(pkg):
    """the base case with a water phase that flows: the SPE1 tables' k_rw stays below 1e-5, so their water never crosses a boundary in
    amounts the balance could see - here k_rw = 0.5 ((Sw - Swco) / (1 - Swco))^2 and Sw around 0.45"""
    fl, d = pkg.fluid.spe1_fluid()
    swof = np.array(d["swof"], float)
    swof[:, 1] = 0.5 * ((swof[:, 0] - swof[0, 0]) / (1.0 - swof[0, 0])) ** 2
    fl = pkg.fluid.Fluid(fl.pvt, [dict(swof=swof.tolist(), sgof=d["sgof"])], rock_pref=fl.rock_pref, rock_cr=fl.rock_cr)
    case = pkg.decks.cartesian_case(9, 9, 2, state="mixed", heterogeneous=True, fluid=fl)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 0] += 0.25
    case["pv"] = np.ascontiguousarray(pv.reshape(-1))
    return case


def test_balance_with_free_sides_around_a_sink(pkg):
    """FREE lateral faces around a sink: oil, water and gas in place change by the time integral of boundary_rates() plus the sources"""
    case = mobile_water_case(pkg)
    recs = make_records(pkg, case, "lateral_free")
    src = sink(case, rate_sm3_per_day=40.0)
    change, from_boundary, from_sources, allowed = run_balance(pkg, case, recs, src, steps=(1.0 * DAY, 2.0 * DAY, 4.0 * DAY, 8.0 * DAY, 10.0 * DAY))
    mismatch = change - (from_boundary + from_sources)
    for e, name in enumerate(("oil", "water", "gas")):
        print("%s in place: change %.6f, boundary %.6f, sources %.6f, mismatch %.3e, allowed %.3e"
              % (name, change[e], from_boundary[e], from_sources[e], mismatch[e], allowed[e]))
    assert np.all(from_boundary > 100.0 * allowed)       # the boundary's inflow is what the balance is about
    assert np.all(np.abs(mismatch) <= allowed)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    case = make_case(pkg, False)
    good = make_records(pkg, case)

    def refused(model, recs, code, word, edit=None):
        bc, keep = C.make_boundary_conditions(recs)
        if edit:
            edit(bc, keep)
        rc = C.lib().opmhip_set_boundary_conditions(model._h, bc)
        msg = C.lib().opmhip_last_error(model._h).decode()
        assert rc == code and word in msg, (rc, msg)

    f = C.HipFluid(case["fluid"])
    refused(f, good, C.NOT_READY, "set_static")
    m = C.HipModel(case)
    refused(m, good, C.NOT_READY, "set_state")
    m.set_state(case["pv"], case["meaning"])
    plain = C.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    jp, rp = plain.assemble(DAY, 0)
    null = lambda name: (lambda bc, keep: setattr(bc, name, None))
    def poke(name, i, v):
        def e(bc, keep):
            keep[name][i] = v
        return e
    cases = [(null(n), "null array") for n in ("cell", "direction", "type", "area", "trans", "depth", "rate")]
    cases += [(poke("cell", 3, 162), "outside [0, 162)"), (poke("cell", 200, -1), "outside [0, 162)"), (poke("direction", 5, 6), "outside 0..5"),
              (poke("direction", 5, -1), "outside 0..5"), (poke("direction", 36, 0), "listed twice"), (poke("area", 7, 0.0), "not positive"),
              (poke("area", 100, -4.0), "not positive"), (poke("trans", 30, -1e-14), "negative or not finite"),
              (poke("trans", 30, np.inf), "negative or not finite"), (poke("trans", 233, np.nan), "negative or not finite"), (poke("type", 50, 2), "unknown type")]
    for edit, word in cases:
        m.set_boundary_conditions(good)
        refused(m, good, C.INVALID_ARGUMENT, word, edit)
        # after a refused call no list is set and the context is usable: an assemble gives the result of a context without a list
        m._nbcfaces = 0
        j, r = m.assemble(DAY, 0)
        assert np.array_equal(j, jp) and np.array_equal(r, rp), word
        assert m.boundary_rates().shape == (0, 12)
    m.set_boundary_conditions(good)
    j, r = m.assemble(DAY, 0)
    assert not np.array_equal(r, rp)                      # (the RATE faces: a good list is taken afterwards)
    # relative-permeability hysteresis: refused with a FREE face, taken with RATE faces alone
    hc = helpers.hysteresis_case(pkg, 9, 9, 2, heterogeneous=True)
    hm = C.HipModel(hc)
    hm.set_state(hc["pv"], hc["meaning"])
    hm.set_hysteresis(0, hc["imbnum"])
    refused(hm, make_records(pkg, hc), C.INVALID_ARGUMENT, "hysteresis")
    hm.assemble(DAY, 0)
    hm.set_boundary_conditions(make_records(pkg, hc)[:1])
    hm.assemble(DAY, 0)
    assert np.all(hm.boundary_rates()[:, 1] < 0.0)
    # ... and hysteresis switched on behind a list with FREE faces is caught by the next assemble
    late = C.HipModel(hc)
    late.set_state(hc["pv"], hc["meaning"])
    late.set_boundary_conditions(make_records(pkg, hc))
    late.assemble(DAY, 0)
    late.set_hysteresis(0, hc["imbnum"])
    with pytest.raises(C.OpmHipError) as e:
        late.assemble(DAY, 0)
    assert e.value.code == C.INVALID_ARGUMENT and "hysteresis" in str(e.value)
    late.set_boundary_conditions(None)
    late.assemble(DAY, 0)
    # water-induced compaction tables
    wc = helpers.wetgas_case(pkg, 9, 9, 2, heterogeneous=True)
    wc["rocknum"] = (np.arange(wc["Nb"]) % 2).astype(np.int32)
    wc["overburden"] = 20e5 + 50.0 * (wc["depth"] - wc["depth"].min())
    wm = C.HipModel(wc)
    wm.set_state(wc["pv"], wc["meaning"])
    wm.set_water_compaction(helpers.ROCK2D_2)
    refused(wm, make_records(pkg, wc), C.INVALID_ARGUMENT, "water-induced compaction")
    wm.assemble(DAY, 0)
    # a decomposed context (loopback, two ranks): out of scope
    sub = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    dd = C.HipModel(sub, comm=("loopback", 2, 0, "bc" + uuid.uuid4().hex), reorder="level_scheduling")
    dd.set_state(sub["pv"], sub["meaning"])
    one = dict(type="free", cells=[0], direction=[0], area=[100.0], trans=[1e-12], depth=[2500.0])
    refused(dd, [one], C.INVALID_ARGUMENT, "decomposed")


# ---- 6. absence -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_a_context_without_a_list_assembles_the_same_bits(pkg, ext):
    """never set, and set and cleared (NULL, then an empty list): the same Jacobian and residual"""
    case = make_case(pkg, ext)
    src = sink(case).reshape(-1)
    out = []
    for form in ("never", "cleared", "cleared by an empty list"):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        m.set_source(src)
        if form != "never":
            m.set_boundary_conditions(make_records(pkg, case))
            m.set_state(moved(case, 1), case["meaning"])
            j, r = m.assemble(DAY, 0)
            m.set_boundary_conditions(None if form == "cleared" else [])
            assert m.boundary_rates().shape == (0, 12)
        m.set_state(moved(case, 2), case["meaning"])
        out.append(m.assemble(DAY, 0))
    assert not np.array_equal(out[0][1], r)
    for j, r in out[1:]:
        assert np.array_equal(j, out[0][0]) and np.array_equal(r, out[0][1])

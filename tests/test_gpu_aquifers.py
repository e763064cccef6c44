"""Analytic aquifers resident on the device (opmhip_set_aquifers) against their CPU form aquifers.HostAquifers and the CPU oracle,
bit for bit: the rates of the connections, the assembled Jacobian and residual, three time steps of the Newton loop, a chopped step,
the refusals - and, independent of any restatement, the water balance of a closed box.

Grid: 9 x 9 x 2 with a Fetkovich aquifer under the bottom face (81 connections: more than one wave, not a multiple of 64), a Carter-Tracy
aquifer on the I- side (the bottom cells of that column sit in both) and a Carter-Tracy aquifer with one connection."""
import uuid

import numpy as np
import pytest

import helpers
import oracle_bind

pytestmark = pytest.mark.gpu

DAY = 86400.0


def make_case(pkg, ext):
    """ext: a fluid with pc_scaling - the extended intensive-quantity record and a non-zero capillary pressure (p_w depends on Sw)"""
    if ext:
        return helpers.hysteresis_case(pkg, 9, 9, 2, heterogeneous=True)
    return pkg.decks.cartesian_case(9, 9, 2, state="mixed", heterogeneous=True)


def make_records(pkg, case, initial_pressure=None):
    A = pkg.aquifers
    under = A.connections(case, (0, 8, 0, 8, 1, 1), "K+")
    side = A.connections(case, (0, 0, 0, 8, 0, 1), "I-")
    one = A.connections(case, (4, 4, 4, 4, 0, 0), "K-")
    assert len(under["cells"]) == 81 and len(side["cells"]) == 18 and len(one["cells"]) == 1 and len(np.intersect1d(under["cells"], side["cells"])) == 9
    datum = float(case["depth"].max()) + 2.5
    td, pd = [0.01, 0.1, 1.0, 3.0], [0.112, 0.315, 0.802, 1.2]      # the later steps of the tests reach beyond the last node
    return [A.carter_tracy(1, side, 2.0e6, 2.0e-3, 1000.0, datum, td, pd, initial_pressure=initial_pressure),
            A.carter_tracy(3, one, 1.0e6, 5.0e-4, 1005.0, datum - 10.0, td, pd, initial_pressure=255.0e5),
            A.fetkovich(2, under, 2.0e6, 5.0e-8, 1.0e-9, 1.0e8, 1010.0, datum, initial_pressure=initial_pressure)]


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


def moved(case, seed, dp=2.0e5):
    """an iterate away from the state of the step's start"""
    rng = np.random.default_rng(seed)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 1] -= dp * rng.uniform(0.5, 1.0, len(pv))
    pv[:, 0] += rng.uniform(-0.01, 0.01, len(pv))
    return pv.reshape(-1)


# ---- 1. rates ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_rates_equal_the_host_form(pkg, ext):
    """value and three derivatives of every connection's Qai_, both types, at time 0 and at a later time with W_flux != 0; the initial
    pressure of two aquifers equilibrated by the library"""
    case = make_case(pkg, ext)
    recs = make_records(pkg, case)
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_aquifers(recs)
    h = pkg.aquifers.HostAquifers(recs, case["depth"])
    h.initial_solution_applied(m)
    d = m.get_aquifers()
    assert np.array_equal(d["init_pressure"], h.data()["init_pressure"]) and d["init_pressure"][1] == 255.0e5 and d["init_pressure"][0] != d["init_pressure"][2]
    assert np.all(m.aquifer_rates() == 0.0) and m.aquifer_rates().shape == (100, 4)
    time = 0.0
    for step, dt in enumerate([0.5 * DAY, 20.0 * DAY, 60.0 * DAY]):
        m.aquifers_begin_time_step(time, dt)
        h.begin_time_step(m, time, dt)
        m.set_state(moved(case, step), case["meaning"])
        m.assemble(dt, 0, fetch=False)
        q = m.aquifer_rates()
        want = h.rates(m.iq_cells(h.cells))
        assert np.array_equal(q, want), (step, np.abs(q - want).max())
        assert np.all(q[:, 0] != 0.0) and np.all(q[:, 2] != 0.0) and (np.any(q[:, 1] != 0.0) == ext)
        m.end_time_step(dt)
        h.end_time_step(dt)
        a, b = m.get_aquifers(), h.data()
        for k in ("W_flux", "pressure", "flux_rate", "init_pressure"):
            assert np.array_equal(a[k], b[k]), (step, k)
        assert np.all(a["W_flux"] != 0.0) and a["pressure"][2] != a["init_pressure"][2]
        m.set_state(case["pv"], case["meaning"])
        time += dt
    assert time / 2.0e6 > 3.0     # the last step read the influence tables beyond their last node


# ---- 2. assembly --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True])
def test_assembly_equals_the_rates_handed_in_as_source(pkg, ext):
    case = make_case(pkg, ext)
    recs = make_records(pkg, case)
    Nb = case["Nb"]
    src = sink(case)
    src[81] = [1e-5, 3e-4, 0.0]                     # a caller's rate on a cell that is in two aquifers ...
    dsrc = np.zeros((Nb, 9))
    dsrc[81, 3:6] = [1e-3, -2e-9, 5e-4]             # ... with a derivative in the water row
    src[5] = [0.0, 1e-4, 0.0]                       # ... and on a cell that is in none (the sink's cell is in the one-connection aquifer)
    dsrc[5, 3:6] = [0.0, -1e-10, 0.0]
    dt = 5.0 * DAY
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src.reshape(-1), dsrc.reshape(-1))
    m.set_aquifers(recs)
    with pytest.raises(pkg.capi.OpmHipError) as e:       # no time step begun
        m.assemble(dt, 0)
    assert e.value.code == pkg.capi.NOT_READY
    m.aquifers_begin_time_step(10.0 * DAY, dt)
    with pytest.raises(pkg.capi.OpmHipError) as e:       # another dt than the one begun
        m.assemble(0.5 * dt, 0)
    assert e.value.code == pkg.capi.INVALID_ARGUMENT
    m.set_state(moved(case, 5), case["meaning"])
    j1, r1 = m.assemble(dt, 0)
    q = m.aquifer_rates()
    j1b, r1b = m.assemble(dt, 1)                         # every assemble forms the influx again, from the arrays the caller left
    m.set_aquifers(None)
    j0, r0 = m.assemble(dt, 0)
    plain = pkg.capi.HipModel(case)                      # a context that never had aquifers
    plain.set_state(moved(case, 5), case["meaning"])
    plain.set_source(src.reshape(-1), dsrc.reshape(-1))
    jp, rp = plain.assemble(dt, 0)
    assert np.array_equal(j0, jp) and np.array_equal(r0, rp)         # the caller's arrays were not disturbed
    assert not np.array_equal(r1, r0) and not np.array_equal(j1, j0)
    s, d = src.copy(), dsrc.copy()
    o = 0
    for r in recs:                                        # aquifer order
        n = len(r["cells"])
        s[r["cells"], 1] += q[o:o + n, 0]
        d[r["cells"], 3:6] += q[o:o + n, 1:]
        o += n
    m.set_source(s.reshape(-1), d.reshape(-1))
    j2, r2 = m.assemble(dt, 0)
    assert np.array_equal(j1, j2) and np.array_equal(r1, r2)
    j3, r3 = m.assemble(dt, 1)
    assert np.array_equal(j1b, j3) and np.array_equal(r1b, r3)


# ---- 3. lock step ---------------------------------------------------------------------------------------------------------------------------
def test_three_time_steps_device_form_against_host_form(pkg):
    case = make_case(pkg, False)
    recs = make_records(pkg, case)
    src = sink(case).reshape(-1)
    N = pkg.newton
    ms, bms = [], []
    for form in ("device", "host"):
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        if form == "device":
            m.set_source(src)
            aq = pkg.aquifers.DeviceAquifers(recs)
        else:
            aq = pkg.aquifers.HostAquifers(recs, case["depth"], base_source=src)
        ms.append(m)
        bms.append(N.BlackoilModelHip(m, aquifer_model=aq))
    time = 0.0
    for dt in (2.0 * DAY, 10.0 * DAY, 20.0 * DAY):
        reps = []
        for bm in bms:
            bm.advance_time_level()
            bm.begin_time_step(dt, time=time)
            reps.append(bm.step(dt))
            bm.end_time_step(dt)
        assert reps[0].total_newton_iterations == reps[1].total_newton_iterations >= 2
        assert reps[0].total_linear_iterations == reps[1].total_linear_iterations
        assert same_state(ms[0], ms[1])
        a, b = bms[0].aquifers.data(ms[0]), bms[1].aquifers.data(ms[1])
        for k in ("W_flux", "pressure", "flux_rate", "init_pressure"):
            assert np.array_equal(a[k], b[k]), k
        time += dt
    assert np.all(a["W_flux"] != 0.0)


@pytest.mark.parametrize("ext", [False, True])
def test_three_time_steps_against_the_oracle(pkg, orc, ext):
    """the comparison of tests/test_gpu_timestep_hooks.py: Jacobian, residual and state bit for bit at every iteration, the oracle's
    solution applied on both sides; the oracle's model carries HostAquifers"""
    case = make_case(pkg, ext)
    recs = make_records(pkg, case)
    src = sink(case).reshape(-1)
    m = pkg.capi.HipModel(case, reorder="line_coloring")
    o = oracle_bind.OracleModel(orc, case)
    for q in (m, o):
        q.set_state(case["pv"], case["meaning"])
    m.set_source(src)
    m.set_aquifers(recs)
    h = pkg.aquifers.HostAquifers(recs, case["depth"], base_source=src)
    h.initial_solution_applied(o)
    time = 0.0
    for step, dt in enumerate([2.0 * DAY, 10.0 * DAY, 20.0 * DAY]):
        m.begin_time_step(dt)
        o.begin_time_step(dt)
        m.aquifers_begin_time_step(time, dt)
        h.begin_time_step(o, time, dt)
        for it in range(4):
            h.add_to_source(o)
            jm, rm = m.assemble(dt, it)
            jo, ro = o.assemble(dt, it)
            assert np.array_equal(jm, jo) and np.array_equal(rm, ro), (step, it)
            x, res = o.solve(tol=1e-6, maxit=200, w=0.9, mode="post_scale", reorder="none")
            m.update(x, 1.0)
            o.update(x)
            assert same_state(m, o)
        h.add_to_source(o)                 # the linearisation endTimeStep sees: the last state's
        jm, rm = m.assemble(dt, 4)
        jo, ro = o.assemble(dt, 4)
        assert np.array_equal(jm, jo) and np.array_equal(rm, ro), step
        for q in (m, o):
            q.end_time_step(dt)
        h.end_time_step(dt)
        a, b = m.get_aquifers(), h.data()
        for k in ("W_flux", "pressure", "flux_rate", "init_pressure"):
            assert np.array_equal(a[k], b[k]), (step, k)
        time += dt
    assert np.all(a["W_flux"] != 0.0)


# ---- 4. chopped step ------------------------------------------------------------------------------------------------------------------------
def test_chopped_step(pkg):
    """advance_time_level, begin (t, dt), two iterations, update_failed, begin (t, dt / 2): W_flux is unchanged, pressure_previous_ is that
    of the rolled-back state (the host form, begun on the rolled-back records, gives the same rates), and the step then matches a run
    that took dt / 2 from the start"""
    case = make_case(pkg, False)
    recs = make_records(pkg, case)
    src = sink(case).reshape(-1)

    def iterate(m, dt, n):
        for it in range(n):
            m.assemble(dt, it, fetch=False)
            assert m.solve_jacobian_system().converged
            m.update(None, 1.0)

    def fresh():
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        m.set_source(src)
        m.set_aquifers(recs)
        m.advance_time_level()              # one accepted step first, so that W_flux is not zero
        m.begin_time_step(DAY)
        m.aquifers_begin_time_step(0.0, DAY)
        iterate(m, DAY, 3)
        m.assemble(DAY, 3, fetch=False)
        m.end_time_step(DAY)
        return m

    t, dt = DAY, 20.0 * DAY
    m, ref = fresh(), fresh()
    assert same_state(m, ref)
    w0 = m.get_aquifers()
    assert np.all(w0["W_flux"] != 0.0)
    start = m.get_state()
    m.advance_time_level()
    m.begin_time_step(dt)
    m.aquifers_begin_time_step(t, dt)
    iterate(m, dt, 2)
    assert not np.array_equal(m.get_state()[0], start[0])
    m.update_failed()
    m.begin_time_step(0.5 * dt)
    m.aquifers_begin_time_step(t, 0.5 * dt)
    w1 = m.get_aquifers()
    for k in ("W_flux", "pressure", "init_pressure"):
        assert np.array_equal(w0[k], w1[k]), k              # a rolled-back step never reaches endTimeStep
    h = pkg.aquifers.HostAquifers(recs, case["depth"])
    h.initial_solution_applied(m)
    for r, w, p, p0 in zip(h.a, w1["W_flux"], w1["pressure"], w1["init_pressure"]):     # the aquifers' state as the device holds it
        r["W_flux"], r["flux_value"], r["pressure"], r["pa0"] = w, w, p, p0
    h.begin_time_step(m, t, 0.5 * dt)                       # the records of the rolled-back state
    ref.advance_time_level()
    ref.begin_time_step(0.5 * dt)
    ref.aquifers_begin_time_step(t, 0.5 * dt)
    for it in range(3):
        (ja, ra), (jb, rb) = m.assemble(0.5 * dt, it), ref.assemble(0.5 * dt, it)
        assert np.array_equal(ja, jb) and np.array_equal(ra, rb), it
        assert np.array_equal(m.aquifer_rates(), h.rates(m.iq_cells(h.cells))), it
        for q in (m, ref):
            assert q.solve_jacobian_system().converged
            q.update(None, 1.0)
        assert same_state(m, ref)
    for q in (m, ref):
        q.assemble(0.5 * dt, 3, fetch=False)
        q.end_time_step(0.5 * dt)
    wa, wb = m.get_aquifers(), ref.get_aquifers()
    for k in ("W_flux", "pressure", "flux_rate"):
        assert np.array_equal(wa[k], wb[k]), k
    assert not np.array_equal(wa["W_flux"], w0["W_flux"])


def test_chopped_step_rates_at_the_rolled_back_state(pkg):
    """after update_failed and a second begin, the first assemble's rates are those of the host form begun on the rolled-back records"""
    case = make_case(pkg, True)
    recs = make_records(pkg, case)
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_aquifers(recs)
    h = pkg.aquifers.HostAquifers(recs, case["depth"])
    h.initial_solution_applied(m)
    dt = 10.0 * DAY
    m.advance_time_level()
    m.aquifers_begin_time_step(0.0, dt)
    for it in range(2):
        m.assemble(dt, it, fetch=False)
        assert m.solve_jacobian_system().converged
        m.update(None, 1.0)
    m.update_failed()
    m.aquifers_begin_time_step(0.0, 0.5 * dt)
    h.begin_time_step(m, 0.0, 0.5 * dt)                 # the records of the rolled-back state
    assert np.array_equal(m.get_state()[0], case["pv"])
    m.assemble(0.5 * dt, 0, fetch=False)
    assert np.array_equal(m.aquifer_rates(), h.rates(m.iq_cells(h.cells)))
    m.solve_jacobian_system()
    m.update(None, 1.0)
    m.assemble(0.5 * dt, 1, fetch=False)
    assert np.array_equal(m.aquifer_rates(), h.rates(m.iq_cells(h.cells)))      # p_prev still the rolled-back state's, p_cur the iterate's


# ---- 5. water balance -------------------------------------------------------------------------------------------------------------------------
def water_in_place(m, case):
    iq = m.iq()
    return float(np.sum(case["volume"] * iq[:, -1, 0] * iq[:, 0, 0] * iq[:, 6, 0]))      # V phi S_w b_w


def test_water_balance_of_a_closed_box(pkg):
    """independent of any restatement of the aquifer classes: over five time steps the water in place changes by what the Fetkovich
    aquifer delivered (W_flux) plus the sources' water volume.  Allowed mismatch: what the Newton loop converged to - per step
    MB_w = |B_avg,w R_sum,w| dt / pvSum <= tolerance_mb, i.e. a water volume of tolerance_mb * pvSum / B_avg,w - summed over the steps"""
    case = make_case(pkg, False)
    A = pkg.aquifers
    under = A.connections(case, (0, 8, 0, 8, 1, 1), "K+")
    recs = [A.fetkovich(1, under, 2.0e6, 5.0e-8, 1.0e-9, 1.0e8, 1010.0, float(case["depth"].max()) + 2.5)]
    src = sink(case)
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src.reshape(-1))
    m.set_drift_compensation(False)
    bm = pkg.newton.BlackoilModelHip(m, aquifer_model=A.DeviceAquifers(recs))
    w0 = water_in_place(m, case)
    time, allowed, from_sources = 0.0, 0.0, 0.0
    for dt in (1.0 * DAY, 3.0 * DAY, 8.0 * DAY, 15.0 * DAY, 30.0 * DAY):
        bm.advance_time_level()
        bm.begin_time_step(dt, time=time)
        assert bm.step(dt).converged
        c = m.convergence(dt, bm.param.tolerance_cnv)
        assert c[15] <= bm.param.tolerance_mb
        allowed += bm.param.tolerance_mb * c[9] / c[7]
        bm.end_time_step(dt)
        from_sources += float(src[:, 1].sum()) * dt
        time += dt
    W = m.get_aquifers()["W_flux"][0]
    change = water_in_place(m, case) - w0
    print("water in place: change %.6f m3, W_flux %.6f, sources %.6f, mismatch %.3e, allowed %.3e" % (change, W, from_sources, change - (W + from_sources), allowed))
    assert W > 100.0 * allowed                       # the influx is what the balance is about
    assert abs(change - (W + from_sources)) <= allowed


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    C = pkg.capi
    case = make_case(pkg, False)
    good = make_records(pkg, case, initial_pressure=250e5)

    def refused(model, recs, code, word, edit=None):
        aq, keep = C.make_aquifers(recs)
        if edit:
            edit(aq, keep)
        rc = C.lib().opmhip_set_aquifers(model._h, aq)
        msg = C.lib().opmhip_last_error(model._h).decode()
        assert rc == code and word in msg, (rc, msg)

    f = C.HipFluid(case["fluid"])
    refused(f, good, C.NOT_READY, "set_static")
    m = C.HipModel(case)
    refused(m, good, C.NOT_READY, "set_state")
    m.set_state(case["pv"], case["meaning"])
    m.set_aquifers(good)
    assert m.get_aquifers()["init_pressure"][0] == 250e5
    change = lambda i, **kw: [dict(r, **kw) if k == i else r for k, r in enumerate(good)]
    null = lambda name: (lambda aq, keep: setattr(aq, name, None))
    def poke(name, i, v):
        def e(aq, keep):
            keep[name][i] = v
        return e
    cases = [(good, "null array", null("cell")), (good, "null array", null("alpha")), (good, "null array", null("time_constant")),
             (good, "null array", null("td")), (good, "null array", null("prod_index")), (good, "null array", null("initial_pressure")),
             (good, "conn_pointers", poke("conn_pointers", 1, 30)), (good, "conn_pointers", poke("conn_pointers", 0, 1)),
             (good, "type", poke("type", 2, 5)), ([good[2], good[0]], "Carter-Tracy first", None),
             (good, "outside", poke("cell", 3, 162)), (good, "outside", poke("cell", 20, -1)), (good, "repeated", poke("cell", 25, case["Nb"] - 1)),
             (change(0, time_constant=0.0), "time constant", None), (change(2, time_constant=-1.0), "time constant", None),
             (change(0, td=[0.1, 0.1, 1.0, 2.0]), "not ascending", None), (change(1, td=[0.1], pd=[0.2]), "fewer than two nodes", None),
             (change(2, total_compr=0.0), "total_compr * initial_watvolume", None), (change(2, initial_watvolume=-1.0), "total_compr * initial_watvolume", None),
             (change(0, restart=dict(W_flux=1.0)), "restart", None)]
    for recs, word, edit in cases:
        m.set_aquifers(good)
        refused(m, recs, C.INVALID_ARGUMENT, word, edit)
        # after a refused call no list is set: an assemble needs no aquifer time step and gives the no-aquifer result
        m._naq = m._naqconn = 0
        j, r = m.assemble(DAY, 0)
    plain = C.HipModel(case)
    plain.set_state(case["pv"], case["meaning"])
    jp, rp = plain.assemble(DAY, 0)
    assert np.array_equal(j, jp) and np.array_equal(r, rp)
    # Fetkovich restart data is taken
    m.set_aquifers(change(2, restart=dict(W_flux=12.5, pressure=249e5)))
    d = m.get_aquifers()
    assert d["W_flux"][2] == 12.5 and d["pressure"][2] == 249e5 and d["init_pressure"][2] == 250e5 and d["W_flux"][0] == 0.0
    with pytest.raises(C.OpmHipError):
        m.aquifers_begin_time_step(0.0, 0.0)
    # a decomposed context (loopback, two ranks): out of scope
    sub = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    dd = C.HipModel(sub, comm=("loopback", 2, 0, "aq" + uuid.uuid4().hex), reorder="level_scheduling")
    dd.set_state(sub["pv"], sub["meaning"])
    one = pkg.aquifers.fetkovich(1, dict(cells=[0, 1], alpha=[0.5, 0.5]), 1e6, 1e-8, 1e-9, 1e10, 1000.0, 2500.0, initial_pressure=250e5)
    refused(dd, [one], C.INVALID_ARGUMENT, "decomposed")

"""Passive tracers on the device (opmhip_set_tracers ... opmhip_tracers_end_time_step) against tracers.HostTracers, the plain-numpy
restatement of ebos/ecltracermodel.hh: the system bit for bit, the storage cache, the batched ILU0-BiCGStab in every ordering of the
context with its freeze logic, the time-step loop with host and device wells, the refusals, and that a context without tracers does
what it did."""
import uuid

import numpy as np
import pytest

import tracer_states as S

pytestmark = pytest.mark.gpu
DAY, DT = S.DAY, S.DT


def model_at(pkg, case, pv, **kw):
    m = pkg.capi.HipModel(case, **kw)
    m.set_state(pv, case["meaning"])
    return m


def host_and_device(pkg, case, pv1, phase, c, conn=None, model_kw=None, **solver):
    """a context and the host form, begun at the case's own state and standing at pv1, fed the same records"""
    T = pkg.tracers
    m = model_at(pkg, case, case["pv"], **(model_kw or {}))
    d = T.DeviceTracers(m, phase, c, **solver)
    h = T.HostTracers(case, phase, c, **{k: v for k, v in solver.items() if v is not None})
    d.begin_time_step()
    h.begin_time_step(m.iq())
    m.set_state(pv1, case["meaning"])
    h.set_records(m.iq())
    if conn is not None:
        d.set_connections(*conn)
        h.set_connections(*conn)
    return m, d, h


# ---- 1. the system, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("wells", [False, True], ids=["no-connections", "connections"])
def test_system_bit_for_bit(pkg, ext, wells):
    """9 x 9 x 2 = 162 rows (more than two waves, no multiple of 64), heterogeneous, `mixed`, gravity, one THPRES-blocked face; a water batch
    of three and an oil batch of one; with connections one cell is named twice"""
    T = pkg.tracers
    case, pv1 = S.system_case(pkg, (9, 9, 2), ext=ext)
    phase, c = S.system_tracers(case)
    conn = S.system_connections(case, len(phase)) if wells else None
    m, d, h = host_and_device(pkg, case, pv1, phase, c, conn)
    assert m.iq().shape[1] == (19 if ext else 17)
    differ = 0
    for ph in (S.WATER, S.OIL):
        Md, rd = d.system(ph, DT)
        Mh, rh = h.system(ph, DT)
        assert np.array_equal(Md, Mh), (ph, np.abs(Md - Mh).max())
        assert np.array_equal(rd, rh), (ph, np.abs(rd - rh).max())
        assert rd.shape == (3 if ph == S.WATER else 1, case["Nb"])
        # the case exercises what it is for
        f, up = T.face_values(case, h.iq, ph)
        off = np.repeat(np.arange(case["Nb"]), np.diff(case["rowptr"])) != case["col"]
        if ph == S.OIL:
            assert (up & off & (f != 0)).sum() > 20 and (~up & off & (f != 0)).sum() > 20      # both upwind directions occur
        a = (9 // 2) + 9 * (9 // 2)
        assert f[S.entry(case, a, a + 1)] == 0.0 and f[S.entry(case, a + 1, a)] == 0.0           # the blocked face carries nothing
        differ += int(((f + f[h._tr]) != 0.0).sum())
    print("faces whose two-sided evaluations are not bitwise antisymmetric: %d" % differ)
    assert differ > 0, "no face of this case tells the two evaluations apart"
    # nothing was solved and nothing changed
    assert np.array_equal(m.get_tracers(), c)


@pytest.mark.parametrize("dims", [(1, 1, 1), (70, 1, 1)], ids=["1x1x1", "70x1x1"])
def test_system_on_edge_grids(pkg, dims):
    """a row without faces; a row of cells that crosses a wave boundary, every row with at most two neighbours"""
    case, pv1 = S.system_case(pkg, dims)
    phase, c = S.system_tracers(case)
    conn = S.system_connections(case, len(phase))
    m, d, h = host_and_device(pkg, case, pv1, phase, c, conn)
    for ph in (S.WATER, S.OIL):
        Md, rd = d.system(ph, DT)
        Mh, rh = h.system(ph, DT)
        assert np.array_equal(Md, Mh) and np.array_equal(rd, rh)
    res = d.end_time_step(DT)
    res_h = h.end_time_step(DT, order=m.ordering()[:2])
    assert all(r["converged"] for r in res) and [r["iterations"] for r in res] == [r["iterations"] for r in res_h]
    assert update_error(c, d.c, h.last_dx) <= 10 * S.DX_MARGIN


# ---- 2. begin / end bookkeeping -------------------------------------------------------------------------------------------------------------
def test_begin_bookkeeping(pkg):
    case, pv1 = S.system_case(pkg, (9, 9, 2))
    phase, c = S.system_tracers(case)
    m, d, h = host_and_device(pkg, case, pv1, phase, c)
    m.set_state(case["pv"], case["meaning"])
    s1, c0 = m.tracer_storage()
    assert np.array_equal(s1, h.storage1) and np.array_equal(c0, h.c_initial) and np.array_equal(c0, c)
    # a chopped step: the state moves, the step is given up, begin again from the rolled-back state
    m.set_state(pv1, case["meaning"])
    m.set_state(case["pv"], case["meaning"])
    d.begin_time_step()
    s2, c2 = m.tracer_storage()
    assert np.array_equal(s2, s1) and np.array_equal(c2, c0)
    # begin at another state gives other storage, the same c_initial
    m.set_state(pv1, case["meaning"])
    d.begin_time_step()
    h.begin_time_step(m.iq())
    s3, c3 = m.tracer_storage()
    assert np.array_equal(s3, h.storage1) and not np.array_equal(s3, s1) and np.array_equal(c3, c0)


def update_error(c_before, c_after, dx_ref):
    """how far the device's update is from dx_ref, relative to the largest |dx_ref| of the tracer.  The device's dx itself does not come
    back: c_after = c_before - dx does, rounded once - so up to one spacing of the largest concentration is the subtraction's, not the
    solve's, and is taken off before the comparison"""
    out = 0.0
    for cb, ca, dx in zip(c_before, c_after, dx_ref):
        s = np.abs(dx).max()
        if s == 0.0:
            assert np.array_equal(cb, ca)
            continue
        err = np.abs(ca - (cb - dx)).max() - np.spacing(np.abs(cb).max())
        out = max(out, max(float(err), 0.0) / s)
    return out


# ---- 3. the solve ---------------------------------------------------------------------------------------------------------------------------
ORDERINGS = [("level_scheduling", (9, 9, 2), {}), ("graph_coloring_greedy", (9, 9, 2), {}), ("line_coloring", (12, 12, 12), dict(chain_length=4))]


def solve_pair(pkg, reorder, dims, kw, **solver):
    sc = S.solve_case(pkg, dims)
    m, d, h = host_and_device(pkg, sc["case"], sc["pv1"], sc["phase"], sc["c"], (sc["cells"], sc["rates"], sc["injected"]),
                              model_kw=dict(reorder=reorder, **kw), **solver)
    info = m.ordering_info()
    if reorder == "line_coloring" and not (info["ilu_ordering"] == "line_coloring" and info["chain_length"] == 4):
        pytest.skip("the pattern did not take the chained order: %r" % (info,))
    return sc, m, d, h


@pytest.mark.parametrize("reorder,dims,kw", ORDERINGS, ids=[o[0] for o in ORDERINGS])
def test_solve_in_every_ordering(pkg, reorder, dims, kw):
    """tolerance 1e-2: the same number of half iterations per tracer as the host form in that ordering, dx within 10 x the margin measured
    between two summation orders on the CPU (tracer_states.DX_MARGIN); the batch's right-hand sides are very different - the zero tracer
    takes no iteration and keeps its concentrations, the other two stop at different half iterations: the freeze logic"""
    sc, m, d, h = solve_pair(pkg, reorder, dims, kw)
    c_before = d.c
    res_h = h.end_time_step(DT, order=m.ordering()[:2])
    assert S.clear_decisions(res_h, 1e-2)                  # the equal-iterations check below is not hostage to a rounding
    res_d = d.end_time_step(DT)
    its_h, its_d = [r["iterations"] for r in res_h], [r["iterations"] for r in res_d]
    print("%s %r: iterations host %r device %r, reductions %r" % (reorder, dims, its_h, its_d, [r["reduction"] for r in res_d]))
    assert its_d == its_h
    assert all(r["converged"] for r in res_d) and all(r["converged"] for r in res_h)
    assert its_d[2] == 0.0 and 0.0 < its_d[0] != its_d[1] > 0.0
    diff = update_error(c_before, d.c, h.last_dx)
    print("  rel. difference of dx %.3e (margin %.3e)" % (diff, 10 * S.DX_MARGIN))
    assert np.array_equal(d.c[2], c_before[2]) and np.all(d.c[2] == 0.0)
    assert diff <= 10 * S.DX_MARGIN
    # the same input gives the same bits from call to call
    sc2, m2, d2, h2 = solve_pair(pkg, reorder, dims, kw)
    d2.end_time_step(DT)
    assert np.array_equal(d2.c, d.c)


def test_solve_to_a_tight_tolerance_equals_the_dense_solve(pkg):
    sc, m, d, h = solve_pair(pkg, "graph_coloring_greedy", (9, 9, 2), {}, tolerance=1e-12, maxit=100)
    case = sc["case"]
    M, r = d.system(S.OIL, DT)
    A = S.dense(case, M)
    kappa = np.linalg.cond(A)
    c_before = d.c
    res = d.end_time_step(DT)
    assert all(q["converged"] for q in res), res
    ref = np.linalg.solve(A, r.T).T
    err = update_error(c_before, d.c, ref)
    print("tolerance 1e-12: iterations %r, cond %.3e, rel. error against the dense solve %.3e" % ([q["iterations"] for q in res], kappa, err))
    assert err <= kappa * 1e-12


def test_maxit_one_is_applied_and_reported(pkg):
    sc, m, d, h = solve_pair(pkg, "graph_coloring_greedy", (9, 9, 2), {}, tolerance=1e-10, maxit=1)
    c_before = d.c
    res_h = h.end_time_step(DT, order=m.ordering()[:2])
    res = d.end_time_step(DT)
    assert [q["converged"] for q in res] == [q["converged"] for q in res_h]
    assert not res[1]["converged"] and res[1]["iterations"] == 1.0 and res[2]["converged"]
    assert np.abs(c_before[1] - d.c[1]).max() > 0.0         # the unconverged dx was applied all the same
    assert update_error(c_before, d.c, h.last_dx) <= 10 * S.DX_MARGIN


# ---- 4. through the time-step loop -------------------------------------------------------------------------------------------------------------
class Both:
    """the device's and the host's tracer model behind one set of hooks: the same records and rates at every step"""

    def __init__(self, T, dev, host):
        self.T, self.dev, self.host = T, dev, host
        self.log = []
        self.allowed = 0.0

    def on_begin_time_step(self, model):
        self.dev.on_begin_time_step(model)
        self.host.on_begin_time_step(model)
        self.inplace0 = self.inplace(model)

    def inplace(self, model):
        vol = model.case["volume"] * self.T.phase_volume(model.iq(), S.WATER)
        return float((vol * self.dev.c[0]).sum())

    def on_end_time_step(self, model, dt, connections=None):
        cells, rates = connections
        self.host.set_records(model.iq())
        self.host.set_connections(cells, rates, self.host.injected)
        M, r = self.host.system(S.WATER, dt)
        rd = self.dev.on_end_time_step(model, dt, connections)
        rh = self.host.on_end_time_step(model, dt, connections)
        q = rates[:, S.WATER]
        c = self.dev.c[0]
        injected = float((q[q > 0] * self.host.injected[0][q > 0]).sum()) * dt
        produced = float((-q[q < 0] * c[cells[q < 0]]).sum()) * dt
        # the margin of the solve, compounded: this step's solve may differ by 10 x DX_MARGIN of its largest dx; the difference carried in
        # from the step before enters through storage1 = vol_old c and leaves as M^-1 (vol_old V / dt) e - M is column-dominant with
        # vol_new V / dt on its diagonal, so that map has 1-norm max vol_old / vol_new, within a per cent of 1 over these steps - and the
        # subtraction c - dx rounds once on either side
        self.allowed = 1.01 * self.allowed + 10 * S.DX_MARGIN * float(np.abs(self.host.last_dx).max()) + float(np.spacing(np.abs(self.host.c).max()))
        self.log.append(dict(rd=rd, rh=rh, injected=injected, produced=produced, d_inplace=self.inplace(model) - self.inplace0,
                             bound=np.sqrt(len(c)) * 1e-2 * float(np.linalg.norm(r[0])) * dt, diff=float(np.abs(self.host.c - self.dev.c).max()),
                             allowed=self.allowed))



def loop_wells(pkg, case):
    W = pkg.wells
    def well(name, cells, producer, control, limit, inj=None):
        tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return W.Well(name, cells, tw, case["depth"][cells[0]], producer, control, limit, inj_phase=inj)
    nx, ny, nz = case["nx"], case["ny"], case["nz"]
    col = lambda i, j: [i + nx * (j + ny * k) for k in range(nz)]
    return [well("I", col(0, 0), False, ("rate", W.WATER, 20.0 / DAY), 600e5, "water"), well("P", col(nx - 1, ny - 1), True, ("rate", W.OIL, 15.0 / DAY), 50e5)]


@pytest.mark.parametrize("wells,steps", [("host", 3), ("device", 1)], ids=["host-wells", "device-wells"])
def test_through_the_time_step_loop(pkg, wells, steps):
    """6 x 6 x 3, an injector whose water carries tracer concentration 1 and a producer.  Per step the device and the host form differ by
    the solve's margin (10 x DX_MARGIN of the step's largest dx) and inherit the difference of the concentrations they started from,
    carried through an update that is linear in c (Both.on_end_time_step states the sum).  In place + produced = injected up to the linear
    residual: summing the equations at the new concentrations the fluxes cancel and what is left is sum(rho) dt, |sum(rho)| <=
    sqrt(N) ||rho|| <= sqrt(N) tol ||r_0||."""
    T = pkg.tracers
    case = pkg.decks.cartesian_case(6, 6, 3, state="mixed", heterogeneous=True)
    m = model_at(pkg, case, case["pv"], tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
    wl = loop_wells(pkg, case)
    w = pkg.wells.DeviceStandardWells(wl, case["depth"], m) if wells == "device" else pkg.wells.StandardWells(wl, case["depth"], arithmetic="stated")
    c0 = np.zeros((1, case["Nb"]))
    both = Both(T, T.DeviceTracers(m, [S.WATER], c0), T.HostTracers(case, [S.WATER], c0))
    inj = np.zeros((1, len(w.cells)))
    inj[0, :3] = 1.0                                            # WTRACER on the injector's three connections
    both.dev.set_injected(inj)
    both.host.set_injected(inj)
    ts = pkg.newton.AdaptiveTimeStepping(pkg.newton.BlackoilModelHip(m, well_model=w, tracer_model=both), pkg.newton.TimeSteppingParameters(initial_dt=DAY))
    for _ in range(steps):
        ts.advance_report_step(DAY)
    assert len(both.log) >= steps
    for n, e in enumerate(both.log):
        print("step %d: device %r host %r injected %.6e produced %.6e in place %+.6e bound %.3e diff %.3e (allowed %.3e)"
              % (n, e["rd"], e["rh"], e["injected"], e["produced"], e["d_inplace"], e["bound"], e["diff"], e["allowed"]))
        assert [q["iterations"] for q in e["rd"]] == [q["iterations"] for q in e["rh"]] and e["rd"][0]["converged"]
        assert e["diff"] <= e["allowed"], (e["diff"], e["allowed"])
        assert e["injected"] > 0.0
        assert abs(e["d_inplace"] + e["produced"] - e["injected"]) <= e["bound"] + 1e-12 * e["injected"]
    assert both.dev.c.max() > 0.0


# ---- 5. refusals and neutrality ----------------------------------------------------------------------------------------------------------------
def refused(call, code, word):
    with pytest.raises(Exception) as e:
        call()
    assert getattr(e.value, "code", None) == code and word in str(e.value), (e.value, code, word)


def test_refusals(pkg):
    import helpers
    C = pkg.capi
    case = pkg.decks.cartesian_case(4, 3, 2, state="mixed", heterogeneous=True)
    Nb = case["Nb"]
    m = model_at(pkg, case, case["pv"])
    ones = np.ones((1, Nb))
    refused(lambda: m.set_tracers([2], ones), C.INVALID_ARGUMENT, "gas tracer")
    refused(lambda: m.set_tracers([3], ones), C.INVALID_ARGUMENT, "phase")
    bad = ones.copy()
    bad[0, 5] = np.nan
    refused(lambda: m.set_tracers([0], bad), C.INVALID_ARGUMENT, "not finite")
    with pytest.raises(ValueError):
        m.set_tracers([0, 1], ones)                                # ragged
    refused(lambda: m.set_tracer_connections([0], [[0.0, 0.0, 0.0]], np.zeros((0, 1))), C.NOT_READY, "before set_tracers")
    # a refused call leaves no tracers set: end_time_step is a no-op
    assert m.tracers_end_time_step(DT) == []
    m.set_tracers([0, 1], np.ones((2, Nb)))
    refused(lambda: m.tracers_end_time_step(DT), C.NOT_READY, "begin_time_step")
    refused(lambda: m.tracer_system(0, DT, 1), C.NOT_READY, "begin_time_step")
    m.tracers_begin_time_step()
    refused(lambda: m.tracers_end_time_step(0.0), C.INVALID_ARGUMENT, "dt")
    refused(lambda: m.set_tracer_connections([Nb], [[0.0, 0.0, 0.0]], [[1.0], [1.0]]), C.INVALID_ARGUMENT, "outside")
    refused(lambda: m.set_tracer_connections([0], [[0.0, np.inf, 0.0]], [[1.0], [1.0]]), C.INVALID_ARGUMENT, "not finite")
    with pytest.raises(ValueError):
        m.set_tracer_connections([0, 1], [[0.0, 0.0, 0.0]], [[1.0], [1.0]])
    refused(lambda: m.set_tracer_solver(0.0, 100), C.INVALID_ARGUMENT, "tolerance")
    refused(lambda: m.set_tracer_solver(1e-2, 0), C.INVALID_ARGUMENT, "maxit")
    # a state is needed
    fresh = C.HipModel(case)
    fresh.set_tracers([0], ones)
    refused(fresh.tracers_begin_time_step, C.NOT_READY, "set_state")
    # an oil tracer on a fluid with PVTG; a water tracer is taken
    wet = helpers.wetgas_case(pkg, 4, 3, 4)
    mw = model_at(pkg, wet, wet["pv"])
    refused(lambda: mw.set_tracers([1], np.ones((1, wet["Nb"]))), C.INVALID_ARGUMENT, "PVTG")
    mw.set_tracers([0], np.ones((1, wet["Nb"])))
    # a decomposed context (loopback, two ranks)
    sub = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    dd = C.HipModel(sub, comm=("loopback", 2, 0, "tr" + uuid.uuid4().hex), reorder="level_scheduling")
    dd.set_state(sub["pv"], sub["meaning"])
    refused(lambda: dd.set_tracers([0], np.ones((1, sub["Nb"]))), C.INVALID_ARGUMENT, "decomposed")


def test_a_context_without_tracers_does_what_it_did(pkg):
    """a Newton step's Jacobian and residual of a context whose tracers were set and cleared equal those of one that never heard of
    tracers, and the profile shows the same launches"""
    case = pkg.decks.cartesian_case(5, 4, 3, state="mixed", heterogeneous=True)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=50.0)
    out = []
    for touched in (False, True):
        m = model_at(pkg, case, case["pv"])
        if touched:
            m.set_tracers([0, 1], np.ones((2, case["Nb"])))
            m.set_tracers([], None)
        m.set_source(src)
        m.profile_enable(True)
        if touched:
            m.tracers_begin_time_step()
            assert m.tracers_end_time_step(DAY) == []
        j, r = m.assemble(DAY, 0)
        res = m.solve_jacobian_system()
        m.update(None, 1.0)
        j2, r2 = m.assemble(DAY, 1)
        out.append((j, r, j2, r2, res.iterations, m.profile(), m.get_state()))
    a, b = out
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert a[4] == b[4] and np.array_equal(a[6][0], b[6][0])
    pa, pb = {k: v[0] for k, v in a[5].items()}, {k: v[0] for k, v in b[5].items()}
    print("launches per profile class without / with cleared tracers:", pa, pb)
    assert pa == pb and sum(pa.values()) > 0

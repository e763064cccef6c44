"""The tracer kernels (csrc/tracers.hip) where tests/test_gpu_tracers.py does not take them: batches wider than one chunk of TR_CH = 8
tracers up to the cap of 32, scalar products over two and three reduction workgroups with a ragged last one, cells without mobile water
(the phase-volume clamp, faces with one or no mobile side), a pivot that is not finite, connection lists beyond one wave and their
replacement by shorter and empty ones, the extended record, and opmhip_set_tracers called again on a live context.  The comparator is
tracers.HostTracers in the context's ordering: systems bit for bit, solves with the same half iterations per tracer and dx within
10 x tracer_states.DX_MARGIN (tools/tracer_margin.py walks the same cases).  tests/test_tracers.py proves on the CPU that each case has
the property it is here for."""
import numpy as np
import pytest

import tracer_states as S
from test_gpu_tracers import host_and_device, model_at, update_error

pytestmark = pytest.mark.gpu
DT = S.DT
WATER, OIL = S.WATER, S.OIL
REORDERS = ["level_scheduling", "graph_coloring_greedy"]


def conn_of(sc):
    return sc["cells"], sc["rates"], sc["injected"]


def pair_of(pkg, sc, reorder=None, **solver):
    return host_and_device(pkg, sc["case"], sc["pv1"], sc["phase"], sc["c"], conn_of(sc), model_kw=dict(reorder=reorder) if reorder else None, **solver)


def systems_equal(d, h, case, phase):
    """M and the residual of both phases, bit for bit -> {phase: (M, residual)} of the device"""
    out = {}
    for ph in (WATER, OIL):
        Md, rd = d.system(ph, DT)
        Mh, rh = h.system(ph, DT)
        assert np.array_equal(Md, Mh), (ph, np.abs(Md - Mh).max())
        assert np.array_equal(rd, rh), (ph, np.abs(rd - rh).max())
        assert rd.shape == (list(phase).count(ph), case["Nb"])
        out[ph] = (Md, rd)
    return out


def solves_equal(m, d, h, tol=1e-2):
    """one step on both: every decision of the host form clear, the same half iterations per tracer, everything converged, dx within
    10 x the margin -> (host results, device results, concentrations before)"""
    c_before = d.c
    res_h = h.end_time_step(DT, order=m.ordering()[:2])
    assert S.clear_decisions(res_h, tol)
    res_d = d.end_time_step(DT)
    its_h, its_d = [r["iterations"] for r in res_h], [r["iterations"] for r in res_d]
    print("iterations host %r device %r" % (its_h, its_d))
    assert its_d == its_h
    assert all(r["converged"] for r in res_d) and all(r["converged"] for r in res_h)
    diff = update_error(c_before, d.c, h.last_dx)
    print("rel. difference of dx %.3e (margin %.3e)" % (diff, 10 * S.DX_MARGIN))
    assert diff <= 10 * S.DX_MARGIN
    return res_h, res_d, c_before


# ---- 1. batch widths through the chunked kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [WATER, OIL], ids=["wide-water-then-oil-1", "water-1-then-wide-oil"])
@pytest.mark.parametrize("nt", S.WIDTHS)
def test_wide_batches_bit_for_bit_and_solved(pkg, nt, wide):
    """9 x 9 x 2 of the system comparison; a batch of nt in one phase and of one in the other, interleaved in the caller's list.  The system
    of both phases bit for bit - the residual rows all differ, so a row of a later chunk that took an earlier chunk's values shows -, then
    the step: the Krylov vectors, d_y, the scalars and the partial sums serve the water batch and then the oil batch at another stride"""
    sc = S.wide_solve_case(pkg, nt, wide)
    case, phase, c = sc["case"], sc["phase"], sc["c"]
    m, d, h = pair_of(pkg, sc)
    for ph, (M, r) in systems_equal(d, h, case, phase).items():
        assert r.shape[0] == (nt if ph == wide else 1)
        assert len({row.tobytes() for row in r}) == len(r)        # no two tracers' rows alike: chunks can be told apart
        assert np.isfinite(M).all() and np.isfinite(r).all()
    assert np.array_equal(m.get_tracers(), c)
    solves_equal(m, d, h)


def run_protos(pkg, proto, reorder):
    sc = S.proto_solve_case(pkg, (9, 9, 2), proto)
    m, d, h = pair_of(pkg, sc, reorder)
    res_h, res_d, c_before = solves_equal(m, d, h)
    return [r["iterations"] for r in res_d], c_before, d.c


@pytest.mark.parametrize("reorder", REORDERS)
def test_seventeen_copies_of_three_prototypes(pkg, reorder):
    """17 oil tracers, copies of solve_case's injector-only, uniform and zero tracer spread over the chunks [0, 8), [8, 16), [16, 17).  A
    tracer's sums do not depend on its slot (k_tracer_dot gives tracer t the lanes tid % nt == t and walks with a stride that is a
    multiple of nt), so the copies of a prototype end bitwise alike, and so does every tracer when the slots are permuted"""
    proto = np.array(S.PROTO_17)
    its, c_before, c = run_protos(pkg, proto, reorder)
    stops = [set(np.array(its)[proto == p]) for p in (0, 1, 2)]
    assert all(len(s) == 1 for s in stops) and len(set.union(*stops)) == 3 and stops[2] == {0.0}, its     # the freeze logic across the chunks
    for p in (0, 1, 2):
        slots = np.flatnonzero(proto == p)
        for s in slots[1:]:
            assert np.array_equal(c[s], c[slots[0]]), (p, s)
    assert np.array_equal(c[16], c_before[16]) and np.all(c[16] == 0.0)
    assert np.abs(c[0] - c_before[0]).max() > 0.0 and np.abs(c[1] - c_before[1]).max() > 0.0
    perm = np.array(S.PERM_17)
    its2, _, c2 = run_protos(pkg, proto[perm], reorder)
    assert its2 == [its[s] for s in perm]
    for s in range(17):
        assert np.array_equal(c2[s], c[perm[s]]), s


# ---- 2. reductions over more than one workgroup -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [3, 9])
@pytest.mark.parametrize("reorder", REORDERS)
@pytest.mark.parametrize("dims", S.REDUCTION_GRIDS, ids=["17x17x1", "23x23x1"])
def test_reductions_over_several_workgroups(pkg, dims, reorder, nt):
    """289 cells: two workgroups of 145 and 144 cells; 529: three of 177, 177, 175 (tests/test_tracers.py restates the arithmetic).  nt = 9
    leaves four of the 256 lanes idle"""
    sc = S.solve_case(pkg, dims) if nt == 3 else S.proto_solve_case(pkg, dims, S.PROTO_9)
    assert len(sc["phase"]) == nt
    m, d, h = pair_of(pkg, sc, reorder)
    assert m.ordering_info()["ilu_ordering"] == reorder
    res_h, res_d, c_before = solves_equal(m, d, h)
    proto = np.array(sc.get("proto", (0, 1, 2)))
    for s in np.flatnonzero(proto == 2):
        assert res_d[s]["iterations"] == 0.0 and np.array_equal(d.c[s], c_before[s])
    for p in (0, 1):
        slots = np.flatnonzero(proto == p)
        assert res_d[slots[0]]["iterations"] > 0.0
        for s in slots[1:]:
            assert np.array_equal(d.c[s], d.c[slots[0]]), (p, s)


TIGHT = [((9, 9, 2), S.PROTO_17), ((23, 23, 1), S.PROTO_9)]


@pytest.mark.parametrize("dims,proto", TIGHT, ids=["17-tracers-three-chunks", "9-tracers-three-workgroups"])
def test_tight_tolerance_equals_the_dense_solve(pkg, dims, proto):
    """at tolerance 1e-2 no solve of these cases goes past its first iteration.  At 1e-12 the uniform tracers do - the p update and beta,
    with the other tracers of the batch frozen long before - and the result is held to the dense solve as test_gpu_tracers holds its
    three-tracer case: within cond(M) x the tolerance"""
    sc = S.proto_solve_case(pkg, dims, proto)
    m, d, h = pair_of(pkg, sc, "graph_coloring_greedy", tolerance=1e-12, maxit=100)
    M, r = d.system(OIL, DT)
    A = S.dense(sc["case"], M)
    kappa = np.linalg.cond(A)
    c_before = d.c
    res = d.end_time_step(DT)
    its = [q["iterations"] for q in res]
    assert all(q["converged"] for q in res), res
    assert max(its) >= 1.5, its                                   # a second iteration was begun: k_tracer_pupdate ran
    err = update_error(c_before, d.c, np.linalg.solve(A, r.T).T)
    print("tolerance 1e-12: iterations %r, cond %.3e, rel. error against the dense solve %.3e" % (its, kappa, err))
    assert err <= kappa * 1e-12
    p = np.array(proto)
    for q in (0, 1, 2):
        slots = np.flatnonzero(p == q)
        for s in slots[1:]:
            assert its[s] == its[slots[0]] and np.array_equal(d.c[s], d.c[slots[0]]), (q, s)


# ---- 3. cells without mobile water -----------------------------------------------------------------------------------------------------------
def test_cells_without_mobile_water(pkg):
    sc = S.dry_case(pkg)
    case, dry = sc["case"], sc["dry"]
    m, d, h = pair_of(pkg, sc)
    iq = m.iq()
    assert np.all(iq[dry, pkg.tracers.F_MOB + WATER, 0] == 0.0) and np.all(pkg.tracers.phase_volume(iq, WATER)[dry] == 1e-10)
    s1, c0 = m.tracer_storage()
    assert np.array_equal(s1, h.storage1) and np.array_equal(c0, h.c_initial)
    assert np.all(s1[0, dry] == 1e-10 * sc["c"][0, dry])
    systems_equal(d, h, case, sc["phase"])
    solves_equal(m, d, h)


# ---- 4. the pivot flag -------------------------------------------------------------------------------------------------------------------------
def last_error(pkg, m):
    return pkg.capi.lib().opmhip_last_error(m._h).decode()


def test_a_pivot_that_is_not_finite_is_reported_and_does_not_leak(pkg):
    """two producing oil connections of -1e308 in one cell: that row's diagonal is +inf, the ILU0 replaces the pivot by 1 and raises the flag;
    the call succeeds, both oil tracers are reported as not converged and the text names the phase.  The water batch of the same context is
    solved as ever, in this step (before the oil batch) and in the next (after the flag was raised: k_tracer_copy resets it)"""
    sc = S.pivot_case(pkg)
    m, d, h = pair_of(pkg, sc, maxit=2)
    c_before = d.c
    with np.errstate(all="ignore"):
        res_h = h.end_time_step(DT, order=m.ordering()[:2])
    assert S.clear_decisions([res_h[1]], 1e-2)
    res_d = d.end_time_step(DT)                                # returns: OPMHIP_SUCCESS
    text = last_error(pkg, m)
    print("step 1: host %r\n        device %r\n        last error %r" % ([(r["converged"], r["iterations"]) for r in res_h], res_d, text))
    assert [bool(r["converged"]) for r in res_d] == [False, True, False] == [bool(r["converged"]) for r in res_h]
    assert [r["iterations"] for r in res_d] == [r["iterations"] for r in res_h]
    assert "phase 1" in text and "pivot" in text
    assert np.isfinite(d.c[1]).all()
    assert update_error(c_before[1:2], d.c[1:2], h.last_dx[1:2]) <= 10 * S.DX_MARGIN
    # the next step, a sane list in place of the first: every tracer whose concentrations are still finite converges.  The host form goes
    # on from the device's concentrations, so that this step's comparison is this step's alone
    c1 = d.c
    finite = np.isfinite(c1).all(axis=1)
    print("tracers still finite after the first step: %r" % (finite.tolist(),))
    assert finite[1]
    h.c = c1.copy()
    d.begin_time_step()
    h.begin_time_step()
    d.set_connections(*sc["sane"])
    h.set_connections(*sc["sane"])
    with np.errstate(all="ignore"):
        res_h = h.end_time_step(DT, order=m.ordering()[:2])
    res_d = d.end_time_step(DT)
    keep = np.flatnonzero(finite)
    assert S.clear_decisions([res_h[t] for t in keep], 1e-2)
    for t in keep:
        assert res_d[t]["converged"] and res_h[t]["converged"] and res_d[t]["iterations"] == res_h[t]["iterations"], (t, res_d[t], res_h[t])
    assert update_error(c1[keep], d.c[keep], h.last_dx[keep]) <= 10 * S.DX_MARGIN
    for t in np.flatnonzero(~finite):
        assert not res_d[t]["converged"]


# ---- 5. connections across a wave boundary -----------------------------------------------------------------------------------------------------
def test_connection_lists_beyond_one_wave_and_their_replacement(pkg):
    """71 distinct connected cells (k_tracer_wells takes a second workgroup), one of them named five times; then the four connections of the
    system comparison in their place, then none: nothing of a longer list survives"""
    T = pkg.tracers
    case, pv1 = S.system_case(pkg, (9, 9, 2))
    phase, c = S.wide_tracers(case, 9, WATER)
    cells, rates, inj, many = S.wave_connections(case, len(phase))
    m, d, h = host_and_device(pkg, case, pv1, phase, c, (cells, rates, inj))
    long_ = systems_equal(d, h, case, phase)
    short = S.system_connections(case, len(phase))
    d.set_connections(*short)
    h.set_connections(*short)
    short_ = systems_equal(d, h, case, phase)
    for ph in (WATER, OIL):
        assert not np.array_equal(long_[ph][1][:, many], short_[ph][1][:, many]) and not np.array_equal(long_[ph][0], short_[ph][0])
    d.set_connections(np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((len(phase), 0)))
    bare = T.HostTracers(case, phase, c)
    bare.storage1, bare.c_initial = h.storage1, h.c_initial     # the same begin of the step
    bare.set_records(m.iq())
    none_ = systems_equal(d, bare, case, phase)
    for ph in (WATER, OIL):
        assert not np.array_equal(none_[ph][1], short_[ph][1]) and not np.array_equal(none_[ph][0], short_[ph][0])
    # and back to the long list on the same context
    d.set_connections(cells, rates, inj)
    h.set_connections(cells, rates, inj)
    again = systems_equal(d, h, case, phase)
    for ph in (WATER, OIL):
        assert np.array_equal(again[ph][0], long_[ph][0]) and np.array_equal(again[ph][1], long_[ph][1])


# ---- 6. the extended record ---------------------------------------------------------------------------------------------------------------------
def test_extended_record_storage_and_solve(pkg):
    sc = S.ext_solve_case(pkg)
    case, pv1 = sc["case"], sc["pv1"]
    m, d, h = host_and_device(pkg, case, pv1, sc["phase"], sc["c"])
    assert m.iq().shape[1] == 19
    # the storage comparison of test_gpu_tracers.test_begin_bookkeeping on the 19-field record
    m.set_state(case["pv"], case["meaning"])
    s1, c0 = m.tracer_storage()
    assert np.array_equal(s1, h.storage1) and np.array_equal(c0, h.c_initial) and np.array_equal(c0, sc["c"])
    m.set_state(pv1, case["meaning"])
    m.set_state(case["pv"], case["meaning"])
    d.begin_time_step()
    s2, c2 = m.tracer_storage()
    assert np.array_equal(s2, s1) and np.array_equal(c2, c0)
    m.set_state(pv1, case["meaning"])
    d.begin_time_step()
    h.begin_time_step(m.iq())
    s3, c3 = m.tracer_storage()
    assert np.array_equal(s3, h.storage1) and not np.array_equal(s3, s1) and np.array_equal(c3, c0)
    # the solve
    m, d, h = pair_of(pkg, sc)
    assert m.iq().shape[1] == 19
    systems_equal(d, h, case, sc["phase"])
    solves_equal(m, d, h)


# ---- 7. set_tracers again on a live context -------------------------------------------------------------------------------------------------------
def one_step(m, case, pv1, phase, c, conn):
    """set, begin at the case's state, move to pv1, connections, both systems, the step -> everything that came back"""
    m.set_tracers(phase, c)
    m.set_state(case["pv"], case["meaning"])
    m.tracers_begin_time_step()
    out = list(m.tracer_storage())
    m.set_state(pv1, case["meaning"])
    m.set_tracer_connections(*conn)
    for ph in sorted(set(phase)):
        out += list(m.tracer_system(ph, DT, list(phase).count(ph)))
    res = m.tracers_end_time_step(DT)
    out.append(np.array([[r["converged"], r["iterations"], r["reduction"]] for r in res], float))
    out.append(m.get_tracers())
    return out


def test_set_tracers_again_with_a_wider_batch(pkg):
    """a water batch of two, a step, then 17 water and 3 oil tracers on the same context: maxnt grows and every scratch array is allocated
    anew; begin, both systems and the step give the bits of a fresh context that was handed the second set only"""
    case, pv1 = S.system_case(pkg, (9, 9, 2))
    Nb = case["Nb"]
    rng = np.random.default_rng(21)
    first = ([WATER, WATER], rng.uniform(0.0, 1.0, (2, Nb)), S.system_connections(case, 2))
    phase = [WATER] * 20
    for t in (1, 7, 15):
        phase[t] = OIL
    second = (phase, rng.uniform(0.0, 1.0, (20, Nb)), S.system_connections(case, 20))
    live = model_at(pkg, case, case["pv"])
    a = one_step(live, case, pv1, *first)
    assert a[-2][:, 0].all() and np.abs(a[-1] - first[1]).max() > 0.0      # the first set was solved and moved
    b = one_step(live, case, pv1, *second)
    fresh = one_step(model_at(pkg, case, case["pv"]), case, pv1, *second)
    assert len(b) == len(fresh) == 8
    for x, y in zip(b, fresh):
        assert x.shape == y.shape and np.array_equal(x, y)
    assert b[-2][:, 0].all() and np.isfinite(b[-1]).all() and np.abs(b[-1] - second[1]).max() > 0.0

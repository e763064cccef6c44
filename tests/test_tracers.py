"""Passive tracers at the drop-in boundary and in their CPU form, without a GPU: the symbols are exported, the binding's TracerResult mirrors
opmhip_tracer_result as a C compiler sees include/opmhip.h, and tracers.HostTracers - the comparator of tests/test_gpu_tracers.py - is held
against hand-written scalar arithmetic on the oracle's records of a 3 x 2 x 2 case, against the discrete conservation statements read off
ebos/ecltracermodel.hh:216-337, against a dense solve and against the flow equations' own residual."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_bind
import tracer_states as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("opmhip_set_tracers", "opmhip_set_tracer_solver", "opmhip_set_tracer_connections", "opmhip_tracers_begin_time_step",
               "opmhip_tracers_end_time_step", "opmhip_get_tracers", "opmhip_get_tracer_system", "opmhip_get_tracer_storage",
               "opmhip_get_tracer_timings")
G = 9.80665
DT = S.DT
WATER, OIL = S.WATER, S.OIL


def test_the_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11          # additive: no existing struct changed


def test_tracer_result_matches_the_header(pkg, tmp_path):
    fields = [f[0] for f in pkg.capi.TracerResult._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "opmhip.h"', 'int main(void) {', '  printf("tr %zu\\n", sizeof(opmhip_tracer_result));']
    for f in fields:
        lines.append('  printf("tr.%s %%zu\\n", offsetof(opmhip_tracer_result, %s));' % (f, f))
    lines += ['  printf("cap %d\\n", OPMHIP_TRACERS_MAX_PER_PHASE);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["tr"]) == ctypes.sizeof(pkg.capi.TracerResult)
    assert fields == ["converged", "iterations", "reduction"]
    for f in fields:
        assert int(out["tr." + f]) == getattr(pkg.capi.TracerResult, f).offset, f
    assert int(out["cap"]) == 32


# ---- the 3 x 2 x 2 case ---------------------------------------------------------------------------------------------------------------------
NO_OIL = 4        # a cell of the gas cap with S_w + S_g = 1: an oil tracer there sits on the floor of 1e-10
BLOCKED = (1, 2)  # the THPRES-blocked face


@pytest.fixture(scope="module")
def small(pkg, orc):
    """the records at the start and at the end of a time step, the host form standing at the end: two water tracers and one oil tracer,
    an injecting and a producing connection"""
    case = pkg.decks.cartesian_case(3, 2, 2, state="mixed", heterogeneous=True)
    pv0 = case["pv"].reshape(-1, 3).copy()
    assert case["meaning"][NO_OIL] == pkg.decks.SW_PO_SG
    pv0[NO_OIL, 0], pv0[NO_OIL, 2] = 0.5, 0.5
    case["pv"] = np.ascontiguousarray(pv0.reshape(-1))
    S.block_face(case, *BLOCKED)
    pv1 = S.moved_state(case).reshape(-1, 3)
    pv1[NO_OIL, 0], pv1[NO_OIL, 2] = 0.5, 0.5
    pv1 = np.ascontiguousarray(pv1.reshape(-1))
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    iq0 = o.iq()
    o.set_state(pv1, case["meaning"])
    iq1 = o.iq()
    rng = np.random.default_rng(3)
    c = rng.uniform(0.1, 1.0, (3, case["Nb"]))
    cells, rates = np.array([0, 11]), np.array([[1.0e-3, 2.0e-3, 0.0], [-5.0e-4, -3.0e-3, -0.2]])
    inj = np.array([[0.7, 0.0], [0.2, 0.0], [0.9, 0.0]])

    def host(**kw):
        h = pkg.tracers.HostTracers(case, [WATER, WATER, OIL], c, **kw)
        h.begin_time_step(iq0)
        h.set_records(iq1)
        h.set_connections(cells, rates, inj)
        return h
    return dict(case=case, iq0=iq0, iq1=iq1, c=c, cells=cells, rates=rates, inj=inj, host=host, pv1=pv1, orc=o)


def scalar_face(case, iq, ph, i, j):
    """f = A v b_up with i as the interior cell, written out in Python floats from ebos/eclfluxmodule.hh:212-357 and
    ecltracermodel.hh:182-213 -> (f, i is upstream)"""
    k = S.entry(case, i, j)
    mob_i, mob_j = float(iq[i, 9 + ph, 0]), float(iq[j, 9 + ph, 0])
    if mob_i <= 0.0 and mob_j <= 0.0:
        return 0.0, False
    rho = (float(iq[i, 12 + ph, 0]) + float(iq[j, 12 + ph, 0])) / 2.0
    dz = float(case["depth"][i]) - float(case["depth"][j])
    dp = (float(iq[j, 3 + ph, 0]) + rho * (dz * G)) - float(iq[i, 3 + ph, 0])
    if dp > 0.0:
        up = False
    elif dp < 0.0:
        up = True
    else:
        up = case["volume"][i] > case["volume"][j] or (case["volume"][i] == case["volume"][j] and i < j)
    th = float(case["thpres"][k])
    if not abs(dp) > th:
        return 0.0, False
    dp = dp + th if dp < 0.0 else dp - th
    t, a = float(case["trans"][k]), float(case["area"][k])
    if up:
        v = dp * mob_i * 1.0 * (-t / a)
        surf = float(iq[i, 6 + ph, 0]) * v
    else:
        v = dp * (mob_j * 1.0 * (-t / a))
        surf = float(iq[j, 6 + ph, 0]) * v
    return (0.0 + surf) * a, up


def scalar_row(d, ph, tracer, i):
    """residual and diagonal of row i by hand: storage, faces in ascending column, connections in list order"""
    case, iq0, iq1, c = d["case"], d["iq0"], d["iq1"], d["c"]
    V = float(case["volume"][i])
    vol = lambda q, cell: max(float(q[cell, ph, 0]) * float(q[cell, 6 + ph, 0]) * float(q[cell, 16, 0]), 1e-10)
    r = (vol(iq1, i) * c[tracer, i] - vol(iq0, i) * c[tracer, i]) * V / DT
    dg = vol(iq1, i) * V / DT
    rp, col = case["rowptr"], case["col"]
    for k in range(rp[i], rp[i + 1]):
        j = int(col[k])
        if j == i:
            continue
        f, up = scalar_face(case, iq1, ph, i, j)
        r = r + f * c[tracer, i if up else j]
        if up:
            dg = dg + f
    for n, cell in enumerate(d["cells"]):
        q = d["rates"][n, ph]
        if cell == i and q > 0:
            r = r - q * d["inj"][tracer, n]
        elif cell == i and q < 0:
            r = r - q * c[tracer, i]
            dg = dg - q
    return r, dg


def test_host_form_against_scalar_arithmetic(small):
    d = small
    case, iq1 = d["case"], d["iq1"]
    h = d["host"]()
    sys = {ph: h.system(ph, DT) for ph in (WATER, OIL)}
    # one interior face in each upwind direction (oil): the entry (J, I) carries -f where I is upstream, 0 where it is not
    found = {True: None, False: None}
    for i in range(case["Nb"]):
        for k in range(case["rowptr"][i], case["rowptr"][i + 1]):
            j = int(case["col"][k])
            if j == i or (i, j) == BLOCKED or (j, i) == BLOCKED:
                continue
            f, up = scalar_face(case, iq1, OIL, i, j)
            if f != 0.0 and found[up] is None:
                found[up] = (i, j, f)
    assert found[True] is not None and found[False] is not None
    M = sys[OIL][0]
    i, j, f = found[True]
    assert f > 0.0 and M[S.entry(case, j, i)] == -f
    i, j, f = found[False]
    assert f < 0.0
    g, upj = scalar_face(case, iq1, OIL, j, i)
    assert upj and M[S.entry(case, j, i)] == 0.0 and M[S.entry(case, i, j)] == -g
    # the THPRES-blocked face carries nothing in either phase
    a, b = BLOCKED
    for ph in (WATER, OIL):
        assert scalar_face(case, iq1, ph, a, b) == (0.0, False)
        assert sys[ph][0][S.entry(case, a, b)] == 0.0 and sys[ph][0][S.entry(case, b, a)] == 0.0
    # every row of every tracer, residual and diagonal: the cells of the connections, of the blocked face and of the floor among them
    for ph, tracers in ((WATER, [0, 1]), (OIL, [2])):
        M, r = sys[ph]
        for slot, t in enumerate(tracers):
            for i in range(case["Nb"]):
                rr, dg = scalar_row(d, ph, t, i)
                assert r[slot, i] == rr, (ph, t, i)
                assert M[S.entry(case, i, i)] == dg, (ph, i)
    # the cell without oil: the oil tracer's storage runs on the floor of 1e-10
    assert d["iq1"][NO_OIL, 1, 0] == 0.0
    assert pkg_phase_volume(h, OIL)[NO_OIL] == 1e-10 and h.storage1[2, NO_OIL] == 1e-10 * d["c"][2, NO_OIL]
    # the injecting and the producing connection (oil): - q c_inj into the residual; - q c and - q on the diagonal
    M, r = sys[OIL]
    no_wells = d["host"]()
    no_wells.set_connections([], np.zeros((0, 3)), np.zeros((3, 0)))
    M0, r0 = no_wells.system(OIL, DT)
    assert r[0, 0] == r0[0, 0] - 2.0e-3 * 0.9 and M[S.entry(case, 0, 0)] == M0[S.entry(case, 0, 0)]
    assert r[0, 11] == r0[0, 11] - (-3.0e-3) * d["c"][2, 11] and M[S.entry(case, 11, 11)] == M0[S.entry(case, 11, 11)] - (-3.0e-3)


def pkg_phase_volume(h, ph):
    import importlib
    return importlib.import_module("opm-autodiff_amd").tracers.phase_volume(h.iq, ph)


def test_column_sums_are_the_conservation_statement(small):
    """sum_I M[I][J] = vol_J V_J / dt - sum of the producing q of J: the flux f a cell J sends downstream enters its own diagonal and, negated,
    the row of the receiving cell (ecltracermodel.hh:285-288) - the same bits, so they cancel up to the rounding of the diagonal's
    sequential sum: a few spacings of the largest term of the column"""
    d = small
    case = d["case"]
    h = d["host"]()
    for ph in (WATER, OIL):
        M, _ = h.system(ph, DT)
        A = S.dense(case, M)
        vol = pkg_phase_volume(h, ph)
        expect = vol * case["volume"] / DT
        for n, cell in enumerate(d["cells"]):
            if d["rates"][n, ph] < 0:
                expect[cell] -= d["rates"][n, ph]
        scale = np.abs(A).max(axis=0)
        assert np.all(np.abs(A.sum(axis=0) - expect) <= 8 * np.spacing(scale))
        assert np.all(np.diag(A) > 0) and np.all(A - np.diag(np.diag(A)) <= 0)


def test_closed_box_conserves_the_tracer(small):
    """without connections sum vol V c changes over a step by what the solve leaves: summing the equations at the new concentrations, the
    fluxes cancel (column sums) and (in place new - in place old) / dt = sum of the linear residual rho = r - M dx; so the change is
    sum(rho) dt up to the rounding of sums of N terms of the size of the in-place amounts"""
    d = small
    case = d["case"]
    for tol in (1e-2, 1e-13):
        h = d["host"](tolerance=tol)
        h.set_connections([], np.zeros((0, 3)), np.zeros((3, 0)))
        before = {ph: pkg_phase_volume(h, ph) for ph in (WATER, OIL)}
        old = h.storage1 * case["volume"][None, :]
        sysm = {ph: h.system(ph, DT) for ph in (WATER, OIL)}
        h.end_time_step(DT)
        for ph, tracers in ((WATER, [0, 1]), (OIL, [2])):
            M, r = sysm[ph]
            A = S.dense(case, M)
            for slot, t in enumerate(tracers):
                rho = r[slot] - A @ h.last_dx[t]
                new = before[ph] * case["volume"] * h.c[t]
                change = new.sum() - old[t].sum()
                assert abs(change - rho.sum() * DT) <= 64 * np.spacing(np.abs(old[t]).sum()), (tol, t, change, rho.sum() * DT)
                assert np.linalg.norm(rho) <= tol * np.linalg.norm(r[slot]) * (1 + 1e-6) + 1e-300


def test_tight_tolerance_equals_the_dense_solve(small):
    d = small
    case = d["case"]
    h = d["host"](tolerance=1e-13)
    sysm = {ph: h.system(ph, DT) for ph in (WATER, OIL)}
    res = h.end_time_step(DT)
    assert all(r["converged"] for r in res)
    for ph, tracers in ((WATER, [0, 1]), (OIL, [2])):
        M, r = sysm[ph]
        A = S.dense(case, M)
        kappa = np.linalg.cond(A)
        ref = np.linalg.solve(A, r.T).T
        for slot, t in enumerate(tracers):
            assert np.abs(h.last_dx[t] - ref[slot]).max() <= kappa * 1e-13 * np.abs(ref[slot]).max()
    # the orderings the solver may be handed give the same answer to that accuracy
    for name, order in S.emulated_orders(3, 2, 2).items():
        g = d["host"](tolerance=1e-13)
        g.end_time_step(DT, order)
        assert S.rel_diff(h.last_dx, g.last_dx) <= 1e-10, name


def test_unit_concentration_follows_the_flow_residual(pkg, small):
    """c = 1 everywhere, injected at 1: the tracer's residual IS the residual of its phase's component in the flow equations (water: the
    water equation; oil on a fluid without vaporised oil: the oil equation) - storage (vol - vol_old) V / dt, the faces' A v b_up, the
    connection rates.  So c stays 1 exactly where the flow equations are met exactly and otherwise moves by M^-1 times their residual: it
    does NOT stay 1 at a state that is converged to a Newton tolerance only.  Checked against the oracle's assembly of the same step."""
    d = small
    case, o = d["case"], d["orc"]
    Nb = case["Nb"]
    o.set_state(case["pv"], case["meaning"])
    src = np.zeros((Nb, 3))                              # equations: oil, water, gas
    for n, cell in enumerate(d["cells"]):
        src[cell, 0], src[cell, 1] = d["rates"][n, OIL], d["rates"][n, WATER]
    o.set_source(np.ascontiguousarray(src.reshape(-1)))
    o.set_drift_compensation(False)
    o.assemble(DT, 0)                                    # the old time level's storage
    o.update(case["pv"] - d["pv1"])
    assert np.array_equal(o.get_state()[0], d["pv1"])
    _, R = o.assemble(DT, 1)
    R = R.reshape(Nb, 3)
    h = pkg.tracers.HostTracers(case, [WATER, OIL], np.ones((2, Nb)))
    h.begin_time_step(d["iq0"])
    h.set_records(o.iq())
    h.set_connections(d["cells"], d["rates"], np.ones((2, 2)))
    for ph, eq in ((WATER, 1), (OIL, 0)):
        M, r = h.system(ph, DT)
        # (the oracle sums the same terms in its own order and divides the storage by dt before the volume: roundings of the row's largest term)
        f, _ = pkg.tracers.face_values(case, h.iq, ph)
        rows = np.repeat(np.arange(Nb), np.diff(case["rowptr"]))
        scale = pkg_phase_volume(h, ph) * case["volume"] / DT
        np.maximum.at(scale, rows, np.abs(f))
        np.maximum.at(scale, d["cells"], np.abs(d["rates"][:, ph]))
        if ph == OIL:
            keep = np.arange(Nb) != NO_OIL               # (the floor of 1e-10 is the tracer model's alone)
        else:
            keep = np.ones(Nb, bool)
        assert np.all(np.abs(r[0] - R[:, eq])[keep] <= 16 * np.spacing(scale[keep])), (ph, np.abs(r[0] - R[:, eq]).max())
        assert np.abs(R[:, eq]).max() > 1e3 * np.spacing(scale.max())    # this state is not converged: the residual is there
    h.tolerance = 1e-13
    h.end_time_step(DT)
    assert np.abs(h.c - 1.0).max() > 1e-6                # ... and c moves with it
    # where nothing flows and nothing changes, c = 1 stays 1 to the bit
    still = pkg.tracers.HostTracers(case, [WATER, OIL], np.ones((2, Nb)))
    flat = dict(case, trans=np.zeros_like(case["trans"]))
    still.case = flat
    still.begin_time_step(d["iq0"])
    still.end_time_step(DT)
    assert np.array_equal(still.c, np.ones((2, Nb)))


def test_refusals_and_tables(pkg, small):
    T = pkg.tracers
    case = small["case"]
    with pytest.raises(ValueError, match="gas tracers"):
        T.HostTracers(case, [2], np.ones((1, case["Nb"])))
    with pytest.raises(ValueError):
        T.HostTracers(case, [0], np.full((1, case["Nb"]), np.nan))
    # TVDPF: linear between the nodes, constant beyond the table's ends
    v = T.from_tvdpf([2500.0, 2510.0, 2530.0], [0.0, 1.0, 0.5], [2400.0, 2500.0, 2505.0, 2520.0, 2530.0, 9999.0])
    assert list(v) == [0.0, 0.0, 0.5, 0.75, 0.5, 0.5]
    with pytest.raises(ValueError):
        T.from_tvdpf([1.0, 1.0], [0.0, 1.0], [1.0])
    # the reporting sums (ecltracermodel.hh:298-327, 385-438): one injector, one producer with a crossflowing connection
    pp, producer = [0, 1, 4], [False, True]
    cells, rates = [0, 5, 6, 7], np.array([2.0, -3.0, -1.0, 0.5])
    inj = np.array([[1.0, 0.0, 0.0, 0.25]])
    conc = np.zeros((1, 12))
    conc[0, [5, 6]] = 0.5, 0.1
    bucket = T.BUCKET_PR_DAY
    out = T.well_tracer_rates(pp, producer, cells, rates, inj, conc, official_rate=[2.0, -3.5])
    assert out[0, 0] == 2.0
    assert math.isclose(out[1, 0], (0.5 * 0.25 + -3.0 * 0.5 + -1.0 * 0.1) * (-3.5 / -4.0), rel_tol=1e-15)
    assert T.well_tracer_rates(pp, producer, cells, rates, inj, conc, official_rate=[2.0, -0.5 * bucket])[1, 0] == 0.0     # below a bucket per day
    assert math.isclose(T.well_tracer_rates(pp, producer, cells, rates, inj, conc, official_rate=[2.0, -4.0])[1, 0], 0.5 * 0.25 - 1.5 - 0.1, rel_tol=1e-15)


def test_connection_rates_of_a_host_well_model(pkg):
    class Wm:
        cells = np.array([3, 4])
        last_perf_rates = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])   # components: oil, water, gas
    cells, rates = pkg.tracers.connection_rates(Wm())
    assert list(cells) == [3, 4] and rates.tolist() == [[2.0, 1.0, 3.0], [5.0, 4.0, 6.0]]     # phases: water, oil, gas
    with pytest.raises(ValueError):
        class Fresh:
            cells = np.array([0])
        pkg.tracers.connection_rates(Fresh())


# ---- the cases of tests/test_gpu_tracer_edges.py: what each is for, shown on the oracle's records ------------------------------------------
def records(orc, case, pv):
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(pv, case["meaning"])
    return o.iq()


def host_at(pkg, orc, sc, **kw):
    """the host form of a solve case, begun at the case's own state and standing at pv1"""
    case = sc["case"]
    h = pkg.tracers.HostTracers(case, sc["phase"], sc["c"], **kw)
    h.begin_time_step(records(orc, case, case["pv"]))
    h.set_records(records(orc, case, sc["pv1"]))
    h.set_connections(sc["cells"], sc["rates"], sc["injected"])
    return h


def test_wide_batches_cross_the_chunks(pkg, orc):
    TR_CH = 8
    case, _ = S.system_case(pkg, (9, 9, 2))
    assert S.WIDTHS == (8, 9, 17, 32)
    for nt in S.WIDTHS:
        for wide in (WATER, OIL):
            phase, c = S.wide_tracers(case, nt, wide)
            members = [t for t, p in enumerate(phase) if p == wide]
            assert len(members) == nt and len(phase) == nt + 1 and members != list(range(nt))
            assert phase.count(WATER if wide == OIL else OIL) == 1
            assert len({row.tobytes() for row in c}) == nt + 1
    # the 17 copies: each chunk holds every prototype that fits, the zero tracer in the last slot and below the first chunk's end
    p = S.PROTO_17
    assert len(p) == 17 and p[16] == 2 and 2 in p[:TR_CH]
    assert set(p[:TR_CH]) == set(p[TR_CH:2 * TR_CH]) == {0, 1, 2}
    assert sorted(S.PERM_17) == list(range(17)) and all(a != b for a, b in enumerate(S.PERM_17))
    assert [p[s] for s in S.PERM_17] != list(p)
    assert sorted(S.PROTO_9) == [0, 0, 0, 1, 1, 1, 2, 2, 2] and any(S.PROTO_9[s] != S.PROTO_9[s % 3] for s in range(9))
    # the prototypes stop at three different half iterations, every decision clear
    sc = S.proto_solve_case(pkg, (9, 9, 2), (0, 1, 2))
    res = host_at(pkg, orc, sc).end_time_step(DT)
    its = [r["iterations"] for r in res]
    assert S.clear_decisions(res, 1e-2) and all(r["converged"] for r in res)
    assert its[2] == 0.0 and len(set(its)) == 3, its


def reduction_layout(Nb):
    """opmhip_set_tracers (csrc/capi_tracers.cpp): nblk = max(1, min(256, ceil(Nb / 256))), cellsPerBlock = ceil(Nb / nblk); k_tracer_dot:
    workgroup b sums the cells [b cells, min(Nb, b cells + cells))"""
    nblk = max(1, min(256, (Nb + 255) // 256))
    cells = (Nb + nblk - 1) // nblk
    return nblk, cells, [(b * cells, min(Nb, b * cells + cells)) for b in range(nblk)]


def test_reduction_grids_take_more_than_one_workgroup():
    want = {(17, 17, 1): (2, 145, [145, 144]), (23, 23, 1): (3, 177, [177, 177, 175])}
    assert set(S.REDUCTION_GRIDS) == set(want)
    for dims, (nblk, cells, sizes) in want.items():
        Nb = dims[0] * dims[1] * dims[2]
        n, c, ranges = reduction_layout(Nb)
        assert (n, c) == (nblk, cells) and [b - a for a, b in ranges] == sizes
        assert all(b > a for a, b in ranges) and ranges[0][0] == 0 and ranges[-1][1] == Nb
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(n - 1))
        assert sizes[-1] < cells                                 # a ragged last workgroup
    assert reduction_layout(162)[0] == 1                         # the grids of the older tests stay in one
    for nt, W in ((3, 255), (9, 252), (17, 255), (32, 256)):
        assert 256 - 256 % nt == W


def test_dry_case_sits_on_the_clamp_and_has_one_sided_faces(pkg, orc):
    T = pkg.tracers
    sc = S.dry_case(pkg)
    case, dry = sc["case"], sc["dry"]
    assert len(dry) == 13 and case["Nb"] == 90
    rows = np.repeat(np.arange(case["Nb"]), np.diff(case["rowptr"]))
    cols = np.asarray(case["col"])
    isolated = dry[-1]
    assert not np.isin(cols[rows == isolated], dry[:-1]).any()   # no neighbour of the isolated cell is dry
    wet = np.ones(case["Nb"], bool)
    wet[dry] = False
    for pv in (case["pv"], sc["pv1"]):
        iq = records(orc, case, pv)
        assert np.all(iq[dry, T.F_MOB + WATER, 0] == 0.0) and np.all(iq[wet, T.F_MOB + WATER, 0] > 0.0)
        vol = T.phase_volume(iq, WATER)
        assert np.all(vol[dry] == 1e-10) and np.all(vol[wet] > 1e-10)
        assert np.all(T.phase_volume(iq, OIL) > 1e-10)
    f, up = T.face_values(case, iq, WATER)
    off = rows != cols
    mob = iq[:, T.F_MOB + WATER, 0] > 0.0
    both_dry = off & ~mob[rows] & ~mob[cols]
    assert both_dry.sum() >= 2 and np.all(f[both_dry] == 0.0)
    one_in = off & ~mob[rows] & mob[cols]                       # the interior cell is the immobile one
    one_ex = off & mob[rows] & ~mob[cols]
    for one in (one_in, one_ex):
        assert (one & up).sum() > 0 and (one & ~up).sum() > 0    # each upwind direction occurs
    # an immobile upstream side carries nothing; a mobile one carries water into the dry cell
    assert np.all(f[one_in & up] == 0.0) and np.all(f[one_ex & ~up] == 0.0)
    assert np.all(f[one_in & ~up] != 0.0) and np.all(f[one_ex & up] != 0.0)
    # a producing connection inside the dry column, an injecting one outside
    q = sc["rates"][:, WATER]
    assert any(q[n] < 0 and sc["cells"][n] in dry[:-1] for n in range(len(q))) and any(q[n] > 0 and wet[sc["cells"][n]] for n in range(len(q)))
    h = host_at(pkg, orc, sc)
    assert np.all(h.storage1[0, dry] == 1e-10 * sc["c"][0, dry])
    res = h.end_time_step(DT)
    assert S.clear_decisions(res, 1e-2) and all(r["converged"] for r in res)


def test_pivot_case_is_reported_bad_by_the_host_form(pkg, orc):
    T = pkg.tracers
    sc = S.pivot_case(pkg)
    case, cell = sc["case"], sc["cell"]
    assert np.isfinite(sc["rates"]).all() and list(sc["cells"]).count(cell) == 2 and sc["c"][0, cell] == 0.0
    h = host_at(pkg, orc, sc, maxit=2)
    with np.errstate(all="ignore"):
        M, r = h.system(OIL, DT)
        assert M[S.entry(case, cell, cell)] == np.inf and np.isfinite(np.delete(M, S.entry(case, cell, cell))).all()
        assert np.isfinite(r[0]).all()                           # the tracer that is absent from the cell keeps a finite residual
        rp, ci, va, dg = T.permute_csr(case["Nb"], h.rowptr, h.col, M)
        lu, invd, bad = T.ilu0(rp, ci, va, dg)
        assert bad and np.isfinite(lu).all() and np.isfinite(invd).all()      # nothing that is not finite is stored
        res = h.end_time_step(DT)
    assert [q["converged"] for q in res] == [False, True, False]
    assert res[0]["iterations"] == 2.0 and res[2]["iterations"] == 2.0 and 0.0 < res[1]["iterations"] < 2.0
    assert S.clear_decisions([res[1]], 1e-2) and np.isfinite(h.c[1]).all()
    # a step later, with a sane list: the water tracer is solved as ever
    h.begin_time_step()
    h.set_connections(*sc["sane"])
    with np.errstate(all="ignore"):
        res2 = h.end_time_step(DT)
    assert res2[1]["converged"] and S.clear_decisions([res2[1]], 1e-2) and np.isfinite(h.c[1]).all()


def test_wave_connections_name_71_cells_and_one_of_them_five_times():
    case = dict(Nb=162)
    cells, rates, inj, many = S.wave_connections(case, 11)
    assert len(cells) == 75 and rates.shape == (75, 3) and inj.shape == (11, 75)
    assert len(set(cells.tolist())) == 71 > 64 and list(cells).count(many) == 5
    once = cells != many
    assert list(cells[once]) != sorted(cells[once])              # shuffled cell order
    for ph in (WATER, OIL):
        assert (np.sign(rates[~once, ph]) == [1, -1, 0, -1, 1]).all()
        assert (rates[once, ph] > 0).sum() > 10 and (rates[once, ph] < 0).sum() > 10
    assert 0 <= cells.min() and cells.max() < 162

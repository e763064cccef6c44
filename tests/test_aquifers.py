"""Analytic aquifers at the drop-in boundary and in their CPU form, without a GPU: the symbols are exported, the Python binding's Aquifers
mirrors opmhip_aquifers field by field as a C compiler sees include/opmhip.h, the struct builder rejects ragged input, connections()
follows AquiferInterface::initializeConnections, and aquifers.HostAquifers - the comparator of tests/test_gpu_aquifers.py - is held
against hand-written scalar arithmetic, a finite difference of its own rates and the sequential sum of Q dt."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("opmhip_set_aquifers", "opmhip_aquifers_begin_time_step", "opmhip_get_aquifers", "opmhip_get_aquifer_rates")
G = 9.80665


def test_the_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11          # additive: no existing struct changed


def test_aquifers_struct_matches_the_header(pkg, tmp_path):
    fields = [f[0] for f in pkg.capi.Aquifers._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "opmhip.h"', 'int main(void) {', '  printf("aq %zu\\n", sizeof(opmhip_aquifers));']
    for f in fields:
        lines.append('  printf("aq.%s %%zu\\n", offsetof(opmhip_aquifers, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["aq"]) == ctypes.sizeof(pkg.capi.Aquifers)
    assert len(out) == 1 + len(fields) == 22
    for f in fields:
        assert int(out["aq." + f]) == getattr(pkg.capi.Aquifers, f).offset, f


def two_records(pkg):
    A = pkg.aquifers
    ct = A.carter_tracy(7, dict(cells=[4, 2, 9], alpha=[0.5, 0.25, 0.25]), 1e7, 2e-4, 1000.0, 2600.0, [0.1, 1.0, 10.0], [0.3, 0.8, 1.6])
    fk = A.fetkovich(8, dict(cells=[2, 3], alpha=[0.4, 0.6]), 3e7, 5e-8, 1e-9, 2e10, 1020.0, 2610.0, initial_pressure=260e5, restart=dict(W_flux=5.0, pressure=259e5))
    return ct, fk


def test_struct_builder(pkg):
    ct, fk = two_records(pkg)
    s, keep = pkg.capi.make_aquifers([ct, fk])
    assert s.num_aquifers == 2
    assert list(keep["type"]) == [0, 1] and list(keep["id"]) == [7, 8]
    assert list(keep["conn_pointers"]) == [0, 3, 5] and list(keep["cell"]) == [4, 2, 9, 2, 3]
    assert list(keep["table_pointers"]) == [0, 3, 3] and list(keep["td"]) == [0.1, 1.0, 10.0]
    assert list(keep["has_initial_pressure"]) == [0, 1] and keep["initial_pressure"][1] == 260e5
    assert list(keep["has_restart"]) == [0, 1] and keep["restart_W_flux"][1] == 5.0 and keep["restart_pressure"][1] == 259e5
    assert s.cell == keep["cell"].ctypes.data and s.pd == keep["pd"].ctypes.data
    assert pkg.capi.make_aquifers(None) == (None, []) and pkg.capi.make_aquifers([]) == (None, [])


@pytest.mark.parametrize("which,key,change", [(0, "alpha", lambda a: a[:-1]), (0, "cells", lambda a: np.append(a, 1)), (0, "pd", lambda a: a[:-1]),
                                              (0, "td", lambda a: np.append(a, 20.0)), (1, "alpha", lambda a: np.append(a, 0.1)),
                                              (1, "type", lambda a: "numerical"), (1, "prod_index", None), (0, "influx_constant", None),
                                              (0, "time_constant", None)])
def test_struct_builder_rejects_ragged_input(pkg, which, key, change):
    recs = list(two_records(pkg))
    if change is None:
        del recs[which][key]
    else:
        recs[which][key] = change(recs[which][key] if isinstance(recs[which][key], str) else np.asarray(recs[which][key]))
    with pytest.raises(ValueError):
        pkg.capi.make_aquifers(recs)


def test_connections(pkg):
    A = pkg.aquifers
    case = pkg.decks.cartesian_case(5, 4, 3)
    bottom = A.connections(case, (0, 4, 0, 3, 2, 2), "K+")
    assert len(bottom["cells"]) == 20 and np.array_equal(bottom["cells"], 40 + np.arange(20))
    assert abs(bottom["alpha"].sum() - 1.0) < 1e-15 and np.all(bottom["alpha"] == 0.05) and np.all(bottom["area"] == 400.0)
    # an interior box: connected cells, none of them at the grid's boundary -> every alpha 0 (the sum is below sqrt(eps))
    inner = A.connections(case, (1, 3, 1, 2, 1, 1), "K+")
    assert len(inner["cells"]) == 6 and np.all(inner["alpha"] == 0.0)
    # the wrong face: the bottom layer has no boundary towards K-
    wrong = A.connections(case, (0, 4, 0, 3, 2, 2), "K-")
    assert np.all(wrong["area"] == 0.0) and np.all(wrong["alpha"] == 0.0)
    # the whole box with a side face: only the cells of that side count, weighted by the coefficients handed in
    side = A.connections(case, (0, 4, 0, 3, 0, 2), "I-", influx_coeff=np.arange(60) + 1.0)
    on = side["alpha"] > 0.0
    assert np.array_equal(side["cells"][on] % 5, np.zeros(12)) and on.sum() == 12 and abs(side["alpha"].sum() - 1.0) < 1e-15
    assert np.array_equal(side["alpha"][on], (side["cells"][on] + 1.0) / (side["cells"][on] + 1.0).sum())
    # the same on a grid given as connections (transmissibility.cartesian_faces) with an inactive cell: its upper neighbour's K+ face becomes a boundary
    act = np.ones(60, int)
    act[45] = 0
    g = pkg.transmissibility.cartesian_faces(5, 4, 3, 20.0, 20.0, 5.0, 2500.0, actnum=act)
    mid = A.connections((g, (5, 4, 3)), (0, 4, 0, 3, 1, 1), "K+")
    assert len(mid["cells"]) == 20 and list(mid["cells"][mid["alpha"] > 0.0]) == [25] and mid["alpha"][5] == 1.0


class FakeModel:
    """a model object with whole-array hooks only: records handed out as they are, sources kept"""

    def __init__(self, n):
        self.rec = np.zeros((n, 17, 4))
        self.source = self.dsource = None

    def iq(self):
        return self.rec

    def set_source(self, s, d=None):
        self.source, self.dsource = np.array(s).reshape(-1, 3), np.array(d).reshape(-1, 9)


def test_host_aquifers_against_scalar_arithmetic(pkg):
    """one connection per aquifer, both types, a three-node influence table read inside, at a node and beyond its last node"""
    A = pkg.aquifers
    depth = np.array([2500.0, 2520.0, 2540.0])
    Tc, beta, rho, datum, pa0 = 4.0e6, 3.0e-4, 1010.0, 2530.0, 255.0e5
    x, y = [0.5, 2.0, 6.0], [0.6, 1.1, 1.9]
    ct = A.carter_tracy(1, dict(cells=[2], alpha=[0.7]), Tc, beta, rho, datum, x, y, initial_pressure=pa0)
    J, Ct, V0, paf = 4.0e-8, 2.0e-9, 1.0e10, 251.0e5
    fk = A.fetkovich(2, dict(cells=[1], alpha=[0.9]), 2.5e6, J, Ct, V0, rho, datum, initial_pressure=paf)
    m = FakeModel(3)
    base = np.zeros((3, 3))
    base[2] = [-1e-3, 2e-3, 0.0]
    h = A.HostAquifers([ct, fk], depth, base_source=base)
    h.initial_solution_applied(m)
    W = [0.0, 0.0]
    pa = paf
    time = 0.0
    for step, (dt, expect_interval) in enumerate([(1.0e6, 0), (7.0e6, 1), (3.0e7, 1)]):    # td + dt = 0.25 (left of the table), 2.0 (a node), 9.5 (beyond the last)
        m.rec[:, 3, 0] = [250.1e5 - 1e4 * step, 250.4e5 - 2e4 * step, 250.9e5 - 3e4 * step]
        h.begin_time_step(m, time, dt)
        pprev = m.rec[:, 3, 0].copy()
        m.rec[:, 3, :] = [[249.0e5, 0.1, 1.0, 0.0], [249.5e5, -3e3, 1.0, 0.0], [250.0e5, -2e3, 1.0, 5.0]]     # the iterate: p_w with derivatives
        h.add_to_source(m)
        # Carter-Tracy by hand (AquiferCarterTracy.hpp:135-169)
        tdp = (dt + time) / Tc
        j = expect_interval
        assert (x[j] <= tdp or j == 0) and (tdp < x[j + 1] or j == 1)
        slope = (y[j + 1] - y[j]) / (x[j + 1] - x[j])
        PItd = slope * (tdp - x[j]) + y[j]
        gdz = G * (depth[2] - datum)
        dpai = pa0 + rho * gdz - pprev[2]
        denom = Tc * (PItd - (time / Tc) * slope)
        a = (beta * dpai - W[0] * slope) / denom
        b = beta / denom
        q_ct = 0.7 * (a - b * (250.0e5 - pprev[2]))
        dq_ct = [0.7 * -(b * d) for d in (-2e3, 1.0, 5.0)]
        # Fetkovich by hand (AquiferFetkovich.hpp:112-148)
        coef = (1 - math.exp(-(dt / 2.5e6))) / (dt / 2.5e6)
        gdzf = G * (depth[1] - datum)
        c = coef * 0.9 * J
        q_fk = c * (pa + rho * gdzf - 249.5e5)
        dq_fk = [c * -d for d in (-3e3, 1.0, 0.0)]
        assert np.array_equal(h.a[0]["Q"], [[q_ct] + dq_ct]) and np.array_equal(h.a[1]["Q"], [[q_fk] + dq_fk])
        assert q_ct != 0.0 and q_fk != 0.0
        want = base.copy()
        want[2, 1] += q_ct
        want[1, 1] += q_fk
        assert np.array_equal(m.source, want)
        assert np.array_equal(m.dsource[2, 3:6], dq_ct) and np.array_equal(m.dsource[1, 3:6], dq_fk) and np.count_nonzero(m.dsource) == 5
        h.end_time_step(dt)
        W[0] += q_ct * dt
        W[1] += q_fk * dt
        pa = paf - W[1] / (Ct * V0)
        d = h.data()
        assert np.array_equal(d["W_flux"], W) and np.array_equal(d["pressure"], [pa0, pa]) and np.array_equal(d["init_pressure"], [pa0, paf])
        assert np.array_equal(d["flux_rate"], [q_ct, q_fk])
        time += dt
    assert pa != paf


def test_equilibrium_pressure_and_refusals_of_the_host_form(pkg):
    A = pkg.aquifers
    depth = np.array([2500.0, 2510.0, 2520.0, 2530.0])
    m = FakeModel(4)
    m.rec[:, 3, 0] = [250e5, 251e5, 252e5, 253e5]
    m.rec[:, 12, 0] = [1000.0, 1001.0, 1002.0, 1003.0]
    fk = A.fetkovich(1, dict(cells=[3, 1], alpha=[0.25, 0.75]), 1e6, 1e-8, 1e-9, 1e10, 1000.0, 2515.0)
    h = A.HostAquifers([fk], depth)
    h.initial_solution_applied(m)
    # ascending cell order: cell 1 first (AquiferInterface.hpp:330-373)
    s = 0.0
    s += 0.75 * (251e5 - 1001.0 * (G * (2510.0 - 2515.0)))
    s += 0.25 * (253e5 - 1003.0 * (G * (2530.0 - 2515.0)))
    assert h.data()["init_pressure"][0] == s / (0.25 + 0.75) and h.data()["pressure"][0] == s / (0.25 + 0.75)
    ct, fk2 = two_records(pkg)
    with pytest.raises(ValueError):
        A.HostAquifers([fk2, ct], np.zeros(10))                      # Carter-Tracy first
    ct["restart"] = dict(W_flux=1.0)
    with pytest.raises(ValueError):
        A.HostAquifers([ct], np.zeros(10)).initial_solution_applied(FakeModel(10))
    with pytest.raises(ValueError):
        A.HostAquifers([A.fetkovich(1, dict(cells=[1, 1], alpha=[0.5, 0.5]), 1e6, 1e-8, 1e-9, 1e10, 1000.0, 2515.0)], depth)


def test_dsource_is_the_derivative_of_the_rates_on_the_oracle_model(pkg, orc):
    """HostAquifers on the oracle's model: what it hands over as dsource equals a central finite difference of Q in the primary variables.
    p_w = p_o - pcow(Sw) with a piecewise-linear pcow: Q is linear in p and, inside a table interval, in Sw - the difference quotient has
    no truncation error and the tolerance is its rounding error alone: p_w carries an error of eps |p_w| on either side, so the quotient of
    Q = c (P - p_w) is off by at most c * 2 eps |p_w| / (2 h) in the units of h; twice that is allowed (the record's own rounding)."""
    A = pkg.aquifers
    case = helpers.hysteresis_case(pkg, 4, 3, 3, perturb=False)      # non-zero capillary pressure: p_w depends on Sw
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    recs = pkg.decks.two_aquifers(case, None, None)
    h = A.HostAquifers(recs, case["depth"])
    h.initial_solution_applied(om)
    h.begin_time_step(om, 3.0e6, 2.0e6)
    pv0 = case["pv"].reshape(-1, 3).copy()
    pv0[:, 1] += 2.0e5                       # an iterate away from the state of the step's start
    om.set_state(pv0.reshape(-1), case["meaning"])
    q = h.rates(om.iq()[h.cells]).copy()
    assert np.all(q[:, 2] != 0.0) and np.any(q[:, 1] != 0.0) and np.all(q[:, 3] == 0.0)
    pw = np.abs(om.iq()[h.cells, 3, 0]).max()
    eps = np.finfo(float).eps
    for var, step in ((0, 1e-5), (1, 100.0), (2, 1e-6)):
        qq = []
        for sgn in (+1.0, -1.0):
            pv = pv0.copy()
            pv[:, var] += sgn * step
            om.set_state(pv.reshape(-1), case["meaning"])
            qq.append(h.rates(om.iq()[h.cells])[:, 0].copy())
        fd = (qq[0] - qq[1]) / (2.0 * step)
        tol = 2.0 * np.abs(q[:, 2]) * 2.0 * eps * pw / (2.0 * step)
        assert np.all(np.abs(fd - q[:, 1 + var]) <= tol), (var, np.abs(fd - q[:, 1 + var]).max(), tol.min())


def test_w_flux_is_the_sequential_sum_of_q_dt(pkg):
    A = pkg.aquifers
    n = 11
    rng = np.random.default_rng(3)
    depth = 2500.0 + 5.0 * np.arange(n)
    conn = dict(cells=rng.permutation(n)[:7], alpha=np.full(7, 1.0 / 7.0))
    fk = A.fetkovich(1, conn, 1e6, 1e-8, 1e-9, 1e10, 1000.0, 2520.0, initial_pressure=255e5)
    ct = A.carter_tracy(2, conn, 2e6, 1e-4, 1000.0, 2520.0, [0.1, 1.0, 5.0], [0.3, 0.8, 1.4], initial_pressure=256e5)
    m = FakeModel(n)
    h = A.HostAquifers([ct, fk], depth)
    h.initial_solution_applied(m)
    W = [0.0, 0.0]
    t = 0.0
    for dt in (1e5, 3e5, 2e5):
        m.rec[:, 3, 0] = 250e5 + 1e4 * rng.standard_normal(n)
        h.begin_time_step(m, t, dt)
        m.rec[:, 3, 0] -= 1e4
        m.rec[:, 3, 2] = 1.0
        h.add_to_source(m)
        h.end_time_step(dt)
        for k, r in enumerate(h.a):
            for qv in r["Q"][:, 0]:
                W[k] += qv * dt
        t += dt
        assert np.array_equal(h.data()["W_flux"], W)
    assert W[0] != 0.0 and W[1] != 0.0

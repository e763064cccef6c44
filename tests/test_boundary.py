"""Open boundaries (FREE and RATE faces of the BC keyword) at the drop-in boundary and in their CPU form, without a GPU: the symbols are
exported, the binding's struct mirrors opmhip_boundary_conditions as a C compiler sees include/opmhip.h, the struct builder rejects
ragged input, faces() finds the grid's boundary faces with their geometry, and boundary.HostBoundary - the comparator of
tests/test_gpu_boundary.py - is held against the properties that do not depend on its own statement order: no flux at the capture
state, derivatives against central differences, the composition an inflowing and an outflowing phase carries, a RATE face's numbers.
The records come from the CPU oracle's intensive quantities."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers
import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("opmhip_set_boundary_conditions", "opmhip_get_boundary_rates")
LATERAL = ("I-", "I+", "J-", "J+")
ALL = LATERAL + ("K-", "K+")


def test_the_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11          # additive: no existing struct changed


def test_struct_matches_the_header(pkg, tmp_path):
    S = pkg.capi.BoundaryConditions
    fields = [f[0] for f in S._fields_]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "opmhip.h"', 'int main(void) {',
             '  printf("bc %zu\\n", sizeof(opmhip_boundary_conditions));', '  printf("types %d\\n", OPMHIP_BC_RATE * 10 + OPMHIP_BC_FREE);']
    for f in fields:
        lines.append('  printf("bc.%s %%zu\\n", offsetof(opmhip_boundary_conditions, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["bc"]) == ctypes.sizeof(S) and len(out) == 2 + len(fields) == 10
    assert int(out["types"]) == pkg.capi.BOUNDARY_TYPES["rate"] * 10 + pkg.capi.BOUNDARY_TYPES["free"]
    for f in fields:
        assert int(out["bc." + f]) == getattr(S, f).offset, f


def test_struct_builder(pkg):
    B = pkg.boundary
    case = pkg.decks.cartesian_case(3, 2, 2)
    west, top = B.faces(case, (0, 2, 0, 1, 0, 1), "I-"), B.faces(case, (0, 2, 0, 1, 0, 1), "K-")
    recs = [B.free(west), B.rate(top, [0.0, -2.0e-4, 0.0])]
    s, keep = pkg.capi.make_boundary_conditions(recs)
    assert s.num_faces == 4 + 6 and list(keep["cell"]) == [0, 3, 6, 9, 0, 1, 2, 3, 4, 5]
    assert list(keep["type"]) == [1] * 4 + [0] * 6 and list(keep["direction"]) == [0] * 4 + [4] * 6
    assert keep["rate"].shape == (30,) and np.all(keep["rate"][:12] == 0.0) and list(keep["rate"][12:15]) == [0.0, -2.0e-4, 0.0]
    assert s.cell == keep["cell"].ctypes.data and s.rate == keep["rate"].ctypes.data
    assert pkg.capi.make_boundary_conditions(None)[0] is None and pkg.capi.make_boundary_conditions([])[0] is None
    for key, change in (("area", lambda a: a[:-1]), ("depth", lambda a: np.append(a, 1.0)), ("type", lambda a: "thermal"), ("trans", None)):
        bad = dict(recs[0])
        if change is None:
            del bad[key]
        else:
            bad[key] = change(bad[key])
        with pytest.raises(ValueError):
            pkg.capi.make_boundary_conditions([bad])
    with pytest.raises(ValueError):
        pkg.capi.make_boundary_conditions([dict(recs[1], rate=np.zeros((5, 3)))])
    with pytest.raises(ValueError):
        B.HostBoundary([B.free(west), B.rate(west, [0.0, 0.0, 0.0])], case["depth"], case["fluid"])        # a (cell, direction) pair twice


def test_faces_of_a_row_of_three_cells(pkg):
    """3 x 1 x 1: the end cells have five boundary faces, the middle cell four; areas, face depths and half transmissibilities"""
    B = pkg.boundary
    case = pkg.decks.cartesian_case(3, 1, 1, dx=20.0, dy=10.0, dz=4.0, top=1000.0, perm_md=100.0)
    per_cell = np.zeros(3, int)
    for face in ALL:
        fc = B.faces(case, (0, 2, 0, 0, 0, 0), face)
        per_cell[fc["cells"]] += 1
        axis = pkg.boundary.FACES[face] // 2
        area = [10.0 * 4.0, 20.0 * 4.0, 20.0 * 10.0][axis]
        half = [10.0, 5.0, 2.0][axis]
        assert np.all(fc["area"] == area) and np.all(fc["direction"] == B.FACES[face])
        np.testing.assert_allclose(fc["trans"], case["perm"][fc["cells"]] * area / half, rtol=1e-14)            # K A d / d^2
        want_depth = 1002.0 + {"K-": -2.0, "K+": 2.0}.get(face, 0.0)
        assert np.all(fc["depth"] == want_depth)
        assert len(fc["cells"]) == (1 if axis == 0 else 3)
    assert list(per_cell) == [5, 4, 5]
    assert len(B.faces(case, (1, 1, 0, 0, 0, 0), "I-")["cells"]) == 0                      # the middle cell has no boundary towards I-
    assert B.faces(case, (1, 1, 0, 0, 0, 0), "I-")["trans"].shape == (0,)


def test_faces_of_a_corner_point_grid_with_an_inactive_cell(pkg):
    """a sheared, dipping 4 x 3 x 2 corner-point grid with one inactive cell: its neighbours' faces towards it become boundaries; areas are
    those of the cells' own quadrilaterals, depths their centres', the half transmissibility K |A . d| / |d|^2"""
    B, T = pkg.boundary, pkg.transmissibility
    nx, ny, nz = 4, 3, 2
    coord, zcorn = T.cartesian_cornerpoint(nx, ny, nz, 20.0, 10.0, 4.0, top=2000.0, shear=(0.05, 0.0), dip=0.02)
    act = np.ones(nx * ny * nz, int)
    dead = 1 + nx * 1                      # (1, 1, 0)
    act[dead] = 0
    g = T.cornerpoint_faces(nx, ny, nz, coord, zcorn, actnum=act)
    corners = T.cornerpoint_corners(nx, ny, nz, coord, zcorn)
    perm = np.tile(np.array([1.0, 2.0, 0.1]) * 1e-13, (g["n"], 1))
    whole = (0, nx - 1, 0, ny - 1, 0, nz - 1)
    count = {f: len(B.faces((g, (nx, ny, nz)), whole, f, perm=perm, corners=corners)["cells"]) for f in ALL}
    # the box's own sides minus the dead cell's share, plus the faces of its five active neighbours that look at it (it lies in the top
    # layer, away from the lateral sides: its K- face was a boundary of the box, its K+ neighbour's K- face becomes one)
    assert count == {"I-": ny * nz + 1, "I+": ny * nz + 1, "J-": nx * nz + 1, "J+": nx * nz + 1, "K-": nx * ny - 1 + 1, "K+": nx * ny}
    with pytest.raises(ValueError):
        B.faces((g, (nx, ny, nz)), whole, "I-")
    comp = {int(c): n for n, c in enumerate(g["cart"])}
    fc = B.faces((g, (nx, ny, nz)), whole, "I+", perm=perm, corners=corners)
    assert comp[dead - 1] in fc["cells"]                                                   # (0, 1, 0) now has a boundary towards I+
    n = list(fc["cells"]).index(comp[dead - 1])
    c = corners[dead - 1]
    quad = np.array([c[0, 0, 1], c[0, 1, 1], c[1, 1, 1], c[1, 0, 1]])
    centre = quad.mean(axis=0)
    # a planar parallelogram: its area is |e1 x e2|
    area = np.linalg.norm(np.cross(quad[1] - quad[0], quad[3] - quad[0]))
    np.testing.assert_allclose(fc["area"][n], area, rtol=1e-13)
    assert fc["depth"][n] == centre[2]
    d = centre - g["centroid"][comp[dead - 1]]
    nrm = np.cross(quad[1] - quad[0], quad[3] - quad[0])
    np.testing.assert_allclose(fc["trans"][n], 1e-13 * abs(nrm @ d) / (d @ d), rtol=1e-13)


# ---- HostBoundary on the oracle's records ---------------------------------------------------------------------------------------------
def lateral_free(pkg, case):
    B = pkg.boundary
    box = (0, case["nx"] - 1, 0, case["ny"] - 1, 0, case["nz"] - 1)
    return [B.free(B.faces(case, box, f)) for f in LATERAL]


def make_case(pkg, kind):
    if kind == "wetgas":
        return helpers.wetgas_case(pkg, 4, 3, 3, heterogeneous=True)
    return pkg.decks.cartesian_case(4, 3, 2, state="mixed", heterogeneous=True)


def oracle_at(orc, case, pv=None):
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"] if pv is None else pv, case["meaning"])
    return o


def moved(case, sign, dp=2.0e5, seed=3):
    rng = np.random.default_rng(seed)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 1] += sign * dp * rng.uniform(0.5, 1.0, len(pv))
    return pv


@pytest.mark.parametrize("kind", ["blackoil", "wetgas"])
def test_no_flux_at_the_capture_state(pkg, orc, kind):
    """every lateral FREE face of a box grid: distZ = 0 and equal pressures - zero to the bit, value and derivative rows of the value"""
    case = make_case(pkg, kind)
    h = pkg.boundary.HostBoundary(lateral_free(pkg, case), case["depth"], case["fluid"])
    o = oracle_at(orc, case)
    h.initial_solution_applied(o)
    Q = h.rates_now(o)
    assert Q.shape == (2 * (4 + 3) * case["nz"], 12) and np.all(Q[:, :3] == 0.0)
    assert np.all(h.composition == 0) and not np.any(h.upwind_exterior)
    # top and bottom faces: gravity alone drives a flux there, but with equal raw pressures no phase adds to the equations
    B = pkg.boundary
    box = (0, 3, 0, 2, 0, case["nz"] - 1)
    hz = B.HostBoundary([B.free(B.faces(case, box, "K-")), B.free(B.faces(case, box, "K+"))], case["depth"], case["fluid"])
    hz.initial_solution_applied(o)
    assert np.all(hz.rates_now(o) == 0.0) and np.any(hz.upwind_exterior)


@pytest.mark.parametrize("kind", ["blackoil", "wetgas"])
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_derivatives_against_central_differences(pkg, orc, kind, sign):
    """the 3 x 3 derivative of every face (all six sides, so that gravity takes part) against central differences of the value, with the
    steps and the bound of the well-equation check of tests/test_spe1_deck.py; |dp| is 1 to 2 bar, far from the switch of the branches"""
    case = make_case(pkg, kind)
    B = pkg.boundary
    box = (0, 3, 0, 2, 0, case["nz"] - 1)
    h = B.HostBoundary([B.free(B.faces(case, box, f)) for f in ALL], case["depth"], case["fluid"])
    h.initial_solution_applied(oracle_at(orc, case))
    pv = moved(case, sign)
    Q = h.rates_now(oracle_at(orc, case, pv.reshape(-1))).copy()
    up0, comp0 = h.upwind_exterior.copy(), h.composition.copy()
    assert np.all(up0[np.isin(h.direction, (0, 1, 2, 3))] == (sign < 0)) and np.all(comp0 == (1 if sign < 0 else -1))
    D = Q[:, 3:].reshape(-1, 3, 3)
    meaning = case["meaning"][h.cells]
    worst = 0.0
    for v in range(3):
        step = np.array([1e-6, 50.0, 1e-6])[v] * np.ones(case["Nb"])
        if v == 2:
            step = np.where(case["meaning"] == 0, 1e-6, 1e-4)
        vals = []
        for s in (1.0, -1.0):
            p = pv.copy()
            p[:, v] += s * step
            vals.append(h.rates_now(oracle_at(orc, case, p.reshape(-1)))[:, :3].copy())
            assert np.array_equal(h.upwind_exterior, up0) and np.array_equal(h.composition, comp0)
        fd = (vals[0] - vals[1]) / (2 * step[h.cells])[:, None]
        for e in range(3):
            scale = np.abs(D[:, e, :]).max()
            worst = max(worst, float((np.abs(D[:, e, v] - fd[:, e]) / (2e-5 * np.abs(fd[:, e]) + 1e-9 * scale)).max()))
            np.testing.assert_allclose(D[:, e, v], fd[:, e], rtol=2e-5, atol=1e-9 * scale)
    print("worst deviation / allowed: %.3f" % worst)
    assert np.any(D != 0.0) and len(set(meaning.tolist())) >= 2


def only_phase(rec, ext, ph):
    """records and captured state in which only phase ph is mobile"""
    rec, ext = rec.copy(), {k: v.copy() for k, v in ext.items()}
    for other in range(3):
        if other != ph:
            rec[:, 9 + other, :] = 0.0
            ext["mob"][:, other] = 0.0
    return rec, ext


@pytest.mark.parametrize("kind", ["blackoil", "wetgas"])
def test_composition_of_inflow_and_outflow(pkg, orc, kind):
    """an inflowing phase delivers the captured 1/B, Rs and Rv, an outflowing one the interior's: with one phase mobile at a time, the ratio
    of the equations' contributions is Rs (oil phase) or Rv (gas phase, wet gas) of that side, and the own component's contribution is
    1/B of that side times the volume flux; gas-bearing and undersaturated cells are both among the faces"""
    case = make_case(pkg, kind)
    wet = kind == "wetgas"
    h = pkg.boundary.HostBoundary(lateral_free(pkg, case), case["depth"], case["fluid"])
    assert h.wet == wet
    h.initial_solution_applied(oracle_at(orc, case))
    captured = h.ext
    assert len(set(case["meaning"][h.cells].tolist())) >= 2            # saturated and undersaturated cells
    for sign in (-1.0, 1.0):                                            # pressure below the captured one: inflow; above: outflow
        rec = oracle_at(orc, case, moved(case, sign).reshape(-1)).iq()[h.cells]
        for ph in range(3):
            r1, x1 = only_phase(rec, captured, ph)
            h.ext = x1
            Q = h.rates(r1)[:, :3]
            assert np.all(h.composition[:, ph] == (1 if sign < 0 else -1)) and np.all(h.upwind_exterior[:, ph] == (sign < 0))
            own = Q[:, pkg.boundary.COMP[ph]]
            mob = x1["mob"][:, ph] if sign < 0 else r1[:, 9 + ph, 0]
            flows = mob > 0.0
            assert np.all((own < 0.0) == (flows & (sign < 0))) and np.all((own > 0.0) == (flows & (sign > 0)))   # positive out of the cell
            b = x1["b"][:, ph] if sign < 0 else r1[:, 6 + ph, 0]
            dp = (x1["p"][:, ph] - r1[:, 3 + ph, 0])                    # lateral faces: no gravity term
            tm = r1[:, 17, 0] if (wet and sign > 0) else 1.0
            np.testing.assert_allclose(own, b * (dp * mob * (-h.trans * tm / h.area)) * h.area, rtol=1e-13, atol=0.0)
            rs = x1["rs"] if sign < 0 else r1[:, 15, 0]
            rv = (x1["rv"] if sign < 0 else r1[:, 16, 0]) if wet else np.zeros(len(own))
            if ph == 1:
                np.testing.assert_allclose(Q[:, 2], rs * own, rtol=1e-14, atol=0.0)
                assert np.all(Q[:, 1] == 0.0) and np.any(flows) and np.any(rs[flows] > 0.0)
            elif ph == 2:
                np.testing.assert_allclose(Q[:, 0], rv * own, rtol=1e-14, atol=0.0)
                assert np.all(Q[:, 1] == 0.0) and (not wet or np.any(rv[flows] > 0.0))
            else:
                assert np.all(Q[:, 0] == 0.0) and np.all(Q[:, 2] == 0.0) and np.any(flows)
    h.ext = captured
    # the captured values differ from the moved interior's, so the two sides are told apart
    rec = oracle_at(orc, case, moved(case, -1.0).reshape(-1)).iq()[h.cells]
    assert np.all(rec[:, 7, 0] != captured["b"][:, 1])


def test_rate_faces(pkg, orc):
    """a RATE face: mass rate / reference density of the component times the area, no derivative, whatever the state"""
    B = pkg.boundary
    case = make_case(pkg, "blackoil")
    west = B.faces(case, (0, 0, 0, 2, 0, 1), "I-")
    rates = np.array([[1e-5 * (n + 1), -3e-4 * (n + 2), 2e-7 * n] for n in range(len(west["cells"]))])
    h = B.HostBoundary([B.rate(west, rates), B.free(B.faces(case, (0, 0, 0, 2, 0, 1), "J-"))], case["depth"], case["fluid"])
    h.initial_solution_applied(oracle_at(orc, case))
    Q = h.rates_now(oracle_at(orc, case, moved(case, 1.0).reshape(-1)))
    n = len(west["cells"])
    rho = np.array(case["fluid"].pvt[0]["density"])
    assert np.array_equal(Q[:n, :3], rates / rho * west["area"][:, None]) and np.all(Q[:n, 3:] == 0.0)
    assert np.all(Q[n:, :3] != 0.0)                                     # the FREE faces behind them are not disturbed
    # handed to a model with whole-array hooks: the caller's source minus the rates, a cell with two faces one after the other
    class Whole:
        def iq(self_):
            return o.iq()
        def set_source(self_, s, d):
            self_.s, self_.d = s.reshape(-1, 3), d.reshape(-1, 9)
    o = oracle_at(orc, case, moved(case, 1.0).reshape(-1))
    base = np.full((case["Nb"], 3), 1e-3)
    h2 = B.HostBoundary(h_records(B, case, rates), case["depth"], case["fluid"], base_source=base)
    h2.initial_solution_applied(oracle_at(orc, case))
    w = Whole()
    h2.add_to_source(w)
    want = base.copy()
    for f, c in enumerate(h2.cells):
        want[c] = want[c] - h2.Q[f, :3]
    assert np.array_equal(w.s, want) and np.count_nonzero(w.d) > 0 and np.array_equal(w.s[5], base[5])


def h_records(B, case, rates):
    return [B.rate(B.faces(case, (0, 0, 0, 2, 0, 1), "I-"), rates), B.free(B.faces(case, (0, 0, 0, 2, 0, 1), "J-"))]

"""Synthetic black-oil cases in the form the hot path consumes (arrays, SI units): what Flow's deck-side setup
(EclProblem / EclTransmissibility / equilibration, all outside the hot path) would hand to the assembly.

Recipes follow SURVEY.md §8(d): Cartesian nx x ny x nz, DX = DY = 20 m, DZ = 5 m, tops at 2500 m, PORO 0.25,
PERM 100 mD (homogeneous) or log-normal exp(N(ln 100, 1)) with rng(12345); SPE1 fluid; hydrostatic initial state,
p = 250 bar at the top, Sw = 0.2 and either Sg = 0 with Rs = 0.8 RsSat(p) ("undersaturated") or Sg = 0.1
("saturated"), perturbed with rng(2024) by +-1 % on p and +-0.02 on the saturations.
"""
import numpy as np

from . import fluid as _fluid
from . import grid as _grid

MILLIDARCY = 9.869232667160130e-16
SW_PO_SG, SW_PO_RS = 0, 1  # PrimaryVariables::PrimaryVarsMeaning


def rs_sat(fl, p, region=0):
    """Saturated Rs(p) of the PVTO table (piecewise linear in the bubble-point pressures, linear extrapolation)."""
    nodes = fl.pvt[region]["pvto"]
    xp = np.array([n["p"][0] for n in nodes])
    fp = np.array([n["rs"] for n in nodes])
    p = np.asarray(p, float)
    s = np.clip(np.searchsorted(xp, p, side="right") - 1, 0, len(xp) - 2)
    return fp[s] + (fp[s + 1] - fp[s]) * (p - xp[s]) / (xp[s + 1] - xp[s])


def cartesian_cells(nx, ny, nz, dx=20.0, dy=20.0, dz=5.0, top=2500.0, poro=0.25, perm_md=100.0, heterogeneous=False,
                    state="undersaturated", perturb=True, fluid=None, seed_state=2024):
    """Per-cell arrays of the synthetic case (no connectivity): geometry, rock and the initial state."""
    fl = fluid if fluid is not None else _fluid.spe1_fluid()[0]
    Nb = nx * ny * nz
    if heterogeneous:
        perm = np.exp(np.random.default_rng(12345).normal(np.log(perm_md), 1.0, Nb)) * MILLIDARCY
    else:
        perm = np.full(Nb, perm_md * MILLIDARCY)
    k = np.arange(Nb) // (nx * ny)
    volume = np.full(Nb, dx * dy * dz)
    depth = top + (k + 0.5) * dz
    rng = np.random.default_rng(seed_state)
    p = 250e5 + 7000.0 * (depth - top)
    sw = np.full(Nb, 0.2)
    if perturb:
        p = p * (1.0 + rng.uniform(-0.01, 0.01, Nb))
        sw = sw + rng.uniform(-0.02, 0.02, Nb)
    pv = np.zeros((Nb, 3))
    pv[:, 0], pv[:, 1] = sw, p
    if state == "undersaturated":
        meaning = np.full(Nb, SW_PO_RS, np.uint8)
        pv[:, 2] = 0.8 * rs_sat(fl, p)
    elif state == "saturated":
        meaning = np.full(Nb, SW_PO_SG, np.uint8)
        pv[:, 2] = 0.1 + (rng.uniform(-0.02, 0.02, Nb) if perturb else 0.0)
    elif state == "mixed":  # both meanings in one grid: gas cap in the upper half
        meaning = np.where(depth < np.median(depth), SW_PO_SG, SW_PO_RS).astype(np.uint8)
        pv[:, 2] = np.where(meaning == SW_PO_SG, 0.1 + (rng.uniform(-0.02, 0.02, Nb) if perturb else 0.0),
                            0.8 * rs_sat(fl, p))
    else:
        raise ValueError(state)
    return dict(Nb=Nb, nx=nx, ny=ny, nz=nz, dx=dx, dy=dy, dz=dz, top=top, perm=perm, poro=np.full(Nb, float(poro)),
                volume=volume, depth=np.ascontiguousarray(depth), fluid=fl, pv=np.ascontiguousarray(pv.reshape(-1)), meaning=meaning)


def cartesian_case(nx, ny, nz, dx=20.0, dy=20.0, dz=5.0, top=2500.0, poro=0.25, perm_md=100.0, heterogeneous=False,
                   state="undersaturated", perturb=True, fluid=None, seed_state=2024):
    c = cartesian_cells(nx, ny, nz, dx, dy, dz, top, poro, perm_md, heterogeneous, state, perturb, fluid, seed_state)
    pat = _grid.cartesian_pattern(nx, ny, nz)
    _, _, area = _grid.cartesian_geometry(pat, dx, dy, dz, top)
    trans = _grid.tpfa_transmissibility(pat, c["perm"], c["perm"], c["perm"], dx, dy, dz)
    return dict(Nb=c["Nb"], nx=nx, ny=ny, nz=nz, rowptr=pat["rowptr"], col=pat["col"], face_dir=pat["face_dir"],
                trans=np.ascontiguousarray(trans), area=np.ascontiguousarray(area), poro=c["poro"],
                volume=np.ascontiguousarray(c["volume"]), depth=c["depth"], fluid=c["fluid"], pv=c["pv"], meaning=c["meaning"],
                perm=c["perm"], dx=dx, dy=dy, dz=dz)


def with_well_cliques(case, wells):
    """The case on the pattern that also holds a block for every pair of one well's perforated cells (grid.with_well_cliques): what the
    matrix-add form of the resident wells writes into (wells.DeviceStandardWells(matrix_add=True)).  wells: wells.Well objects (or anything
    with .cells), a wells.StandardWells, or plain lists of cells.
    For the assembly a clique entry is a face with transmissibility zero: trans and thpres (where the case has it) are 0 there, so the flux
    and all its derivatives vanish and the Jacobian's clique blocks are zero until the wells are added.  area is 1.0 there - the flux
    divides by the face area, and an area of 0 would make 0 / 0 - and face_dir is grid.CLIQUE_FACE (no direction).  Every per-cell array
    is shared with `case`.
    A row may hold at most 64 blocks (the assembly tile; opmhip_set_static refuses longer rows): the row of a perforated cell holds its
    stencil and the well's other cells that are not in the stencil already - see DESIGN.md section 5 for what that allows."""
    lists = [np.asarray(getattr(w, "cells", w), np.int64) for w in getattr(wells, "wells", wells)]
    pat, old_pos = _grid.with_well_cliques(dict(Nb=case["Nb"], rowptr=case["rowptr"], col=case["col"], face_dir=case.get("face_dir")), lists)
    n = len(pat["col"])
    out = dict(case)
    out.update(rowptr=pat["rowptr"], col=pat["col"])
    if case.get("face_dir") is not None:
        out["face_dir"] = pat["face_dir"]
    for key, fill in (("trans", 0.0), ("thpres", 0.0), ("area", 1.0)):
        if case.get(key) is not None:
            v = np.full(n, fill)
            v[old_pos] = case[key]
            out[key] = v
    return out


def spe1_case(props=None, state="equil"):
    """The SPE1CASE1 deck (python/test_data/SPE1CASE1/SPE1CASE1.DATA; FIELD units converted to SI in data/spe1_fluid.json): its grid
    (10 x 10 x 3, layered DZ / PERM, :64-108), its PROPS (:109-250) and, state = "equil", its SOLUTION section (:252-290) - EQUIL 8400 ft /
    4800 psia, contacts outside the reservoir, RSVD 1.27 Mscf/stb - equilibrated by equil.equilibrate (initstateequil.hh's algorithm, held
    by the twelve decks of tests/test_equil.cc) on top of `props`: an object with probe(p, rs, sw, sg) - capi.HipFluid(fluid), the DEVICE's
    property functions (the default: a GPU is needed), or the oracle's in CPU tests.  The case carries the SCHEDULE section's DRSDT 0
    ("drsdt", "drsdt_all_cells": the Rs cap of eclproblem.hh:1711-1732 with the keyword's option ALL - every cell's Rs is held at its value
    of the last accepted step, :2053-2070) and, under "schedule", its wells and report steps (spe1_wells builds the well model).
    state = "rough" (no props needed): a constant oil gradient from the datum pressure, Sw = connate, Rs = the RSVD value - a plausible
    undersaturated state for tests that only need one."""
    fl, d = _fluid.spe1_fluid()
    g = d["grid"]
    nx, ny, nz = g["nx"], g["ny"], g["nz"]
    pat = _grid.cartesian_pattern(nx, ny, nz)
    Nb = pat["Nb"]
    k = np.arange(Nb) // (nx * ny)
    dzs = np.array(g["dz"])
    dz = dzs[k]
    ztop = g["tops"] + np.concatenate([[0.0], np.cumsum(dzs)[:-1]])[k]
    depth = ztop + 0.5 * dz
    volume = g["dx"] * g["dy"] * dz
    perm = np.array(g["perm"])[k]
    fd = np.abs(pat["face_dir"].astype(int))
    row = _grid.row_of_entries(pat["rowptr"])
    col = pat["col"]
    area = np.zeros(len(col))
    area[fd == 1] = (g["dy"] * dz[row])[fd == 1]
    area[fd == 2] = (g["dx"] * dz[row])[fd == 2]
    area[fd == 3] = g["dx"] * g["dy"]
    # half transmissibilities with per-cell DZ (ebos/ecltransmissibility.cc:928-944), harmonic combination (:352-356)
    T = np.zeros(len(col))
    for dnum, h_of, a_of in ((1, lambda c: np.full(len(c), g["dx"]), lambda c: g["dy"] * dz[c]),
                             (2, lambda c: np.full(len(c), g["dy"]), lambda c: g["dx"] * dz[c]),
                             (3, lambda c: dz[c], lambda c: np.full(len(c), g["dx"] * g["dy"]))):
        m = fd == dnum
        half = lambda c: perm[c] * a_of(c) * (h_of(c) / 2.0) / (h_of(c) / 2.0) ** 2
        t1, t2 = half(row[m]), half(col[m])
        T[m] = 1.0 / (1.0 / t1 + 1.0 / t2)
    e = d["equil"]
    pv = np.zeros((Nb, 3))
    meaning = np.full(Nb, SW_PO_RS, np.uint8)
    if state == "rough":
        rho_o = d["density"]["oil"] * 0.78  # rough reservoir oil gradient; the state only has to be plausible
        pv[:, 0] = d["swof"][0][0]
        pv[:, 1] = e["datum_pressure"] + rho_o * 9.80665 * (depth - e["datum_depth"])
        pv[:, 2] = d["rsvd"][0][1]
    else:
        from . import equil as _equil
        if props is None:
            from . import capi as _capi
            props = _capi.HipFluid(fl)           # the device's fluid and saturation functions (raises without a GPU: no CPU fallback)
        rec = dict(datum=e["datum_depth"], pressure=e["datum_pressure"], zwoc=e["woc"], pcow_woc=0.0, zgoc=e["goc"], pcgo_goc=0.0)
        rsvd = np.array(d["rsvd"])
        limits = dict(Swl=d["swof"][0][0], Swu=d["swof"][-1][0], Sgl=d["sgof"][0][0], Sgu=d["sgof"][-1][0])
        rho = (d["density"]["oil"], d["density"]["water"], d["density"]["gas"])
        # one equilibration per layer (cells of a layer share their centre depth), spread over the layer's cells
        zc = g["tops"] + np.concatenate([[0.0], np.cumsum(dzs)[:-1]]) + 0.5 * dzs
        r = _equil.equilibrate(props, rho, rec, zc, (g["tops"], g["tops"] + float(dzs.sum())), limits,
                               rs_func=_equil.RsVD(props, rsvd[:, 0], rsvd[:, 1]))
        sg = r["sg"][k]
        pv[:, 0] = r["sw"][k]
        pv[:, 1] = r["po"][k]
        pv[:, 2] = np.where(sg > 0.0, sg, r["rs"][k])
        meaning = np.where(sg > 0.0, SW_PO_SG, SW_PO_RS).astype(np.uint8)
    sched = d.get("schedule", {})
    return dict(Nb=Nb, nx=nx, ny=ny, nz=nz, rowptr=pat["rowptr"], col=col, face_dir=pat["face_dir"],
                trans=np.ascontiguousarray(T), area=np.ascontiguousarray(area), poro=np.full(Nb, g["poro"]),
                volume=np.ascontiguousarray(volume), depth=np.ascontiguousarray(depth), fluid=fl,
                pv=np.ascontiguousarray(pv.reshape(-1)), meaning=meaning, perm=perm, dx=g["dx"], dy=g["dy"], dz_cell=dz,
                drsdt=[sched["drsdt"]] if "drsdt" in sched else None,
                drsdt_all_cells=[1 if sched.get("drsdt_option", "ALL") == "ALL" else 0] if "drsdt" in sched else None, schedule=sched)


def spe1_wells(case):
    """The deck's two wells (SPE1CASE1.DATA:383-425) as a wells.StandardWells: INJ, gas at a surface rate of 100 MMscf/day into (1, 1, 1),
    BHP limit 9014 psia; PROD, 20 000 stb/day of oil out of (10, 10, 3), BHP limit 1000 psia; connection factors by Peaceman's formula from
    the cell's permeability and the wellbore diameter (COMPDAT item 9)"""
    from . import wells as _wells
    nx, ny = case["nx"], case["ny"]
    out = []
    for w in case["schedule"]["wells"]:
        cells = [w["i"] + nx * (w["j"] + ny * kk) for kk in range(w["k_upper"], w["k_lower"] + 1)]
        tw = [_wells.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz_cell"][c], w["diameter"]) for c in cells]
        if w["kind"] == "producer":
            ctl = ("rate", _wells.OIL, w["oil_rate"])
            out.append(_wells.Well(w["name"], cells, tw, w["ref_depth"], True, ctl, w["bhp_limit"]))
        else:
            comp = {"gas": _wells.GAS, "water": _wells.WATER, "oil": _wells.OIL}[w["injected"]]
            out.append(_wells.Well(w["name"], cells, tw, w["ref_depth"], False, ("rate", comp, w["surface_rate"]), w["bhp_limit"], inj_phase=w["injected"]))
    return _wells.StandardWells(out, case["depth"])


STB_PER_DAY = 0.158987294928 / 86400.0
PSIA = 6894.757293168361
# (i, j), one-based, of SPE9's 25 producers in the order of the public deck's COMPDAT (the deck is not in the reference tree: a stand-in
# that completes its wells where the comparative-solution project does)
SPE9_PRODUCERS_IJ = [(5, 1), (8, 2), (11, 3), (10, 4), (12, 5), (4, 6), (8, 7), (14, 8), (11, 9), (12, 10), (10, 11), (5, 12), (8, 13),
                     (11, 14), (13, 15), (15, 16), (11, 17), (12, 18), (5, 19), (8, 20), (11, 21), (15, 22), (12, 23), (10, 24), (17, 25)]


def spe9_shaped_wells(case, oil_rate_stb_day=1500.0, water_rate_stb_day=5000.0, producer_bhp_limit=1000.0 * PSIA, injector_bhp_limit=400e5,
                      diameter=0.1524, liquid_rate_stb_day=None, resv_rate=None, groups=None):
    """BASELINE.json configs[2] with wells that are wells (wells.StandardWells) on a 24 x 25 x 15 cartesian_case: SPE9's water injector at
    (24, 25), completed in layers 11-15, on a surface-rate target with an upper BHP limit, and its 25 oil producers, completed in layers
    2-4, on an oil-rate target (1500 stb/day; the SPE9 schedule cuts it to 100 stb/day for a while) with a lower BHP limit of 1000 psia;
    reference depth = the centre of the topmost completion; connection factors by Peaceman's formula from the cell's own permeability,
    so that on the log-normal field some producers cannot hold their target and fall to the BHP limit.  A stand-in like the grid itself:
    the SPE9 deck is not in the reference tree, its fluid and its dipping layers are not reproduced.
    liquid_rate_stb_day / resv_rate (reservoir m^3/s): every producer also gets an LRAT / a RESV limit (wells.Well(limits=)); a RESV limit
    needs the fluid's property functions: build wells.StandardWells(.wells, depth, props=, volume=) from the list returned.
    groups (default None: the list as it was): dict(count=, kind="lrat" | "orat", target_stb_day=[, guide_rate=1.0, nupcol=]) - the 25
    producers go into `count` production groups, producer n into group n % count (a group's wells are interleaved in list order), every
    group with that one target (per group where target_stb_day is a sequence) and mode "none"; the injector stays under FIELD."""
    from . import wells as _wells
    nx, ny, nz = case["nx"], case["ny"], case["nz"]
    if (nx, ny) != (24, 25) or nz < 15:
        raise ValueError("spe9_shaped_wells: a 24 x 25 x 15 grid is expected")
    def column(i, j, k0, k1):
        cells = [(i - 1) + nx * ((j - 1) + ny * k) for k in range(k0 - 1, k1)]
        tw = [_wells.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], diameter) for c in cells]
        return cells, tw
    cells, tw = column(24, 25, 11, 15)
    out = [_wells.Well("INJE1", cells, tw, case["depth"][cells[0]], False, ("rate", _wells.WATER, water_rate_stb_day * STB_PER_DAY), injector_bhp_limit,
                       inj_phase="water")]
    for n, (i, j) in enumerate(SPE9_PRODUCERS_IJ):
        cells, tw = column(i, j, 2, 4)
        limits = {}
        if liquid_rate_stb_day is not None:
            limits["lrat"] = liquid_rate_stb_day * STB_PER_DAY
        if resv_rate is not None:
            limits["resv"] = resv_rate
        out.append(_wells.Well("PRODU%d" % (n + 2), cells, tw, case["depth"][cells[0]], True, ("rate", _wells.OIL, oil_rate_stb_day * STB_PER_DAY), producer_bhp_limit,
                               **({"limits": limits} if limits else {})))
    if groups is not None:
        count, kind = int(groups["count"]), groups.get("kind", "lrat")
        if count < 1 or kind not in ("lrat", "orat"):
            raise ValueError("spe9_shaped_wells: groups needs count >= 1 and kind 'lrat' or 'orat'")
        targets = np.broadcast_to(np.asarray(groups["target_stb_day"], float), (count,))
        for n, w in enumerate(out[1:]):
            w.group, w.guide_rate = n % count, np.full(5, float(groups.get("guide_rate", 1.0)))
        glist = [_wells.Group("G%d" % (g + 1), {kind: targets[g] * STB_PER_DAY}) for g in range(count)]
        return _wells.StandardWells(out, case["depth"], groups=glist, nupcol=groups.get("nupcol", _wells.NUPCOL_DEFAULT))
    return _wells.StandardWells(out, case["depth"])


def gas_condensate_wells(case, allow_crossflow=False, oil_rate=40.0 / 86400.0, gas_rate=4000.0 / 86400.0, orat=0.1 / 86400.0, injection_rate=5000.0 / 86400.0,
                         scale=0.2, diameter=0.15, limits=None, thp_limit=None, vfp_table=None):
    """Three wells that share no cell on a column grid whose top is a gas cap holding vaporised oil (tests/helpers.py wetgas_case: gas cap,
    three-phase zone, oil leg; nx, ny >= 3), as a list of wells.Well for wells.StandardWells / DeviceStandardWells(vaporised_oil=):
      PLONG  a producer through every layer of column (0, 0) on an oil-rate target; its connection factors are scaled down (scale) so that
             its drawdown is of the size of the pressure scatter of the synthetic cases: solved alone it keeps a few reversed perforations
             in all three zones; allow_crossflow, limits (wells.Well(limits=)) and thp_limit / vfp_table are this well's;
      PCAP   a producer of one completion in the gas cap, column (nx - 1, ny - 1) in the second layer, on a gas-rate target (GRAT) with an
             ORAT limit: all its oil is the oil its gas carries, so the limit binds under the wet-gas rate model and never under the default;
      GINJ   a gas injector into the top five layers of column (nx - 1, 0).
    Surface rates in m^3/s; reference depth = the centre of the topmost completion; connection factors by Peaceman's formula."""
    from . import wells as _wells
    nx, ny, nz = case["nx"], case["ny"], case["nz"]
    if nx < 3 or ny < 3 or nz < 6:
        raise ValueError("gas_condensate_wells: at least 3 x 3 x 6 cells are expected")

    def well(name, i, j, ks, producer, control, bhp_limit, factor=1.0, **kw):
        cells = [i + nx * (j + ny * k) for k in ks]
        tw = [factor * _wells.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], diameter) for c in cells]
        return _wells.Well(name, cells, tw, case["depth"][cells[0]], producer, control, bhp_limit, **kw)
    long_kw = dict(allow_crossflow=allow_crossflow, limits=limits)
    if thp_limit is not None:
        long_kw.update(thp_limit=thp_limit, vfp_table=vfp_table)
    return [well("PLONG", 0, 0, range(nz), True, ("rate", _wells.OIL, oil_rate), 200e5, scale, **long_kw),
            well("PCAP", nx - 1, ny - 1, [1], True, ("rate", _wells.GAS, gas_rate), 200e5, limits={"orat": orat}),
            well("GINJ", nx - 1, 0, range(5), False, ("rate", _wells.GAS, injection_rate), 400e5, inj_phase="gas")]


# Field rate of the five-spot pair on a 100 x 100 x 100 grid (scaled with the areal cell count elsewhere): 0.4 % of a well
# cell's pore volume per day.  Fixed-rate sources do not see the mobility of the cell they drain, so rates ten times
# higher desaturate the producer column within weeks and the Newton method then fails on 10-day steps.
BENCH_RATE_SM3_PER_DAY = 200.0


def five_spot_source(case, rate_sm3_per_day=50.0):
    """Fixed-rate source terms (surface m^3/s per cell, equations oil/water/gas): water injected in one corner
    column, the same surface volume of oil (+ its dissolved gas at the initial Rs) produced in the opposite one."""
    Nb, nx, ny, nz = case["Nb"], case["nx"], case["ny"], case["nz"]
    src = np.zeros((Nb, 3))
    q = rate_sm3_per_day / 86400.0 / nz
    for k in range(nz):
        inj = 0 + nx * (0 + ny * k)
        prod = (nx - 1) + nx * ((ny - 1) + ny * k)
        src[inj, 1] += q
        src[prod, 0] -= q
        rs = case["pv"][3 * prod + 2] if case["meaning"][prod] == SW_PO_RS else float(rs_sat(case["fluid"], case["pv"][3 * prod + 1]))
        src[prod, 2] -= q * rs
    return np.ascontiguousarray(src.reshape(-1))


def two_aquifers(case, grid, dims):
    """A Carter-Tracy aquifer on the I- side and a Fetkovich aquifer under the grid (records for capi.HipModel.set_aquifers /
    aquifers.HostAquifers), sized for a measurement rather than for a field: both equilibrate with the reservoir.  grid, dims: what
    transmissibility.cornerpoint_faces / cartesian_faces gave for `case` (the Norne-shaped case of the tests), or None, None for a
    cartesian_case.  The influence table has the shape of a radial infinite-acting aquifer's (AQUTAB's default lives in opm-common)."""
    from . import aquifers as _aq
    g = case if grid is None else (grid, dims)
    nx, ny, nz = (case["nx"], case["ny"], case["nz"]) if grid is None else dims
    depth = np.asarray(case["depth"])
    side = _aq.connections(g, (0, nx - 1, 0, ny - 1, 0, nz - 1), "I-")
    under = _aq.connections(g, (0, nx - 1, 0, ny - 1, 0, nz - 1), "K+")
    keep = lambda c: dict(cells=c["cells"][c["alpha"] > 0.0], alpha=c["alpha"][c["alpha"] > 0.0])   # a cell without the face carries no influx
    side, under = keep(side), keep(under)
    td = [0.01, 0.05, 0.1, 0.5, 1.0, 5.0, 10.0, 50.0, 100.0]
    pd = [0.112, 0.229, 0.315, 0.616, 0.802, 1.362, 1.651, 2.388, 2.723]   # concave and ascending, as such a table is; the values UNVERIFIED
    datum = float(depth.max())
    return [_aq.carter_tracy(1, side, time_constant=200.0 * 86400.0, influx_constant=2.0e-4, water_density=1000.0, datum_depth=datum, td=td, pd=pd),
            _aq.fetkovich(2, under, time_constant=_aq.fetkovich_time_constant(1.0e-9, 2.0e10, 5.0e-8), prod_index=5.0e-8, total_compr=1.0e-9, initial_watvolume=2.0e10,
                          water_density=1000.0, datum_depth=datum)]


def write_case_binary(case, path, source=None):
    """Case file for the C++ host driver (opm-autodiff_amd/host/test_BlackoilModelHip.cpp): named raw arrays."""
    import struct
    fl = case["fluid"]
    arrs = {k: case[k] for k in ("rowptr", "col", "trans", "area", "poro", "volume", "depth", "pv", "meaning")}
    arrs.update(fl.arrays)
    arrs["fluid_hdr"] = np.array([len(fl.pvt), len(fl.sat)], np.int32)
    arrs["rock"] = np.array([fl.rock_pref, fl.rock_cr], np.float64)
    if source is not None:
        arrs["source"] = np.asarray(source, np.float64)
    code = {np.dtype(np.int32): 0, np.dtype(np.float64): 1, np.dtype(np.uint8): 2}
    with open(path, "wb") as f:
        f.write(b"OPMHIPCASE1\0")
        for name, a in arrs.items():
            a = np.ascontiguousarray(a)
            if a.dtype == np.int64:
                a = a.astype(np.int32)
            nb = name.encode()
            f.write(struct.pack("<I", len(nb)) + nb + struct.pack("<BQ", code[a.dtype], a.size))
            f.write(a.tobytes())

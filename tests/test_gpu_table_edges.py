"""The property-table lookups of the per-cell kernels on their nodes, ends and thresholds, and with tables on either side of the
LDS budget.  The states are the labelled ones of tests/table_states.py, one per cell of an N x 1 x 1 grid; the CPU side of every
statement here is in tests/test_table_states.py.

Part 1 - per fluid (SPE1, its two-region variant, wet gas + ROCKTAB, the two-row tables, uneven PVTO columns, two equal bubble
points): iq(), Jacobian and residual, the three probes bit for bit the oracle's; the device against the exact statement within the
bound measured for the oracle; the samples themselves on the nodes; three Newton updates (a small fixed step, twice that step back -
every member of a triple crosses its node in one of the two - and a large seeded one) with state, meanings, switch count and iq()
the oracle's.

Part 2 - k_iq_update / k_newton_update copy the double blob into LDS up to TAB_LDS_DBL = 3072 doubles and read it in global memory
beyond: paddings of SPE1 to exactly 3072 and 3073 doubles, and of the two-region fluid to 100 saturation regions (14 174 doubles),
the padding behind the regions in use (same numbers, larger blob), in front of them (every offset large), and with every region in
use; the 3073 case once more in the extended layout.  Where the padding is in front, the other readers of the blob in global memory
- the hysteresis update, the scaled saturation functions, the well-bore density of a resident well - against the unpadded fluid."""
import numpy as np
import pytest

import helpers
import oracle_bind
import table_states as ts

pytestmark = pytest.mark.gpu
DT = 86400.0


@pytest.fixture(scope="module")
def fluids(pkg):
    return ts.edge_fluids(pkg)


def same(got, want, what, nan=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want, equal_nan=nan):
        g, w = got.reshape(-1), want.reshape(-1)
        bad = np.flatnonzero(~((g == w) | (nan & np.isnan(g) & np.isnan(w))))
        raise AssertionError((what, bad.size, bad[:6], g[bad[:6]], w[bad[:6]]))


def two(pkg, orc, case):
    m = pkg.capi.HipModel(case)
    o = oracle_bind.OracleModel(orc, case)
    for q in (m, o):
        q.set_state(case["pv"], case["meaning"])
    return m, o


def steps_of(rows, seed=3):
    """the three update vectors: +d, -2 d, and a large seeded one (every chop and switch rule fires)"""
    N = len(rows)
    d = np.tile(np.array([1e-12, 1e-3, 1e-12]), (N, 1))
    big = np.random.default_rng(seed).standard_normal((N, 3)) * np.array([0.3, 3e6, 0.3])
    return [d.reshape(-1), (-2.0 * d).reshape(-1), big.reshape(-1)]


def updates_agree(sides, dxs, nan=False):
    """the same updates on every side (a capi.HipModel or an oracle_bind.OracleModel each): switch counts, states, meanings and
    records equal to the first side's after each; -> how many cells changed their meaning in all"""
    changed = 0
    for k, dx in enumerate(dxs):
        before = sides[0].get_state()[1].copy()
        n = [q.update(dx, 1.0) if hasattr(q, "Nloc") else q.update(dx) for q in sides]
        st = [q.get_state() for q in sides]
        for i in range(1, len(sides)):
            assert n[i] == n[0], (k, n)
            same(st[i][1], st[0][1], ("meaning", k, i))
            same(st[i][0], st[0][0], ("state", k, i), nan)
            same(sides[i].iq(), sides[0].iq(), ("iq after update", k, i), nan)
        changed += int((st[0][1] != before).sum())
    return changed


# ---- part 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.EDGE_FLUIDS)
def test_edge_states(pkg, orc, fluids, name):
    e = ts.edge_states(pkg, name, fluids)
    nan = name == "equal_bubble_point"
    case, rows, fl = e["case"], e["rows"], e["fluid"]
    m, o = two(pkg, orc, case)
    iq = m.iq()
    assert iq.shape[1] == (19 if name in ("wet_rocktab", "two_row") else 17)
    same(iq, o.iq(), "iq", nan)
    jm, rm = m.assemble(DT, 0)
    jo, ro = o.assemble(DT, 0)
    same(rm, ro, "residual", nan)
    same(jm, jo, "jacobian", nan)
    assert nan or (np.isfinite(iq).all() and np.isfinite(jm).all() and np.isfinite(rm).all())
    # the probes at the same states
    dev, ora = pkg.capi.HipFluid(fl), oracle_bind.OracleFluid(orc, fl)
    p, rs, sw, sg = ts.probe_arguments(rows)
    with np.errstate(all="ignore"):
        pd, po = (q.probe(p, rs, sw, sg, pvt_region=e["pvt"], sat_region=e["sat"]) for q in (dev, ora))
        sd, so = (q.sat_probe(sw, sg, sat_region=e["sat"]) for q in (dev, ora))
        rv = np.where(rows[:, 3] == ts.SW_PG_RV, rows[:, 2], 0.0)
        gd, go = (q.probe_gas(p, rv, pvt_region=e["pvt"]) for q in (dev, ora))
    same(pd, po, "fluid_probe", nan)
    same(sd, so, "sat_probe", nan)
    same(gd, go, "probe_gas", nan)
    # the device against the exact statement, within the oracle's measured distance x 4
    e["exact"] = ts.exact(fl, rows, e["extras"])
    for what, (d, where) in zip(("probe", "sat_probe", "cache"), ts.distances(e, pd, sd, iq)):
        print("%-20s %-10s %.3e  %s" % (name, what, d, e["labels"][where[0]] if where else ""))
        assert d <= ts.BOUND, (what, d, where, e["labels"][where[0]])
    # on the nodes: the samples themselves
    if not nan:
        ng, no, wrong = ts.on_node_checks(e, pd, last=False)
        assert not wrong and no >= 8 and (ng >= 8 or name == "wet_rocktab"), wrong[:4]
        pair = np.array([l.startswith("pair:") for l in e["labels"]])
        same(iq[pair, 7, 0], pd[pair, 2], "1/Bo of the cache on (Rs node, sample)")
        ng, nw, wrong = ts.node_slope_checks(e, iq)        # the derivatives there: those of the stated segment
        assert not wrong and (name == "two_row" or (nw >= 8 and (ng >= 8 or name == "wet_rocktab"))), (ng, nw, wrong[:4])
    # three updates
    changed = updates_agree([m, o], steps_of(rows), nan)
    assert changed >= 8


@pytest.mark.parametrize("name", ["spe1", "two_region", "two_row", "uneven_columns"])
def test_on_the_last_node_the_device_returns_the_sample(pkg, fluids, name):
    """the last node is the right end of the last segment: the lookup returns the sample itself there (SPE1's PVDG: the interpolation
    formula would miss it by an ulp), as tests/test_table_states.py holds the oracle to"""
    e = ts.edge_states(pkg, name, fluids)
    p, rs, sw, sg = ts.probe_arguments(e["rows"])
    pd = pkg.capi.HipFluid(e["fluid"]).probe(p, rs, sw, sg, pvt_region=e["pvt"], sat_region=e["sat"])
    ng, _, wrong = ts.on_node_checks(e, pd, last=True)
    assert ng >= 8
    assert not wrong, wrong[:4]


# ---- part 2 ------------------------------------------------------------------------------------------------------------------------
PADDINGS = {"3072": ("spe1_3072_%s", "spe1"), "3073": ("spe1_3073_%s", "spe1"), "norne_sized": ("norne_sized_%s", "two_region"),
            "3073_extended": ("wet_rocktab_3073_%s", "wet_rocktab")}


def padded_pair(pkg, fluids, size, where):
    """-> (padded fluid, unpadded fluid, the labelled states of the unpadded fluid's last PVT and saturation region, (PVT, saturation)
    region of those curves in the padded fluid, the same in the unpadded one)"""
    key, base = PADDINGS[size]
    big, small = fluids[key % where][0], fluids[base][0]
    n = ts.blob_doubles(big)
    assert (n == ts.TAB_LDS_DBL) if size == "3072" else (n == ts.TAB_LDS_DBL + 1) if size.startswith("3073") else (n > 10000 and len(big.sat) >= 100 and len(big.pvt) == 2)
    ps, ss = len(small.pvt) - 1, len(small.sat) - 1
    st = ts.states(small, ps, ss)
    if where == "after":
        return big, small, st, (ps, ss), (ps, ss)
    return big, small, st, (len(big.pvt) - 1, len(big.sat) - 1), (ps, ss)


def padded_against_unpadded(pkg, orc, fluids, size, where):
    big, small, (rows, labels, extras), (pr, sr), (ps, ss) = padded_pair(pkg, fluids, size, where)
    here = rows.copy()
    here[:, 4], here[:, 5] = pr, sr
    cb, cs = ts.case_of(pkg, big, here, extras), ts.case_of(pkg, small, rows, extras)
    mb, ob = two(pkg, orc, cb)
    msm = pkg.capi.HipModel(cs)
    msm.set_state(cs["pv"], cs["meaning"])
    assert mb.iq().shape[1] == (19 if size == "3073_extended" else 17)
    same(mb.iq(), ob.iq(), "iq, oracle")
    same(mb.iq(), msm.iq(), "iq, unpadded")
    jb, rb = mb.assemble(DT, 0)
    jo, ro = ob.assemble(DT, 0)
    js, rs_ = msm.assemble(DT, 0)
    same(rb, ro, "residual, oracle")
    same(jb, jo, "jacobian, oracle")
    same(rb, rs_, "residual, unpadded")
    same(jb, js, "jacobian, unpadded")
    cvb, cvs, cvo = mb.convergence(DT), msm.convergence(DT), ob.convergence(DT)
    same(cvb, cvs, "convergence, unpadded")
    np.testing.assert_allclose(cvb[11:17], cvo[11:17], rtol=1e-9, atol=1e-14)      # (the sums are formed in another order on the CPU)
    assert updates_agree([mb, ob, msm], steps_of(rows)) >= 8
    same(mb.convergence(DT), msm.convergence(DT), "convergence after the updates, unpadded")
    return big, small, pr, sr


@pytest.mark.parametrize("size", ["3072", "3073", "norne_sized"])
def test_unused_padding_behind(pkg, orc, fluids, size):
    """the cells keep region 0: a larger blob, the same offsets"""
    padded_against_unpadded(pkg, orc, fluids, size, "after")


@pytest.mark.parametrize("size", ["3072", "3073", "norne_sized", "3073_extended"])
def test_unused_padding_in_front(pkg, orc, fluids, size):
    """the cells use the last PVT and the last saturation region: the same curves behind offsets in the thousands"""
    big, small, pr, sr = padded_against_unpadded(pkg, orc, fluids, size, "before")
    assert pr == len(big.pvt) - 1 and sr == len(big.sat) - 1 >= 17


@pytest.mark.parametrize("size", ["3073", "norne_sized"])
def test_other_readers_of_a_blob_in_global_memory(pkg, orc, fluids, size):
    """padding in front: the scaled saturation functions, the probes and the well-bore density of a resident well in the last
    regions give what the unpadded fluid gives in region 0"""
    big, small, (rows, labels, extras), (pr, sr), (ps, ss) = padded_pair(pkg, fluids, size, "before")
    db, ds = pkg.capi.HipFluid(big), pkg.capi.HipFluid(small)
    p, rs, sw, sg = ts.probe_arguments(rows)
    same(db.probe(p, rs, sw, sg, pvt_region=pr, sat_region=sr), ds.probe(p, rs, sw, sg, pvt_region=ps, sat_region=ss), "fluid_probe")
    same(db.probe_gas(p, 0.0, pvt_region=pr), ds.probe_gas(p, 0.0, pvt_region=ps), "probe_gas")
    same(db.sat_probe(sw, sg, sat_region=sr), ds.sat_probe(sw, sg, sat_region=ss), "sat_probe")
    u = ds.sat_end_points(ss)
    assert db.sat_end_points(sr) == u
    for three in (0, 1):
        es = dict(sat_scaling=1, three_point_kr=three, krw=2, kro=2, krg=2, pcw=1, pcg=1, swl=u["swl"] + 0.03, swcr=u["swcr"] + 0.05, sgcr=u["sgcr"] + 0.02,
                  sowcr=u["sowcr"] + 0.04, sogcr=u["sogcr"] + 0.03, max_krw=0.8 * u["max_krw"], max_krow=0.9 * u["max_krow"], max_krg=0.85 * u["max_krg"])
        a, b = db.sat_probe(sw, sg, es, sat_region=sr), ds.sat_probe(sw, sg, es, sat_region=ss)
        same(a, b, ("sat_probe with an endscale", three))
        same(a, oracle_bind.OracleFluid(orc, big).sat_probe(sw, sg, es, sat_region=sr), ("sat_probe with an endscale, oracle", three))
        assert not np.array_equal(a, ds.sat_probe(sw, sg, sat_region=ss))
    # the well-bore density: a producer through both meanings and a water injector on a 2 x 2 x 12 column
    W = pkg.wells
    dens = []
    for fl, r_p, r_s in ((big, pr, sr), (small, ps, ss)):
        case = pkg.decks.cartesian_case(2, 2, 12, state="mixed", heterogeneous=True, dz=1.0, fluid=fl)
        case["pvtnum"] = np.full(case["Nb"], r_p, np.int32)
        case["satnum"] = np.full(case["Nb"], r_s, np.int32)
        m = pkg.capi.HipModel(case)
        m.set_state(case["pv"], case["meaning"])
        wells = []
        for name, (i, j), producer, control, limit, inj in (("P", (0, 0), True, ("rate", W.OIL, 20.0 / DT), 150e5, None),
                                                              ("I", (1, 1), False, ("rate", W.WATER, 30.0 / DT), 400e5, "water")):
            cells = [i + 2 * (j + 2 * k) for k in range(12)]
            tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
            wells.append(W.Well(name, cells, tw, case["depth"][cells[0]] - 1.5, producer, control, limit, inj_phase=inj))
        W.DeviceStandardWells(wells, case["depth"], m, head_model="wellbore")
        m.std_wells_begin_iteration(0)
        wb = m.std_wells_wellbore()
        dens.append((wb["density"].copy(), wb["p_avg"].copy(), wb["mixture"].copy(), m.std_wells_blocks()["head"].copy()))
    for k, what in enumerate(("density", "p_avg", "mixture", "head")):
        same(dens[0][k], dens[1][k], ("well bore", what))
    assert np.all(dens[0][0] > 10.0) and np.all(dens[0][0] < 1200.0) and len(dens[0][0]) == 24


@pytest.mark.parametrize("size", ["3073", "norne_sized"])
def test_hysteresis_update_behind_a_padding(pkg, orc, fluids, size):
    """a drainage and an imbibition region behind the padding: opmhip_set_hysteresis, three updates towards more gas and water and
    an assembly and the change of time step (end_time_step, begin_time_step), then a step back; turning points, shifts, Jacobian, residual
    and iq() are the oracle's and those of the two regions alone"""
    spe1 = fluids["spe1"][0]
    alone = pkg.fluid.Fluid(spe1.pvt, helpers.hysteresis_sat_regions(pkg), rock_pref=spe1.rock_pref, rock_cr=spe1.rock_cr, pc_scaling=True)
    big = ts.padded_fluid(pkg, alone, ts.TAB_LDS_DBL + 1, where="before") if size == "3073" else ts.padded_fluid(pkg, alone, sat_regions=100, where="before")
    n = ts.blob_doubles(big)
    assert n == ts.TAB_LDS_DBL + 1 if size == "3073" else n > 10000
    sides = []
    for fl in (big, alone):
        case = pkg.decks.cartesian_case(6, 5, 4, state="mixed", heterogeneous=True, fluid=fl)
        ns = len(fl.sat)
        case["pvtnum"] = np.full(case["Nb"], len(fl.pvt) - 1, np.int32)
        case["satnum"] = np.full(case["Nb"], ns - 2, np.int32)
        case["imbnum"] = np.full(case["Nb"], ns - 1, np.int32)
        m, o = two(pkg, orc, case)
        for q in (m, o):
            q.set_hysteresis(0, case["imbnum"])
        sides += [m, o]
    Nb = sides[0].Nb
    rng = np.random.default_rng(9)
    fwd = np.column_stack([-rng.uniform(0.02, 0.1, Nb), rng.uniform(-1e5, 1e5, Nb), -rng.uniform(0.02, 0.1, Nb)]).reshape(-1)
    moved = scanning = 0
    for step, dx in enumerate((fwd, fwd, -1.5 * fwd)):
        before = [a.copy() for a in sides[0].hysteresis()]
        updates_agree(sides, [dx])
        jr = [q.assemble(DT, 0) for q in sides]
        for i in range(1, 4):
            same(jr[i][0], jr[0][0], ("jacobian", step, i))
            same(jr[i][1], jr[0][1], ("residual", step, i))
        for q in sides:
            q.end_time_step(DT)
            q.begin_time_step(DT)          # (the turning points are taken at the start of the next time step)
        h = [q.hysteresis() for q in sides]
        for i in range(1, 4):
            for k in range(4):
                same(h[i][k], h[0][k], ("hysteresis", step, i, k))
            same(sides[i].iq(), sides[0].iq(), ("iq after the change of time step", step, i))
        moved += int(not np.array_equal(h[0][0], before[0])) + int(not np.array_equal(h[0][2], before[2]))
        scanning += int(np.sum(1.0 - sides[0].iq()[:, 1, 0] > h[0][0]))
    assert moved >= 2 and scanning >= 8      # turning points moved; cells sat on scanning curves


@pytest.mark.parametrize("size", ["3072", "3073", "norne_sized", "3073_extended"])
def test_every_region_in_use(pkg, orc, fluids, size):
    """satnum = cell % num_sat, pvtnum = cell % num_pvt on a 9 x 8 x 7 grid: three rounds of assembly, convergence and update"""
    key, base = PADDINGS[size]
    fl = fluids[key % ("before" if size == "3073_extended" else "after")][0]
    if size == "3073_extended":
        case = helpers.wetgas_case(pkg, 9, 8, 7, rocktab=helpers.ROCKTAB_2, heterogeneous=True)
        case["fluid"] = fl
    else:
        case = pkg.decks.cartesian_case(9, 8, 7, state="mixed", heterogeneous=True, fluid=fl)
    Nb = case["Nb"]
    case["pvtnum"] = (np.arange(Nb) % len(fl.pvt)).astype(np.int32)
    case["satnum"] = (np.arange(Nb) % len(fl.sat)).astype(np.int32)
    assert len(np.unique(case["satnum"])) == len(fl.sat)
    rng = np.random.default_rng(41)
    m, o = two(pkg, orc, case)
    same(m.iq(), o.iq(), "iq")
    dt = 3 * DT
    for it in range(3):
        jm, rm = m.assemble(dt, it)
        jo, ro = o.assemble(dt, it)
        same(rm, ro, ("residual", it))
        same(jm, jo, ("jacobian", it))
        np.testing.assert_allclose(m.convergence(dt)[11:17], o.convergence(dt)[11:17], rtol=1e-9, atol=1e-14)
        dx = (rng.standard_normal((Nb, 3)) * np.array([0.05, 2e5, 0.05])).reshape(-1)
        updates_agree([m, o], [dx])
    assert len(np.unique(m.get_state()[1])) >= 2

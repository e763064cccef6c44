"""Fluids in place and region pressures per FIP region on the device (opmhip_set_fip_regions, opmhip_fluid_in_place, ...; kernels
k_fip_cells / k_fip_reduce / k_fip_totals of csrc/fip.hip) against opm-autodiff_amd/fip.py: the reference's own numbers for its summary
deck, the per-cell terms and the region sums bit for bit - the sums in their stated order, whatever the context's ordering -, the
"originally in place" record, the surface-volume balance of the SPE1 deck's first report step, every refusal, and the rest of the
library untouched while no regions are set."""
import ctypes as C
import uuid

import numpy as np
import pytest

import helpers
from test_oracle_ecl_output import check

pytestmark = pytest.mark.gpu

DAY = 86400.0


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("regions", "field"))


def _metric(s):
    return {k: (v / 1e5 if k.startswith(("FPR", "RPR")) else v) for k, v in s.items()}


def test_summary_deck_meets_the_references_numbers_on_the_device(pkg):
    case, fipnum = helpers.summary_deck_case(pkg)
    got = []
    for kw in ({}, {"reorder": "line_coloring"}):
        m = pkg.capi.HipModel(case, **kw)
        m.set_state(case["pv"], case["meaning"])
        m.set_fip_regions({"FIPNUM": fipnum})
        assert m.fip_info() == dict(max_id=3, cells=1000, chunks=5, levels=2)     # 400 + 200 + 400 cells: 2 + 1 + 2 chunks
        ip = m.fluid_in_place()
        check(_metric(pkg.fip.summary(ip)))
        got.append(ip)
    assert _same(got[0], got[1])
    # what the read-back path of tests/test_gpu_ecl_output.py forms from the same records, to rounding (another order, 1 - S_w for S_o + S_g)
    old = helpers.summary_from_iq(m.iq(), case["volume"], fipnum)
    new = _metric(pkg.fip.summary(ip))
    for k, v in old.items():
        assert abs(new[k] - v) <= 1e-12 * abs(v), k


@pytest.mark.parametrize("wet", [False, True])
def test_per_cell_terms_bit_for_bit(pkg, wet):
    case = helpers.wetgas_case(pkg, 7, 6, 8, heterogeneous=True) if wet else pkg.decks.cartesian_case(7, 6, 8, state="mixed", heterogeneous=True)
    m = pkg.capi.HipModel(case, reorder="line_coloring")
    m.set_state(case["pv"], case["meaning"])
    m.set_fip_regions({"FIPNUM": np.ones(case["Nb"], int)})
    iq = m.iq()
    assert iq.shape[1] == (19 if wet else 17)
    want = pkg.fip.cell_terms(iq, case["volume"], case["poro"])
    got = m.fluid_in_place_cells()
    assert got.shape == (12, case["Nb"]) and np.array_equal(got, want)
    T = pkg.fip.T
    assert np.any(want[T["OilInGasPhase"]] > 0.0) == wet and np.any(want[T["GasInLiquidPhase"]] > 0.0) and np.all(want[T["WATER"]] > 0.0)
    assert not np.array_equal(want[T["DynamicPoreVolume"]], want[T["PoreVolume"]])     # the rock's compressibility


# ---- 41 x 41 x 40: 67 240 cells, three sets at once --------------------------------------------------------------------------------
SLABS = (1, 63, 64, 65, 0, 255, 256, 257)      # cells of regions 1 .. 8 (id 5 is carried by no cell), then 100 cells of no region, the rest region 9


@pytest.fixture(scope="module")
def big(pkg):
    nx, ny, nz = 41, 41, 40
    case = pkg.decks.cartesian_case(nx, ny, nz, state="mixed", heterogeneous=True)
    n = case["Nb"]
    slabs = np.full(n, 9)
    at = 0
    for r, cnt in enumerate(SLABS):
        slabs[at:at + cnt] = r + 1
        at += cnt
    slabs[at:at + 60] = 0
    slabs[at + 60:at + 100] = -2
    c = np.arange(n)
    i, j, k = c % nx, (c // nx) % ny, c // (nx * ny)
    sets = {"FIPNUM": np.ones(n, int), "FIPSLAB": slabs, "FIPMIX": (i + j + k) % 3 + 1}
    return dict(case=case, sets=sets, want=None, got=None)


@pytest.mark.parametrize("reorder", [None, "line_coloring"])
def test_sums_equal_the_stated_form_bit_for_bit(pkg, big, reorder):
    case, sets = big["case"], big["sets"]
    m = pkg.capi.HipModel(case, **({} if reorder is None else {"reorder": reorder}))
    m.set_state(case["pv"], case["meaning"])
    m.set_fip_regions(sets)
    assert m.fip_info("FIPNUM") == dict(max_id=1, cells=67240, chunks=263, levels=3)       # 67 240 -> 263 -> 2 -> 1
    assert m.fip_info("FIPSLAB")["max_id"] == 9 and m.fip_info("FIPSLAB")["cells"] == 67240 - 100 and m.fip_info("FIPMIX")["max_id"] == 3
    if big["want"] is None:          # the comparator once: the records do not depend on the ordering (checked below through the terms)
        terms = pkg.fip.cell_terms(m.iq(), case["volume"], case["poro"])
        big["terms"] = terms
        big["want"] = {name: pkg.fip.inplace(terms, region, "stated") for name, region in sets.items()}
    else:
        assert np.array_equal(m.fluid_in_place_cells(), big["terms"])
    got = {name: m.fluid_in_place(name) for name in sets}
    for name in sets:
        assert _same(got[name], big["want"][name]), name
        assert _same(m.fluid_in_place(name), got[name]), name                           # two calls in a row
        assert _same(m.fluid_in_place_initial(name), got[name]), name
    slab = got["FIPSLAB"]["regions"]
    assert slab.shape == (9, 14) and np.all(slab[4, :12] == 0.0) and np.all(np.isnan(slab[4, 12:])) and np.all(slab[[0, 1, 2, 3, 5, 6, 7, 8], 0] > 0.0)
    # cells of no region are in no total: the slabs' field is less than the whole field's
    assert got["FIPSLAB"]["field"][0] < got["FIPNUM"]["field"][0] and got["FIPNUM"]["field"][0] == got["FIPNUM"]["regions"][0, 0]
    # ... and the stated order is not the reference's loop: equal to rounding, not to the bit, on 67 240 cells
    seq = pkg.fip.inplace(big["terms"], sets["FIPNUM"], "sequential")["field"]
    assert np.allclose(seq, got["FIPNUM"]["field"], rtol=67240 * 2.0 ** -52, atol=0.0) and not np.array_equal(seq, got["FIPNUM"]["field"])
    if big["got"] is None:
        big["got"] = got
    else:                            # the other ordering of the context: the same bits
        assert all(_same(got[name], big["got"][name]) for name in sets)


def test_state_follows_the_run_and_the_initial_record_stays(pkg):
    case = pkg.decks.cartesian_case(8, 7, 6, state="mixed", heterogeneous=True)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=100.0)
    m = pkg.capi.HipModel(case, reorder="line_coloring")
    m.set_state(case["pv"], case["meaning"])
    m.set_source(src)
    region = np.arange(case["Nb"]) % 2 + 1
    m.set_fip_regions({"FIPNUM": region})
    with pytest.raises(pkg.capi.OpmHipError) as e:
        m.fluid_in_place_initial()
    assert e.value.code == pkg.capi.NOT_READY
    first = m.fluid_in_place()
    drv = pkg.newton.BlackoilModelHip(m)
    drv.advance_time_level()
    dt = 5 * DAY
    assert drv.step(dt).converged
    drv.end_time_step(dt)
    second = m.fluid_in_place()
    T = pkg.fip.T
    assert not np.array_equal(second["field"], first["field"]) and not np.array_equal(second["regions"], first["regions"])
    assert _same(m.fluid_in_place_initial(), first)
    want = pkg.fip.inplace(pkg.fip.cell_terms(m.iq(), case["volume"], case["poro"]), region, "stated")
    assert _same(second, want)
    s = pkg.fip.summary(second, initial=m.fluid_in_place_initial())
    assert s["FOE"] == second["field"][T["OIL"]] / first["field"][T["OIL"]] and 0.0 < s["FOE"] < 1.0      # oil is produced
    # the sources' own surface volumes, to what the Newton method's stopping rule leaves (MB <= 1e-6 of the pore volume per step)
    moved = src.reshape(-1, 3).sum(axis=0) * dt                                                        # equations: oil, water, gas
    slack = 2e-6 * float((case["volume"] * case["poro"]).sum())
    assert abs((second["field"][T["OIL"]] - first["field"][T["OIL"]]) - moved[0]) <= slack
    assert abs((second["field"][T["WATER"]] - first["field"][T["WATER"]]) - moved[1]) <= slack
    # new regions start a new record
    m.set_fip_regions({"FIPNUM": region})
    assert _same(m.fluid_in_place(), second) and _same(m.fluid_in_place_initial(), second)


def test_spe1_first_report_step_mass_balance(pkg):
    """decks.spe1_case with its two wells over the first report step: the change of the field's OIL, WATER and GAS is what the wells
    moved, within the bound of tests/test_spe1_deck.py::test_first_report_step_on_the_oracle - twice the Newton method's own MB <= 1e-6 of
    the pore volume per sub-step, the gas balance in gas volumes (times the initial Rs, 1.27 Mscf/stb)"""
    case = pkg.decks.spe1_case()
    m = pkg.capi.HipModel(case, tolerance=1e-2, maxit=200, ilu_relaxation=0.9)
    m.set_state(case["pv"], case["meaning"])
    m.set_composition_change_limits(drsdt=case["drsdt"], drsdt_all_cells=case["drsdt_all_cells"])
    m.set_fip_regions({"FIPNUM": np.ones(case["Nb"], int)})
    f0 = m.fluid_in_place()["field"]
    wells = pkg.decks.spe1_wells(case)
    model = pkg.newton.BlackoilModelHip(m, well_model=wells)
    ts = pkg.newton.AdaptiveTimeStepping(model, pkg.newton.TimeSteppingParameters(initial_dt=DAY))
    moved = np.zeros(3)          # surface volumes the wells put into the reservoir, sub-step by sub-step: oil, water, gas

    def on_accept(dt):
        moved[:] += (wells.x[0, :3] + wells.x[1, :3]) * dt
    ts.on_accept = on_accept
    ts.advance_report_step(case["schedule"]["tstep"][0])
    assert all(ok for _, _, ok in ts.history)
    f1 = m.fluid_in_place()["field"]
    T = pkg.fip.T
    mb_slack = 1e-6 * float((case["volume"] * case["poro"]).sum()) * len(ts.history)
    rs_prod = 1.27 * 28.316846592 / 0.158987294928
    for name, q, bound in (("OIL", moved[0], 2.0 * mb_slack), ("WATER", moved[1], 2.0 * mb_slack), ("GAS", moved[2], 2.0 * mb_slack * rs_prod)):
        change = f1[T[name]] - f0[T[name]]
        print("%s: in place %.9e -> %.9e, change %.9e, wells %.9e, bound %.3e" % (name, f0[T[name]], f1[T[name]], change, q, bound))
        assert abs(change - q) <= bound, name
    assert moved[0] < 0.0 < moved[2] and f1[T["GasInGasPhase"]] > f0[T["GasInGasPhase"]] == 0.0       # free gas appears at the injector
    s = pkg.fip.summary(m.fluid_in_place(), initial=m.fluid_in_place_initial())
    assert s["FOE"] == f1[T["OIL"]] / f0[T["OIL"]]


def test_statuses(pkg):
    capi = pkg.capi
    L = capi.lib()
    case = pkg.decks.cartesian_case(5, 4, 3, state="mixed")
    n = case["Nb"]
    m = capi.HipModel(case)
    ones = np.ones(n, np.int32)

    def refused(code, word, fn):
        with pytest.raises(capi.OpmHipError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)

    refused(capi.NOT_READY, "before set_state", lambda: m.fluid_in_place())            # neither a state nor regions
    m.set_fip_regions({"FIPNUM": ones})
    refused(capi.NOT_READY, "before set_state", lambda: m.fluid_in_place())
    refused(capi.NOT_READY, "before set_state", lambda: m.fluid_in_place_cells())
    m.set_fip_regions({})
    m.set_state(case["pv"], case["meaning"])
    refused(capi.NOT_READY, "before set_fip_regions", lambda: m.fluid_in_place())
    refused(capi.NOT_READY, "before set_fip_regions", lambda: m.fluid_in_place_cells())
    refused(capi.NOT_READY, "before set_fip_regions", lambda: m.fip_info(0))
    m.set_fip_regions({"FIPNUM": ones, "FIPTWO": ones * 2})
    good = m.fluid_in_place("FIPTWO")
    for bad in (2, -1):
        refused(capi.INVALID_ARGUMENT, "set %d of 2" % bad, lambda: m.fluid_in_place(bad))
        refused(capi.INVALID_ARGUMENT, "set %d of 2" % bad, lambda: m.fluid_in_place_initial(bad))
    # refused set-ups leave the sets in force
    above = ones.copy()
    above[3] = n + 1
    refused(capi.INVALID_ARGUMENT, "above the %d cells" % n, lambda: m.set_fip_regions({"FIPNUM": above}))
    refused(capi.INVALID_ARGUMENT, "num_sets = 17", lambda: m.set_fip_regions({"FIP%02d" % i: ones for i in range(17)}))
    ptrs = (C.c_void_p * 2)(ones.ctypes.data, None)
    assert L.opmhip_set_fip_regions(m._h, 2, ptrs) == capi.INVALID_ARGUMENT and b"region[1] == NULL" in L.opmhip_last_error(m._h)
    assert L.opmhip_set_fip_regions(m._h, 1, None) == capi.INVALID_ARGUMENT and b"region == NULL" in L.opmhip_last_error(m._h)
    assert L.opmhip_set_fip_regions(m._h, -1, ptrs) == capi.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        m.set_fip_regions({"FIPNUM": ones[:-1]})
    assert m.fip_info("FIPTWO")["max_id"] == 2 and _same(m.fluid_in_place("FIPTWO"), good)
    top = ones.copy()
    top[0] = n                                  # the largest id the check lets through
    m.set_fip_regions({"FIPNUM": top})
    ip = m.fluid_in_place()
    assert ip["regions"].shape == (n, 14) and np.all(ip["regions"][1:n - 1, :12] == 0.0) and ip["regions"][n - 1, 0] > 0.0
    m.set_fip_regions({"F%d" % i: ones for i in range(16)})
    assert _same(m.fluid_in_place("F15"), m.fluid_in_place("F0"))
    # a decomposed context: the sums over the ranks are not formed
    part = pkg.ras.cartesian_subdomain_case(6, 2, 0, state="mixed", heterogeneous=False)
    d = capi.HipModel(part, comm=("loopback", 2, 0, "fip" + uuid.uuid4().hex), reorder="level_scheduling")
    d.set_state(part["pv"], part["meaning"])
    refused(capi.INVALID_ARGUMENT, "decomposed", lambda: d.set_fip_regions({"FIPNUM": np.ones(part["Nb"], int)}))
    refused(capi.NOT_READY, "before set_fip_regions", lambda: d.fluid_in_place())
    assert d.iq().shape[0] == d.Nloc > part["Nb"]


def test_no_regions_no_difference(pkg):
    """a context that has set, used and released regions runs an assemble / solve / update cycle with the launches - counted per class
    by opmhip_profile_get - and the bits of one that never called any of these entry points"""
    case = pkg.decks.cartesian_case(12, 10, 6, state="mixed", heterogeneous=True)
    src = pkg.decks.five_spot_source(case, rate_sm3_per_day=100.0)
    runs = []
    for used in (False, True):
        m = pkg.capi.HipModel(case, reorder="line_coloring")
        m.set_state(case["pv"], case["meaning"])
        m.set_source(src)
        if used:
            m.set_fip_regions({"FIPNUM": np.arange(case["Nb"]) % 4})
            m.fluid_in_place()
            m.fluid_in_place_cells()
            m.set_fip_regions(None)
        m.profile_enable(True)
        j, r = m.assemble(DAY, 0)
        res = m.solve_jacobian_system()
        x = m.get_result()
        m.update(None, 1.0)
        prof = {k: v[0] for k, v in m.profile().items()}
        runs.append((prof, j, r, res.it, x, m.get_state()[0]))
    a, b = runs
    assert a[0] == b[0] and sum(a[0].values()) > 0
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])

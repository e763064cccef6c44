"""The heads from the well-bore density (wells.StandardWells(head_model="wellbore"), opmhip_set_std_wells_head_model) without a GPU: the
new symbols and the struct at the drop-in boundary, the host statement on wells whose numbers can be written out by hand - the CPU
oracle's property functions as the evaluator -, the default model untouched, and the stated form against the NumPy form.

Measured here (numpy 2.2.6) on decks.spe9_shaped_wells after one assembly at a moved well state, stated against NumPy form, largest
relative difference; the test asserts 100 x these, that is equality where the measured value is 0:

    density of the well-bore segments     0
    head                                  0

(These wells have three to five completions: a cumsum and a three-term sum add in the loop's order.)
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("opmhip_set_std_wells_head_model", "opmhip_get_std_wells_wellbore", "opmhip_set_std_wells_perf_state")
MEASURED = dict(density=0.0, head=0.0)
G = 9.80665


# ---- the drop-in boundary -----------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_exported(pkg):
    L = pkg.capi.lib()
    names = pkg.capi.declared_symbols()
    for n in SYMBOLS:
        assert n in names and hasattr(L, n), n
    assert L.opmhip_abi_version() == 11          # additive


def test_wellbore_struct_matches_the_header(pkg, tmp_path):
    fields = [f[0] for f in pkg.capi.StdWellsWellbore._fields_]
    assert fields == ["perf_depth", "ref_depth", "preferred_phase"]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "opmhip.h"', 'int main(void) {', '  printf("wb %zu\\n", sizeof(opmhip_std_wells_wellbore));',
             '  printf("sw %zu\\n", sizeof(opmhip_std_wells));']
    for f in fields:
        lines.append('  printf("wb.%s %%zu\\n", offsetof(opmhip_std_wells_wellbore, %s));' % (f, f))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["wb"]) == ctypes.sizeof(pkg.capi.StdWellsWellbore)
    assert int(out["sw"]) == ctypes.sizeof(pkg.capi.StdWells)        # the list's struct is as it was
    for f in fields:
        assert int(out["wb." + f]) == getattr(pkg.capi.StdWellsWellbore, f).offset, f


def good():
    return dict(perf_depth=[2500.0, 2505.0, 2510.0, 2500.0], ref_depth=[2499.0, 2500.0], preferred_phase=[1, 2])


def test_struct_builder(pkg):
    s, keep = pkg.capi.make_std_wells_wellbore(good(), 2, 4)
    assert s.perf_depth == keep["perf_depth"].ctypes.data and s.ref_depth == keep["ref_depth"].ctypes.data and s.preferred_phase == keep["preferred_phase"].ctypes.data
    assert keep["perf_depth"].dtype == np.float64 and keep["preferred_phase"].dtype == np.int32 and list(keep["preferred_phase"]) == [1, 2]
    assert pkg.capi.make_std_wells_wellbore(None, 2, 4) == (None, {})


@pytest.mark.parametrize("key,value", [("perf_depth", [2500.0] * 3), ("perf_depth", [2500.0] * 5), ("ref_depth", [2499.0]), ("preferred_phase", [1, 1, 1]),
                                       ("preferred_phase", [])])
def test_struct_builder_rejects_ragged_input(pkg, key, value):
    with pytest.raises(ValueError):
        pkg.capi.make_std_wells_wellbore(dict(good(), **{key: value}), 2, 4)


def test_the_classes_refuse_what_they_cannot_state(pkg):
    W = pkg.wells
    w = [W.Well("A", [0, 1], [1.0, 1.0], 0.0, True, ("rate", W.OIL, 1.0), 1e7)]
    with pytest.raises(ValueError):
        W.StandardWells(w, np.zeros(4), head_model="mixture")
    with pytest.raises(ValueError):
        W.StandardWells(w, np.zeros(4), head_model="wellbore")                       # no evaluator
    with pytest.raises(ValueError):
        W.DeviceStandardWells(w, np.zeros(4), model=None, head_model="mixture")
    bad = [W.Well("B", [0], [1.0], 0.0, True, ("rate", W.OIL, 1.0), 1e7, preferred_phase="steam")]
    with pytest.raises(ValueError):
        W.DeviceStandardWells(bad, np.zeros(4), model=None, head_model="wellbore")
    assert w[0].preferred_phase == "oil"


# ---- the host statement on hand-checkable wells ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def column(pkg, orc):
    """2 x 2 x 6, cell = i + 2 (j + 2 k).  Column (0, 0): the deck's mixed state (gas cap above, undersaturated oil below).  Column (1, 0):
    water at its connate saturation and no free gas - only oil is mobile."""
    case = pkg.decks.cartesian_case(2, 2, 6, state="mixed", heterogeneous=True)
    fl = case["fluid"]
    pv = case["pv"].reshape(-1, 3).copy()
    meaning = case["meaning"].copy()
    only_oil = [1 + 2 * (0 + 2 * k) for k in range(6)]
    pv[only_oil, 0] = fl.sat[0]["swof"][0][0]
    pv[only_oil, 2] = 0.5 * pkg.decks.rs_sat(fl, pv[only_oil, 1])
    meaning[only_oil] = pkg.decks.SW_PO_RS
    case = dict(case, pv=np.ascontiguousarray(pv.reshape(-1)), meaning=meaning)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    return case, om.iq(), oracle_bind.OracleFluid(orc, fl)


def col(i, j, ks):
    return [i + 2 * (j + 2 * k) for k in ks]


def build(pkg, column, wells, arithmetic="stated"):
    case, iq, props = column
    return pkg.wells.StandardWells(wells, case["depth"], arithmetic=arithmetic, head_model="wellbore", props=props)


def running_sum(dp):
    out, acc = [], None
    for v in dp:
        acc = float(v) if acc is None else acc + float(v)
        out.append(acc)
    return np.array(out)


def test_a_water_injector_at_rest(pkg, column):
    """(a) three completions, all rates zero: every segment holds water at the mean pressure"""
    case, iq, props = column
    W = pkg.wells
    cells = col(0, 0, [3, 4, 5])
    ref = case["depth"][cells[0]] - 7.0
    sw = build(pkg, column, [W.Well("I", cells, [1e-12] * 3, ref, False, ("rate", W.WATER, 1e-3), 400e5, inj_phase="water")])
    sw.calculate_explicit_quantities(iq)
    po = iq[cells, W.F_P + W.PH_O, 0]
    bhp = po[0] + 1e5
    assert sw.x[0, 3] == bhp
    p_avg = np.array([(po[0] + bhp) / 2, (po[1] + po[0]) / 2, (po[2] + po[1]) / 2])
    bw = props.probe(p_avg)[:, 0]
    rho_w = case["fluid"].pvt[0]["density"][1]
    density = np.array([rho_w / (1.0 / b) for b in bw])                   # inner_product(surface density, mix) / volrat, mix = x = (0, 1, 0)
    z = case["depth"][cells]
    dp = np.array([(z[0] - ref) * density[0] * G, (z[1] - z[0]) * density[1] * G, (z[2] - z[1]) * density[2] * G])
    assert np.array_equal(sw.wellbore["p_avg"], p_avg)
    assert np.array_equal(sw.wellbore["mixture"], [[0.0, 1.0, 0.0]] * 3)
    assert np.array_equal(sw.wellbore["density"], density)
    assert np.array_equal(sw.head, running_sum(dp))
    assert np.allclose(density, rho_w * bw, rtol=4e-16, atol=0.0) and np.all(density > 900.0)      # rho_w,surface * b_w(p_avg), two roundings apart
    # the same well through the NumPy form
    sn = build(pkg, column, [W.Well("I", cells, [1e-12] * 3, ref, False, ("rate", W.WATER, 1e-3), 400e5, inj_phase="water")], "numpy")
    sn.calculate_explicit_quantities(iq)
    assert np.allclose(sn.head, sw.head, rtol=1e-15, atol=0.0)


def test_a_producer_at_rest_takes_the_mobility_ratio(pkg, column):
    """(b) exactly zero rates: tw / sum(tw) * mobility / sum(1/B * mobility); only oil is mobile in its cells: the mixture is (1, 0, 0)"""
    case, iq, props = column
    W = pkg.wells
    cells = col(1, 0, [1, 2, 3])
    assert np.all(iq[cells, W.F_MOB + W.PH_W, 0] == 0.0) and np.all(iq[cells, W.F_MOB + W.PH_G, 0] == 0.0) and np.all(iq[cells, W.F_MOB + W.PH_O, 0] > 0.0)
    sw = build(pkg, column, [W.Well("P", cells, [1e-12, 3e-12, 2e-12], case["depth"][cells[0]], True, ("rate", W.OIL, 1e-3), 100e5)])
    sw.calculate_explicit_quantities(iq)
    assert np.all(sw.perf_rates == 0.0)                                    # the stored rates stay what they were: the fallback is the mixture's alone
    assert np.array_equal(sw.wellbore["mixture"], [[1.0, 0.0, 0.0]] * 3)
    rho_o = case["fluid"].pvt[0]["density"][0]
    p_avg = sw.wellbore["p_avg"]
    pr = props.probe(p_avg)
    bo = props.probe(p_avg, pr[:, 3])[:, 2]                                # no gas rate: the saturated curve
    assert np.array_equal(sw.wellbore["density"], [rho_o / (1.0 / b) for b in bo])
    assert sw.head[0] == 0.0 and np.all(np.diff(sw.head) > 0.0)
    # with the preferred phase gas and nothing mobile to say otherwise?  No: the fallback still decides - the preferred phase is for a
    # perforation without flow only
    sg = build(pkg, column, [W.Well("P", cells, [1e-12, 3e-12, 2e-12], case["depth"][cells[0]], True, ("rate", W.OIL, 1e-3), 100e5, preferred_phase="gas")])
    sg.calculate_explicit_quantities(iq)
    assert np.array_equal(sg.head, sw.head)


def corrected(W, mix, rsmax, rvmax):
    """the rs / rv correction of computeConnectionDensities, written out"""
    x = list(mix)
    rs = rv = 0.0
    if mix[W.OIL] > 1e-12:
        rs = min(mix[W.GAS] / mix[W.OIL], rsmax)
    if mix[W.GAS] > 1e-12:
        rv = min(mix[W.OIL] / mix[W.GAS], rvmax)
    if rs != 0.0:
        x[W.GAS] = (mix[W.GAS] - mix[W.OIL] * rs) / (1.0 - rs * rv)
    if rv != 0.0:
        x[W.OIL] = (mix[W.OIL] - mix[W.GAS] * rv) / (1.0 - rs * rv)
    return x


def test_closed_completions(pkg, column):
    """(c) the middle completion closed while the bottom one flows: the flow from below passes it unchanged.  The bottom two closed: no
    flow at perforations 1 and 2, which take x - the corrected mixture, not the mixture - of the perforation above"""
    case, iq, props = column
    W = pkg.wells
    cells = col(0, 0, [0, 1, 2])                                          # gas-cap cells: water, oil and gas are mobile
    mk = lambda tw: build(pkg, column, [W.Well("P", cells, tw, case["depth"][cells[0]] - 2.0, True, ("rate", W.OIL, 1e-3), 100e5)])
    a = mk([2e-12, 0.0, 1e-12])
    a.calculate_explicit_quantities(iq)
    mix = a.wellbore["mixture"]
    assert np.array_equal(mix[1], mix[2]) and not np.array_equal(mix[0], mix[1]) and np.all(mix > 0.0)
    assert np.allclose(mix.sum(axis=1), 1.0, rtol=1e-15)
    b = mk([2e-12, 0.0, 0.0])
    b.calculate_explicit_quantities(iq)
    mix, x, wb = b.wellbore["mixture"], b.wellbore["x"], b.wellbore
    x0 = corrected(W, mix[0], wb["rsmax"][0], wb["rvmax"][0])
    assert np.array_equal(x[0], x0) and x0[W.GAS] < mix[0][W.GAS]          # dissolved gas taken out of the gas: x is not mix
    assert np.array_equal(mix[1], x[0])                                    # no flow: the x of the perforation above
    x1 = corrected(W, mix[1], wb["rsmax"][1], wb["rvmax"][1])
    assert np.array_equal(x[1], x1) and np.array_equal(mix[2], x[1]) and not np.array_equal(mix[1], mix[0]) and mix[1].sum() < 0.9
    rho = case["fluid"].pvt[0]["density"]
    for p in range(3):
        xp = corrected(W, mix[p], wb["rsmax"][p], wb["rvmax"][p])
        volrat = ((0.0 + xp[0] / wb["b"][p, 0]) + xp[1] / wb["b"][p, 1]) + xp[2] / wb["b"][p, 2]
        sd = ((0.0 + rho[0] * mix[p][0]) + rho[1] * mix[p][1]) + rho[2] * mix[p][2]
        assert wb["density"][p] == sd / volrat, p                           # the density uses mix in the numerator, x in the volume ratio
    # the numpy form takes the same branches
    n = build(pkg, column, [W.Well("P", cells, [2e-12, 0.0, 0.0], case["depth"][cells[0]] - 2.0, True, ("rate", W.OIL, 1e-3), 100e5)], "numpy")
    n.calculate_explicit_quantities(iq)
    assert np.allclose(n.wellbore["mixture"], mix, rtol=1e-14, atol=0.0) and np.allclose(n.head, b.head, rtol=1e-14, atol=0.0)


def test_a_one_completion_well(pkg, column):
    """(d) its head is (perf_depth - ref_depth) * density * g and nothing else"""
    case, iq, props = column
    W = pkg.wells
    cell = col(0, 0, [4])
    ref = case["depth"][cell[0]] - 11.5
    sw = build(pkg, column, [W.Well("P", cell, [1e-12], ref, True, ("rate", W.OIL, 1e-3), 100e5),
                             W.Well("I", col(1, 0, [5]), [1e-12], case["depth"][-1] + 3.0, False, ("rate", W.GAS, 1.0), 400e5, inj_phase="gas")])
    sw.calculate_explicit_quantities(iq)
    assert sw.head[0] == (case["depth"][cell[0]] - ref) * sw.wellbore["density"][0] * G
    assert sw.head[1] == (case["depth"][col(1, 0, [5])[0]] - (case["depth"][-1] + 3.0)) * sw.wellbore["density"][1] * G and sw.head[1] < 0.0
    assert np.array_equal(sw.wellbore["mixture"][1], [0.0, 0.0, 1.0]) and 50.0 < sw.wellbore["density"][1] < 400.0       # gas at 250 bar


def test_the_state_follows_the_assembly(pkg, column):
    """every assembly leaves bhp + head and the rates' values per perforation; state() / set_state() carry them"""
    case, iq, props = column
    W = pkg.wells
    cells = col(0, 0, [2, 3, 4])
    tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
    sw = build(pkg, column, [W.Well("P", cells, tw, case["depth"][cells[0]], True, ("rate", W.OIL, 5.0 / 86400.0), 100e5)])
    st0 = sw.state()
    assert st0[2][0] is None and np.all(st0[2][1] == 0.0) and st0[2][2] is False
    sw.calculate_explicit_quantities(iq)
    head0 = sw.head.copy()
    sw.solve_well_equations(iq)
    assert np.all(sw.perf_rates == 0.0)                                    # the wells alone leave the stored state alone
    wa = sw.assemble(iq)
    assert np.array_equal(sw.perf_pressure, sw.x[0, 3] + sw.head) and np.array_equal(sw.perf_rates.sum(axis=0), wa["source_cells"].reshape(-1, 3).sum(axis=0))
    assert np.all(sw.perf_rates[:, W.OIL] <= 0.0) and sw.perf_rates[:, W.OIL].min() < 0.0
    st1 = sw.state()
    sw.calculate_explicit_quantities(iq)                                   # the next time step: flowing rates, the well's own pressures
    head1 = sw.head.copy()
    assert not np.array_equal(head1, head0) and np.all(head1[1:] > head0[1:]) and np.all(head1[1:] < 2.0 * head0[1:])      # oil from below in place of the gas cap's share
    sw.set_state(st0)
    sw.initialised = False
    sw.calculate_explicit_quantities(iq)
    assert np.array_equal(sw.head, head0)
    sw.set_state(st1)
    sw.initialised = True
    sw.calculate_explicit_quantities(iq)
    assert np.array_equal(sw.head, head1)


def test_a_first_step_given_up(pkg, column):
    """state() from before the first time step, set_state() after its iterations (newton.BlackoilModelHip's roll-back): the retry forms the
    heads of an object that never tried the step - perforation and bottom-hole pressures from the cells again, no segment at half pressure"""
    case, iq, props = column
    W = pkg.wells
    cells = col(0, 0, [1, 2, 3, 4])
    tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
    mk = lambda: build(pkg, column, [W.Well("P", cells, tw, case["depth"][cells[0]] - 3.0, True, ("rate", W.OIL, 20.0 / 86400.0), 100e5),
                                     W.Well("I", col(1, 0, [3, 4, 5]), tw[:3], case["depth"][col(1, 0, [3])[0]], False, ("rate", W.WATER, 1e-4), 400e5, inj_phase="water")])
    fresh, tried = mk(), mk()
    fresh.calculate_explicit_quantities(iq)
    saved = tried.state()
    assert saved[2][0] is None and saved[2][2] is False
    tried.calculate_explicit_quantities(iq)
    tried.solve_well_equations(iq)
    tried.update_well_controls()
    tried.assemble(iq)
    assert tried.initialised and np.any(tried.perf_rates != 0.0)
    tried.set_state(saved)
    assert not tried.initialised and np.all(tried.x == 0.0)
    tried.calculate_explicit_quantities(iq)
    for k in ("density", "p_avg", "mixture"):
        np.testing.assert_array_equal(tried.wellbore[k], fresh.wellbore[k])
    np.testing.assert_array_equal(tried.head, fresh.head)
    assert np.all(tried.wellbore["p_avg"] > 200e5)
    tried.solve_well_equations(iq)
    fresh.solve_well_equations(iq)
    np.testing.assert_array_equal(tried.x, fresh.x)


def test_two_pvt_regions(pkg, orc):
    """the PVT region of a perforation is its cell's: its property functions and its surface densities"""
    fl = pkg.fluid.spe1_fluid()[0]
    r1 = dict(fl.pvt[0])
    r1["density"] = [1.06 * fl.pvt[0]["density"][0], 1.03 * fl.pvt[0]["density"][1], 1.2 * fl.pvt[0]["density"][2]]
    r1["pvtw"] = [fl.pvt[0]["pvtw"][0], 1.04 * fl.pvt[0]["pvtw"][1], 1.5 * fl.pvt[0]["pvtw"][2]] + list(fl.pvt[0]["pvtw"][3:])
    fl2 = pkg.fluid.Fluid([fl.pvt[0], r1], fl.sat, rock_pref=fl.rock_pref, rock_cr=fl.rock_cr)
    case = pkg.decks.cartesian_case(2, 2, 6, state="mixed", heterogeneous=True, fluid=fl2)
    case["pvtnum"] = ((np.arange(case["Nb"]) // 4) % 2).astype(np.int32)
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    props = oracle_bind.OracleFluid(orc, fl2)
    W = pkg.wells
    cells = col(0, 0, [2, 3, 4, 5])
    wells = lambda: [W.Well("I", cells, [1e-12] * 4, case["depth"][cells[0]] - 4.0, False, ("rate", W.WATER, 1e-3), 400e5, inj_phase="water")]
    sw = W.StandardWells(wells(), case["depth"], arithmetic="stated", head_model="wellbore", props=props, pvtnum=case["pvtnum"])
    sw.calculate_explicit_quantities(iq)
    reg = case["pvtnum"][cells]
    assert list(reg) == [0, 1, 0, 1] and list(sw.pvt_of_perf) == [0, 1, 0, 1]
    p_avg = sw.wellbore["p_avg"]
    want = [fl2.pvt[r]["density"][1] / (1.0 / float(props.probe(p_avg[k:k + 1], pvt_region=int(r))[0, 0])) for k, r in enumerate(reg)]
    np.testing.assert_array_equal(sw.wellbore["density"], want)
    one = W.StandardWells(wells(), case["depth"], arithmetic="stated", head_model="wellbore", props=props)
    one.calculate_explicit_quantities(iq)
    assert np.array_equal(one.wellbore["density"][[0, 2]], sw.wellbore["density"][[0, 2]]) and np.all(np.abs(one.wellbore["density"][[1, 3]] / sw.wellbore["density"][[1, 3]] - 1.0) > 0.005)
    # a producer across both regions, both arithmetic forms
    pc = col(1, 0, [0, 1, 2, 3])
    for arithmetic in ("stated", "numpy"):
        pw = W.StandardWells([W.Well("P", pc, [1e-12, 2e-12, 1e-12, 3e-12], case["depth"][pc[0]], True, ("rate", W.OIL, 1e-3), 100e5)], case["depth"],
                             arithmetic=arithmetic, head_model="wellbore", props=props, pvtnum=case["pvtnum"])
        pw.calculate_explicit_quantities(iq)
        rho = np.array([fl2.pvt[r]["density"] for r in case["pvtnum"][pc]])
        wb = pw.wellbore
        np.testing.assert_allclose(wb["density"], (rho * wb["mixture"]).sum(axis=1) / (wb["x"] / wb["b"]).sum(axis=1), rtol=1e-15)


def test_the_default_model_is_untouched(pkg, orc):
    """(e) head_model="cell_oil" is the class as it was: every number of decks.spe1_wells"""
    case = pkg.decks.spe1_case(props=oracle_bind.OracleFluid(orc, pkg.fluid.spe1_fluid()[0]))
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    for arithmetic in ("numpy", "stated"):
        old = pkg.wells.StandardWells(pkg.decks.spe1_wells(case).wells, case["depth"], arithmetic)
        new = pkg.wells.StandardWells(pkg.decks.spe1_wells(case).wells, case["depth"], arithmetic, head_model="cell_oil")
        assert new.head_model == old.head_model == "cell_oil"
        for w in (old, new):
            w.calculate_explicit_quantities(iq)
            w.solve_well_equations(iq)
            w.update_well_controls()
        a, b = old.assemble(iq, case["Nb"]), new.assemble(iq, case["Nb"])
        np.testing.assert_array_equal(new.head, old.head)
        np.testing.assert_array_equal(new.x, old.x)
        for k in ("res_well", "cells", "source_cells", "dsource_cells", "source", "dsource"):
            np.testing.assert_array_equal(b[k], a[k])
        for k in ("val_pointers", "Ccols", "Bcols", "Cnnzs", "Bnnzs", "Dnnzs"):
            np.testing.assert_array_equal(b["wells"][k], a["wells"][k])
        assert len(new.state()) == 2


# ---- stated against NumPy form ------------------------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    d, s = np.abs(a - b), np.maximum(np.abs(a), np.abs(b))
    m = s > 0
    return float((d[m] / s[m]).max()) if m.any() else 0.0


def test_stated_form_against_the_numpy_form(pkg, orc):
    case = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"], case["meaning"])
    iq = om.iq()
    props = oracle_bind.OracleFluid(orc, case["fluid"])
    forms = {a: pkg.wells.StandardWells(pkg.decks.spe9_shaped_wells(case).wells, case["depth"], arithmetic=a, head_model="wellbore", props=props)
             for a in ("numpy", "stated")}
    wn, ws = forms["numpy"], forms["stated"]
    wn.calculate_explicit_quantities(iq)
    wn.solve_well_equations(iq)
    wn.x[:, :3] *= 1.02                                                    # away from the solved state, as tests/test_std_wells_stated.py does
    wn.x[:, 3] += np.where([w.producer for w in wn.wells], -2e5, 3e5)
    wn.assemble(iq)                                                        # flowing rates and the well's own pressures per perforation
    ws.set_state(wn.state())                                               # one well state for both: what differs below is the heads' arithmetic
    ws.initialised = True
    for w in (wn, ws):
        w.calculate_explicit_quantities(iq)
    got = dict(density=rel(wn.wellbore["density"], ws.wellbore["density"]), head=rel(wn.head, ws.head))
    print("spe9-shaped wells, well-bore heads, stated against numpy:", {k: "%.2e" % v for k, v in got.items()})
    assert np.count_nonzero(wn.perf_rates) > 100 and np.all(ws.wellbore["density"] > 100.0) and np.all(ws.wellbore["density"] < 1100.0)
    inj = slice(wn.vp[0], wn.vp[1])
    assert np.all(ws.wellbore["mixture"][inj, pkg.wells.WATER] == 1.0) and np.all(ws.wellbore["density"][inj] > 950.0)
    for k, v in got.items():
        bound = 100.0 * MEASURED[k]
        assert v <= bound, (k, v, bound)          # a measured 0 asks for equality

"""Tables and points the VFP tests share (CPU: test_vfp.py; GPU: test_gpu_vfp.py, test_gpu_std_wells_thp.py): the two fixtures under
tests/golden/ converted to SI at load, and small hand-made tables."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR, DAY = 1e5, 86400.0


def expected():
    with open(os.path.join(GOLDEN, "vfp_expected.json")) as f:
        return json.load(f)


def vfpprod2(vfp):
    """tests/VFPPROD2 in SI: bar * 1e5, Sm3/day / 86400"""
    with open(os.path.join(GOLDEN, "vfpprod2_table.json")) as f:
        t = json.load(f)
    assert (t["table_num"], t["datum_depth"], t["flo_type"], t["wfr_type"], t["gfr_type"]) == (32, 394.0, "LIQ", "WCT", "GOR")
    axes = [np.asarray(t["flo_axis"]) / DAY, np.asarray(t["thp_axis"]) * BAR, t["wfr_axis"], t["gfr_axis"], t["alq_axis"]]
    return vfp.VFPTable(vfp.PROD, t["table_num"], t["datum_depth"], t["flo_type"], axes, np.asarray(t["values"]) * BAR, t["wfr_type"], t["gfr_type"])


def realistic_points(e):
    """the 4096 points of ParseInterpolateRealisticVFPPROD in its loop order (thp, wct, gor, liq) -> aqua, liquid, vapour, thp [Pa], skipped
    (the reference's own rule), reference [bar]"""
    r = e["realistic"]
    tt, ww, gg, ff = np.meshgrid(r["thp"], r["wct"], r["gor"], r["liq"], indexing="ij")
    f_i = -ff.ravel() * 1.1574074074074073e-05
    t_i = tt.ravel() * 100000.0
    aqua = ww.ravel() * f_i
    liquid = f_i - aqua
    vapour = gg.ravel() * liquid
    skipped = ((aqua + liquid) == 0.0) | (liquid == 0.0)
    return aqua, liquid, vapour, t_i, skipped, np.asarray(r["reference"])


def line_table(vfp, e):
    """the ParseInterpolateLine table (FIELD units) in SI: four singleton axes, bhp == thp"""
    t = e["parse_interpolate_line"]
    u = t["units"]
    axes = [np.asarray(t["flo_axis"]) * u["liquid_rate_m3s_per_unit"], np.asarray(t["thp_axis"]) * u["pressure_pa_per_unit"], t["wfr_axis"], t["gfr_axis"],
            t["alq_axis"]]
    return vfp.VFPTable(vfp.PROD, t["table_num"], t["datum_depth"] * u["length_m_per_unit"], t["flo_type"], axes,
                        np.asarray(t["values"]) * u["pressure_pa_per_unit"], t["wfr_type"], t["gfr_type"])


def line_points(e):
    """its 5^5 grid in the loop order (aqua, liquid, vapour, thp, alq), SI already"""
    g = e["parse_interpolate_line"]["grid"]
    k = np.arange(g["n"], dtype=float)
    w, o, v, t, a = np.meshgrid(*(k * g["step"][n] for n in g["loop_order"]), indexing="ij")
    return w.ravel(), o.ravel(), v.ravel(), t.ravel(), a.ravel()


def axis6_table(vfp):
    """a producer table (OIL / WOR / GOR) whose flo axis is the reference's findInterpData axis {1, 5, 7, 9, 11, 15}; two THP entries, the
    other axes singletons; the values are not linear in flo"""
    flo = np.array([1.0, 5.0, 7.0, 9.0, 11.0, 15.0])
    thp = np.array([10.0, 20.0]) * BAR
    values = (thp[:, None] + BAR * (3.0 + 0.5 * flo + 0.07 * flo * flo)[None, :])
    return vfp.VFPTable(vfp.PROD, 6, 1000.0, "OIL", [flo, thp, [0.0], [0.0], [0.0]], values, "WOR", "GOR")


def random_table(vfp, seed=7, kind=None):
    """a seeded table, BHP rising with THP (so the inverse look-up has one answer): the round trip's"""
    rng = np.random.default_rng(seed)
    flo = np.cumsum(rng.uniform(0.1, 0.5, 5))
    thp = np.cumsum(rng.uniform(0.2, 0.4, 4))
    wfr, gfr, alq = np.cumsum(rng.uniform(0.1, 0.3, 3)), np.cumsum(rng.uniform(0.05, 0.2, 4)), np.array([0.0, 20.0, 50.0])
    base = rng.uniform(0.0, 1.0, (3, 4, 3, 5))
    values = 2.0 * thp[:, None, None, None, None] + base[None]
    return vfp.VFPTable(vfp.PROD, 1, 0.0, "LIQ", [flo, thp, wfr, gfr, alq], values, "WCT", "GOR")


def inj_table(vfp, num=3, flo_type="WAT"):
    """VFPINJ: BHP falls with the rate's friction subtracted from the head, rises with THP; not linear in flo"""
    flo = np.array([0.0, 0.002, 0.005, 0.01, 0.03])
    thp = np.array([50.0, 100.0, 200.0]) * BAR
    values = thp[:, None] + BAR * (150.0 - 4.0e3 * flo - 2.0e5 * flo * flo)[None, :]
    return vfp.VFPTable(vfp.INJ, num, 1200.0, flo_type, [flo, thp], values)


def nonmonotone_table(vfp):
    """a producer table whose BHP is not monotone in THP (10, 30, 20, 20, 40 bar at every other coordinate, plus a term in flo): every
    branch of findTHP's unsorted half is reachable, and dy == 0 between the third and fourth entry"""
    flo = np.array([0.001, 0.01])
    thp = np.array([10.0, 20.0, 30.0, 40.0, 50.0]) * BAR
    values = (np.array([10.0, 30.0, 20.0, 20.0, 40.0]) * BAR)[:, None] + np.array([0.0, 2.0 * BAR])[None, :]
    return vfp.VFPTable(vfp.PROD, 9, 0.0, "GAS", [flo, thp, [0.0], [0.0], [0.0]], values, "WGR", "OGR")


def flat_table(vfp):
    """sorted, with two equal BHP values at the low end: findX meets dy == 0 in the sorted half"""
    flo = np.array([0.001, 0.01])
    thp = np.array([10.0, 20.0, 30.0]) * BAR
    values = (np.array([15.0, 15.0, 25.0]) * BAR)[:, None] + np.zeros(2)[None, :]
    return vfp.VFPTable(vfp.PROD, 10, 0.0, "OIL", [flo, thp, [0.0], [0.0], [0.0]], values, "WOR", "GLR")

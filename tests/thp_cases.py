"""The case the THP tests share (CPU: test_std_wells_thp.py over the oracle; GPU: test_gpu_std_wells_thp.py): a 3 x 3 x 65 grid (cell =
i + 3 (j + 3 k), dz = 1 m), a small synthetic VFPPROD / VFPINJ pair made so that the limits bind, and the switching table.

Wells: P65, a producer of 65 completions (the THP row sits behind a second pass of the per-well sums) with a THP limit; W3, a water
injector of three completions with a THP limit; P2, a producer without one.  The connection factors of P65 are scaled down so that its
drawdown is bars, not millibars, and a tubing-head pressure of a few bars more or less changes its rate.

VFPPROD 5 (LIQ / WCT / GOR, datum 2490 m): bhp = thp + 170 bar + 0.1 bar per m3/day + 5e-4 bar per (m3/day)^2 + 20 bar * wct - 0.01 bar * gor,
sampled on axes that leave every point of the tests inside or a little outside the table.  At P65's target (40 m3/day of oil, GOR about 265)
that is thp + 172 bar: its solved BHP of about 235 bar means a tubing-head pressure of about 63 bar, so a limit of 70 bar binds.
VFPINJ 7 (WAT, datum 2490 m): bhp = thp + 240 bar - 0.05 bar per m3/day.  W3's solved BHP of about 255 bar at 60 m3/day means about 17 bar
at the tubing head: an upper limit of 15 bar binds."""
import numpy as np

DAY, BAR = 86400.0, 1e5
PROD_LIMIT, INJ_LIMIT = 70.0 * BAR, 15.0 * BAR
PROD_BHP_LIMIT, INJ_BHP_LIMIT = 200.0 * BAR, 400.0 * BAR


def make_case(pkg, ext=False):
    """ext: a fluid with pc_scaling - the extended (19-field) intensive-quantity record"""
    if ext:
        import helpers
        return helpers.hysteresis_case(pkg, 3, 3, 65, heterogeneous=True, dz=1.0)
    return pkg.decks.cartesian_case(3, 3, 65, state="mixed", heterogeneous=True, dz=1.0)


def column(i, j, ks):
    return [i + 3 * (j + 3 * k) for k in ks]


def tables(pkg):
    vfp = pkg.vfp
    flo = np.array([0.0, 10.0, 30.0, 60.0, 120.0])
    thp = np.array([20.0, 50.0, 100.0, 150.0])
    wct = np.array([0.0, 0.5, 1.0])
    gor = np.array([0.0, 200.0, 400.0, 1000.0])
    t, w, g, f = np.meshgrid(thp, wct, gor, flo, indexing="ij")
    values = (t + 170.0 + 0.1 * f + 5e-4 * f * f + 20.0 * w - 0.01 * g)[:, :, :, None, :] * BAR
    prod = vfp.VFPTable(vfp.PROD, 5, 2490.0, "LIQ", [flo / DAY, thp * BAR, wct, gor, [0.0]], values, "WCT", "GOR")
    qi = np.array([0.0, 20.0, 50.0, 100.0])
    ti = np.array([5.0, 20.0, 60.0])
    tt, qq = np.meshgrid(ti, qi, indexing="ij")
    inj = vfp.VFPTable(vfp.INJ, 7, 2490.0, "WAT", [qi / DAY, ti * BAR], (tt + 240.0 - 0.05 * qq) * BAR)
    return [prod, inj]


def make_wells(pkg, case, limits=True):
    """limits=False: the same wells without THP limits"""
    W = pkg.wells

    def well(name, cells, producer, control, limit, inj=None, scale=1.0, **kw):
        tw = [scale * W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]
        return W.Well(name, cells, tw, case["depth"][cells[0]], producer, control, limit, inj_phase=inj, **kw)
    p = dict(thp_limit=PROD_LIMIT, vfp_table=5) if limits else {}
    i = dict(thp_limit=INJ_LIMIT, vfp_table=7) if limits else {}
    return [well("P65", column(0, 0, range(65)), True, ("rate", W.OIL, 40.0 / DAY), PROD_BHP_LIMIT, scale=0.02, **p),
            well("W3", column(2, 2, [10, 11, 12]), False, ("rate", W.WATER, 60.0 / DAY), INJ_BHP_LIMIT, "water", **i),
            well("P2", column(1, 1, [30, 31]), True, ("rate", W.OIL, 2.0 / DAY), PROD_BHP_LIMIT)]


def transitions(x_solved):
    """The switching table, one forced state per transition: (name, well, control before, x of that well, control after).  x_solved: the
    well unknowns after the wells alone under their rate targets (rates at the targets, BHP about 240 / 255 bar)."""
    p, w = x_solved[0].copy(), x_solved[1].copy()

    def state(x, bhp, rate_factor=1.0):
        y = x.copy()
        y[:3] *= rate_factor
        y[3] = bhp
        return y
    return [("producer rate -> thp", 0, "rate", p, "thp"),
            ("producer bhp -> thp", 0, "bhp", state(p, PROD_BHP_LIMIT, 0.5), "thp"),
            ("producer thp -> bhp", 0, "thp", state(p, PROD_BHP_LIMIT - 10.0 * BAR, 0.5), "bhp"),
            ("producer thp -> rate", 0, "thp", state(p, 245.0 * BAR, 1.5), "rate"),
            ("producer, bhp and thp both violated -> bhp", 0, "rate", state(p, PROD_BHP_LIMIT - 10.0 * BAR, 0.5), "bhp"),
            ("producer stays under thp", 0, "thp", state(p, 245.0 * BAR, 0.5), "thp"),
            ("producer stays under rate: its thp is above the limit", 0, "rate", state(p, 246.0 * BAR, 0.9), "rate"),
            ("injector rate -> thp", 1, "rate", w, "thp"),
            ("injector bhp -> thp", 1, "bhp", state(w, INJ_BHP_LIMIT, 0.5), "thp"),
            ("injector thp -> bhp", 1, "thp", state(w, INJ_BHP_LIMIT + 10.0 * BAR, 0.5), "bhp"),
            ("injector thp -> rate", 1, "thp", state(w, 252.0 * BAR, 1.5), "rate"),
            ("injector, bhp and thp both violated -> bhp", 1, "rate", state(w, INJ_BHP_LIMIT + 10.0 * BAR, 0.5), "bhp"),
            ("injector stays under thp", 1, "thp", state(w, 252.0 * BAR, 0.5), "thp")]


def control_of(well, name):
    return dict(rate=well.rate_control, bhp=("bhp", well.bhp_limit), thp=("thp", well.thp_limit))[name]

"""The cases the rate-limit tests share (tests/test_std_wells_limits.py, on the CPU over the oracle): the 3 x 3 x 65 grid, the wells' geometry
and the VFP tables of tests/thp_cases.py, with producers and an injector that carry several rate limits at once."""
import numpy as np

import thp_cases

DAY, BAR = 86400.0, 1e5
NEVER = 1e9                     # a finite limit no state of these tests violates
ALWAYS = 3e-15                  # ... every flowing state violates
PRODUCER_ORDER = ("bhp", "orat", "wrat", "grat", "lrat", "resv", "thp")      # wells/WellInterfaceFluidSystem.cpp:170-268
INJECTOR_ORDER = ("bhp", "rate", "resv", "thp")                              # :100-166


def tw_of(pkg, case, cells, scale=1.0):
    return [scale * pkg.wells.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15) for c in cells]


def producer(pkg, case, control, limits, use_list_target=True, own=None, thp_limit=None, cells=None, scale=0.02, name="P65"):
    """the long producer of thp_cases; own: its own rate target (default 40 m3/day of oil)"""
    W = pkg.wells
    cells = thp_cases.column(0, 0, range(65)) if cells is None else cells
    own = ("rate", W.OIL, 40.0 / DAY) if own is None else own
    kw = dict(thp_limit=thp_limit, vfp_table=5) if thp_limit is not None else {}
    return W.Well(name, cells, tw_of(pkg, case, cells, scale), case["depth"][cells[0]], True, own if control is None else control, thp_cases.PROD_BHP_LIMIT,
                  limits=limits, use_list_target=use_list_target, rate_control=own, **kw)


def injector(pkg, case, control, limits, use_list_target=True, thp_limit=None):
    W = pkg.wells
    cells = thp_cases.column(2, 2, [10, 11, 12])
    own = ("rate", W.WATER, 60.0 / DAY)
    kw = dict(thp_limit=thp_limit, vfp_table=7) if thp_limit is not None else {}
    return W.Well("W3", cells, tw_of(pkg, case, cells), case["depth"][cells[0]], False, own if control is None else control, thp_cases.INJ_BHP_LIMIT,
                  inj_phase="water", limits=limits, use_list_target=use_list_target, rate_control=own, **kw)


def control_of(well, name):
    if name in well.limits:
        return (name, well.limits[name])
    return dict(rate=well.rate_control, bhp=("bhp", well.bhp_limit), thp=("thp", well.thp_limit))[name]


def ordered_pair_well(pkg, case, order, first, second, in_force):
    """a well of `order` whose limits `first` and `second` (adjacent in that order) are violated by any flowing state on the right side of
    the BHP limit's other side, every other limit is not; `in_force`: the control it is under.  Returns (well, bhp that makes the BHP limit
    violated or not as the pair asks)"""
    is_prod = order is PRODUCER_ORDER
    hit = {first, second}
    own_kind = "orat" if is_prod else "rate"
    lim = {k: (ALWAYS if k in hit else NEVER) for k in order if k not in ("bhp", "thp", own_kind)}
    own_target = ALWAYS if own_kind in hit else NEVER
    if is_prod:
        thp = 1e9 if "thp" in hit else 1.0          # a producer's lower limit: violated when the limit > the tubing-head pressure at hand
        w = producer(pkg, case, None, lim, own=("rate", pkg.wells.OIL, own_target), thp_limit=thp)
        bhp = thp_cases.PROD_BHP_LIMIT + (-10.0 if "bhp" in hit else 40.0) * BAR
    else:
        thp = 1.0 if "thp" in hit else 1e9          # an injector's upper limit
        w = injector(pkg, case, None, lim, thp_limit=thp)
        w.rate_control = ("rate", pkg.wells.WATER, own_target)
        bhp = thp_cases.INJ_BHP_LIMIT + (10.0 if "bhp" in hit else -140.0) * BAR
    w.control = control_of(w, in_force if in_force != own_kind else "rate")
    return w, bhp

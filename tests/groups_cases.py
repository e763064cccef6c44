"""The cases the group-control GPU tests share (tests/test_gpu_std_wells_groups.py): the SPE9-shaped list in three groups and the 70
single-perforation producers in five."""
import numpy as np


def spe9_groups(pkg):
    """(groups, assign): three production groups on the 25 producers of decks.spe9_shaped_wells - producer n (list position n + 1) in group
    n % 2, except n == 5 alone in group 2 and n == 24 directly under FIELD: a group's wells are interleaved in list order, not contiguous.
    The targets lie below what the groups' wells produce at the case's state - a liquid rate, a voidage rate and an oil rate: the three
    groups leave NONE for different modes.  The guide rates differ from well to well."""
    W, S = pkg.wells, pkg.decks.STB_PER_DAY
    groups = [W.Group("G1", {"lrat": 12 * 900.0 * S, "orat": 1e9}), W.Group("G2", {"resv": 11 * 1100.0 * S, "wrat": 1e9}), W.Group("G3", {"orat": 700.0 * S, "grat": 1e9})]

    def assign(wells):
        for n, w in enumerate(wells[1:]):
            w.group = None if n == 24 else (2 if n == 5 else n % 2)
            w.guide_rate = np.full(5, 1.0 + 0.25 * (n % 3))
        wells[0].group = 0                    # the injector names a group and is ignored by it
        return wells
    return groups, assign


def seventy_producers(pkg, case):
    """70 producers of one perforation each on a 6 x 6 x 3 grid, every one in its own cell, in five groups by list position modulo 5: each
    group's wells straddle lane 63 / 64 of a one-lane-per-well kernel.  Own oil targets out of reach, so that they start at their BHP
    limit; a LRAT target per group below what its wells produce."""
    W = pkg.wells
    wells = []
    for n in range(70):
        c = n                                 # cells 0 .. 69 of 108: the two upper layers
        tw = [W.peaceman_factor(case["perm"][c], case["dx"], case["dy"], case["dz"], 0.15)]
        w = W.Well("P%02d" % n, [c], tw, case["depth"][c], True, ("bhp", 150e5), 150e5, rate_control=("rate", W.OIL, 1e9), group=n % 5,
                   guide_rate=[1.0 + (n % 4), 1.0, 1.0, 1.0 + (n % 3), 1.0])
        wells.append(w)
    return wells

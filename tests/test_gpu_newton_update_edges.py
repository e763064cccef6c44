"""k_newton_update (the chopped Newton update and the primary-variable switch) at its edges.  Every update here is made
three times - on the device, on the CPU oracle and by the numpy statement of tests/newton_ref.py - and the three agree
exactly: primary variables, meanings, the returned switch count, and (device against oracle) the intensive quantities.
The numpy statement also says which branch every cell took, so each test can show that it reached what it is about."""
import numpy as np
import pytest

import helpers
import newton_ref
import oracle_bind
from newton_ref import BRANCHES, SW_PO_RS, SW_PO_SG

pytestmark = pytest.mark.gpu


class Trio:
    """one state on the device, on the oracle and in numpy"""

    def __init__(self, pkg, orc, case, pv=None, meaning=None):
        self.case = case
        self.rs_sat = lambda p: pkg.decks.rs_sat(case["fluid"], p)
        self.m = pkg.capi.HipModel(case, reorder="graph_coloring_greedy")
        self.o = oracle_bind.OracleModel(orc, case)
        self.set_state(case["pv"] if pv is None else pv, case["meaning"] if meaning is None else meaning)

    def set_state(self, pv, meaning):
        self.pv, self.mng = np.array(pv, np.float64).reshape(-1, 3), np.array(meaning, np.uint8)
        self.flags = np.zeros(len(self.mng), np.uint8)
        for q in (self.m, self.o):
            q.set_state(self.pv.reshape(-1), self.mng)

    def update(self, dx, relax=1.0):
        """-> (switch count, labels, margin) of the numpy statement, after the device and the oracle were seen to agree with it"""
        dx = np.ascontiguousarray(dx, np.float64).reshape(-1, 3)
        pv, mng, flags, n, lab, margin = newton_ref.update(self.pv, self.mng, self.flags, dx, relax, self.rs_sat, self.case.get("rsmax"))
        assert np.all((margin == 0.0) | (margin >= 1e-9)), margin[(margin > 0) & (margin < 1e-9)]   # (the generator's duty, not the device's)
        n_m = self.m.update(dx.reshape(-1), relax)
        n_o = self.o.update((dx if relax == 1.0 else dx * relax).reshape(-1))      # the oracle takes the relaxed update ready-made
        pm, mm = self.m.get_state()
        po, mo = self.o.get_state()
        bad = np.flatnonzero((pm.reshape(-1, 3) != pv).any(axis=1) | (mm != mng))
        assert bad.size == 0, (bad[:8], pm.reshape(-1, 3)[bad[:8]], pv[bad[:8]], [BRANCHES[b] for b in lab["branch"][bad[:8]]])
        assert np.array_equal(po.reshape(-1, 3), pv) and np.array_equal(mo, mng)
        assert n_m == n and n_o == n
        assert np.array_equal(self.m.iq(), self.o.iq())
        self.pv, self.mng, self.flags = pv, mng, flags
        return n, lab, margin


def rocktab_fluid(pkg):
    """the SPE1 fluid with ROCKTAB: the extended record without wet gas, so k_newton_update<true> takes its Sw_po_Rs arm"""
    fl = pkg.fluid.spe1_fluid()[0]
    return pkg.fluid.Fluid(fl.pvt, fl.sat, rock_pref=fl.rock_pref, rock_cr=fl.rock_cr, rocktab=helpers.ROCKTAB_2)


@pytest.mark.parametrize("layout", ["plain", "rocktab"])
def test_census_run(pkg, orc, layout):
    """four successive updates of the 9 x 8 x 7 case of tests/test_newton_ref.py; every branch label is met by 8 cells or more"""
    case = newton_ref.census_case(pkg, fluid=rocktab_fluid(pkg) if layout == "rocktab" else None)
    if layout == "rocktab":
        case["rocknum"] = (np.arange(case["Nb"]) % 2).astype(np.int32)
        case["overburden"] = 20e5 + 50.0 * (case["depth"] - case["depth"].min())
    t = Trio(pkg, orc, case)
    assert t.m.iq().shape[1] == (19 if layout == "rocktab" else 17)
    rng = np.random.default_rng(5)
    labels = []
    for step in range(4):
        dx = newton_ref.census_dx(rng, t.pv, t.mng, t.flags, t.rs_sat)
        labels.append(t.update(dx)[1])
    n = newton_ref.census_counts(labels)
    assert all(v >= 8 for v in n.values()), n


def test_exact_edges(pkg, orc):
    """one cell per edge, with binary-exact numbers so that both sides of the comparison are the same double"""
    case = pkg.decks.cartesian_case(1, 1, 10, state="mixed", perturb=False)
    p = 1.25 * 2.0 ** 24                                  # 0.3 p = 0.375 * 2^24 without rounding
    assert 0.3 * p == 0.375 * 2.0 ** 24
    rows = [  # meaning, Sw, x[2], dx
        (SW_PO_RS, 0.875, 64.0, (-0.125, 0.0, 0.0)),      # 0 Sw lands on 1.0: >= takes it, water only
        (SW_PO_SG, 0.875, 0.0625, (-0.125, 0.0, 0.0)),    # 1 the same from Sg
        (SW_PO_SG, 0.5, 0.25, (0.25, 0.0, 0.0)),          # 2 largest saturation delta 0.25: chopped by 0.2 / 0.25
        (SW_PO_SG, 0.5, 0.25, (0.2, 0.0, 0.0)),           # 3 largest saturation delta exactly 0.2: no chop
        (SW_PO_RS, 0.5, 64.0, (0.0, 0.3 * p, 0.0)),       # 4 |dp| == 0.3 p: no chop
        (SW_PO_RS, 0.5, 64.0, (0.0, -0.3 * p, 0.0)),      # 5 the same downwards
        (SW_PO_RS, 0.5, 64.0, (0.0, 0.0, 64.0)),          # 6 Rs delta == Rs: > leaves it alone, the result is +0.0
        (SW_PO_RS, 0.5, 64.0, (0.0, 0.0, 96.0)),          # 7 Rs delta above Rs: clamped, 0
        (SW_PO_RS, 0.5, 64.0, (0.0, -0.5 * p, 0.0)),      # 8 a negative pressure delta beyond the chop: p + 0.3 p
        (SW_PO_SG, 0.5, 0.125, (0.0, 0.0, 0.125)),        # 9 Sg lands on 0.0: < -eps (eps = 0) leaves the gas phase in place
    ]
    pv = np.array([[r[1], p, r[2]] for r in rows])
    mng = np.array([r[0] for r in rows], np.uint8)
    dx = np.array([r[3] for r in rows])
    t = Trio(pkg, orc, case, pv, mng)
    n, lab, margin = t.update(dx)
    assert np.all(margin[[0, 1, 3, 4, 5, 6, 9]] == 0.0)      # the comparisons that decide were between equal doubles
    assert [BRANCHES[b] for b in lab["branch"][:2]] == ["water_only_from_rs", "water_only_from_sg"] and n == 1
    assert lab["sat_chop"].tolist() == [False, False, True] + [False] * 7
    assert lab["p_chop"].tolist() == [0] * 8 + [-1, 0]
    assert lab["rs_clamp"].tolist() == [False] * 7 + [True, False, False]
    got = t.m.get_state()[0].reshape(-1, 3)
    assert got[0].tolist() == [1.0, p, 0.0] and got[1].tolist() == [1.0, p, 0.0]
    assert got[2, 0] == 0.5 - 0.25 * (0.2 / 0.25) and got[3, 0] == 0.5 - 0.2
    assert got[4, 1] == p - 0.3 * p and got[5, 1] == p + 0.3 * p and got[8, 1] == p + 0.3 * p
    assert got[6, 2] == 0.0 and not np.signbit(got[6, 2]) and got[7, 2] == 0.0 and not np.signbit(got[7, 2])
    assert got[9, 2] == 0.0 and t.mng[9] == SW_PO_SG and BRANCHES[lab["branch"][9]] == "stays"


@pytest.mark.parametrize("relax", [0.5, 0.9])
def test_relaxed_update(pkg, orc, relax):
    """opmhip_update(dx, relax): the relaxed update dx * relax is formed first and then chopped.  With relax < 1 the relaxed form
    of an update can only lose a chop, never gain one, so the cells are of three kinds: chopped unrelaxed and not relaxed
    (saturation and pressure), chopped either way, chopped neither way - each kind seen"""
    case = newton_ref.census_case(pkg)
    t = Trio(pkg, orc, case)
    rng = np.random.default_rng(23)
    dx = newton_ref.census_dx(rng, t.pv, t.mng, t.flags, t.rs_sat)
    dx[::5, 0] = 0.21                                     # 0.21 is chopped, 0.9 * 0.21 and 0.5 * 0.21 are not
    dx[::5, 2] = 0.0
    dx[1::5, 1] = 0.32 * t.pv[1::5, 1]
    plain = newton_ref.update(t.pv, t.mng, t.flags, dx, 1.0, t.rs_sat)[4]
    n, lab, margin = t.update(dx, relax)
    for key in ("sat_chop", "p_chop"):
        a, b = plain[key] != 0, lab[key] != 0
        assert (a & ~b).sum() >= 8 and (a & b).sum() >= 8 and (~a & ~b).sum() >= 8 and not (~a & b).any(), (key, a.sum(), b.sum())
    t.update(newton_ref.census_dx(rng, t.pv, t.mng, t.flags, t.rs_sat), relax)   # and once more, with flags set


def test_rsmax_caps_both_switches(pkg, orc):
    """RsMax below, at and above the saturated value: gas appears at min(RsMax, RsSat (1 + eps)); a cell whose gas disappears
    receives min(RsMax, RsSat).  The cells with RsMax == RsSat(p) keep their pressure, so that the two stay one double"""
    case = newton_ref.census_case(pkg)
    p0 = case["pv"].reshape(-1, 3)[:, 1]
    kind = np.arange(case["Nb"]) % 3
    case["rsmax"] = np.array([0.6, 1.0, 1.4])[kind] * pkg.decks.rs_sat(case["fluid"], p0)
    t = Trio(pkg, orc, case)
    rng = np.random.default_rng(29)
    seen = {}
    for step in range(2):
        dx = newton_ref.census_dx(rng, t.pv, t.mng, t.flags, t.rs_sat)
        dx[kind == 1, 1] = 0.0
        was = t.mng.copy()
        n, lab, margin = t.update(dx)
        gone = lab["branch"] == BRANCHES.index("gas_disappears")
        rs_new = t.m.get_state()[0].reshape(-1, 3)[:, 2]
        assert np.array_equal(rs_new[gone], np.minimum(case["rsmax"], t.rs_sat(t.pv[:, 1]))[gone])
        for k in range(3):
            seen[(k, "receives the cap")] = seen.get((k, "receives the cap"), 0) + int((gone & (kind == k) & (rs_new == case["rsmax"])).sum())
            for b in ("gas_disappears", "gas_appears", "stays"):
                seen[(k, b)] = seen.get((k, b), 0) + int(((lab["branch"] == BRANCHES.index(b)) & (kind == k) & (was == SW_PO_RS if b != "gas_disappears" else was == SW_PO_SG)).sum())
    above = seen.pop((2, "receives the cap"))             # (RsMax = 1.4 RsSat binds only where the pressure rose a good deal)
    assert all(v >= 8 for v in seen.values()), (seen, above)


def band_case(pkg):
    """a state made for the oscillation band: Sw 0.3, Sg 0.1 in the gas cap, Rs 0.8 RsSat below; update 1 makes the even cells
    switch (the set S), each in its direction, and leaves the pressure alone"""
    case = pkg.decks.cartesian_case(9, 8, 7, state="mixed")
    pv = case["pv"].reshape(-1, 3).copy()
    gas = case["meaning"] == SW_PO_SG
    sat = pkg.decks.rs_sat(case["fluid"], pv[:, 1])
    pv[:, 0] = 0.3
    pv[:, 2] = np.where(gas, 0.1, 0.8 * sat)
    case["pv"] = np.ascontiguousarray(pv.reshape(-1))
    S = np.arange(case["Nb"]) % 2 == 0
    dx1 = np.zeros((case["Nb"], 3))
    dx1[S, 2] = np.where(gas, 0.11, -0.3 * sat)[S]        # Sg -> -0.01 ; Rs -> 1.1 RsSat
    return case, S, dx1


def band_move(t, cells):
    """the move of update 2: the cells named go to Rs = RsSat (1 + 5e-6) or to Sg = -5e-6, the pressure is left alone"""
    half = 0.5 * newton_ref.OSC_THRESHOLD
    dx = np.zeros((len(t.mng), 3))
    x2, sat = t.pv[:, 2], t.rs_sat(t.pv[:, 1])
    dx[cells, 2] = np.where(t.mng == SW_PO_SG, x2 + half, x2 - sat * (1.0 + half))[cells]
    return dx


def test_oscillation_band(pkg, orc):
    """a cell that switched in the update before switches back only beyond 1e-5: three updates"""
    case, S, dx1 = band_case(pkg)
    t = Trio(pkg, orc, case)
    every = np.ones(case["Nb"], bool)
    n1, lab1, _ = t.update(dx1)
    assert n1 == S.sum() and np.array_equal(t.flags != 0, S)
    assert (lab1["branch"][S] == BRANCHES.index("gas_disappears")).sum() >= 8 and (lab1["branch"][S] == BRANCHES.index("gas_appears")).sum() >= 8
    # update 2 moves S and as many cells that did not switch; S stays inside the band, the others switch
    sg_of_S = S & (t.mng == SW_PO_SG)
    n2, lab2, _ = t.update(band_move(t, every))
    assert n2 == (~S).sum() and np.all(lab2["branch"][S] == BRANCHES.index("stays_band")) and np.array_equal(t.flags != 0, ~S)
    got = t.m.get_state()[0].reshape(-1, 3)
    assert np.all(got[sg_of_S, 2] < 0.0) and sg_of_S.sum() >= 8
    # update 3 repeats the move for the cells that stayed: their flag is gone, they switch
    n3, lab3, _ = t.update(band_move(t, S))
    assert n3 == S.sum() and np.array_equal(t.flags != 0, S)


@pytest.mark.parametrize("how", ["set_state", "update_failed", "advance_time_level"])
def test_lifecycle_of_the_switch_flags(pkg, orc, how):
    """pins the present behaviour: opmhip_set_state and opmhip_update_failed clear the flags the oscillation band reads,
    opmhip_advance_time_level keeps them - after the first two the move of update 2 switches every cell, after the third the
    cells that switched in update 1 still stay.  The oracle does the same (its flags are cleared by set_state alone).
    UNVERIFIED against upstream: the reference's BlackoilModelEbos::prepareStep (flow/BlackoilModelEbos.hpp:250-252) fills a
    flag vector of its own, wasSwitched_, with false at every time step; whether that vector is the one
    adaptPrimaryVariables' caller reads is decided in opm-models, which the reference tree does not hold."""
    case, S, dx1 = band_case(pkg)
    t = Trio(pkg, orc, case)
    every = np.ones(case["Nb"], bool)
    t.update(dx1)
    if how == "set_state":
        t.set_state(t.pv, t.mng)
    elif how == "update_failed":
        t.m.advance_time_level()
        t.m.update_failed()                       # back to the level just kept: the same state, the flags cleared
        t.o.set_state(t.pv.reshape(-1), t.mng)
        t.flags[:] = 0
        assert np.array_equal(t.m.get_state()[0].reshape(-1, 3), t.pv)
    else:
        t.m.advance_time_level()
    n2, lab2, _ = t.update(band_move(t, every))
    assert n2 == ((~S).sum() if how == "advance_time_level" else case["Nb"])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sizes_around_one_workgroup(pkg, orc, n):
    case = newton_ref.census_case(pkg, 1, 1, n, seed=n)
    t = Trio(pkg, orc, case)
    rng = np.random.default_rng(100 + n)
    for step in range(2):
        t.update(newton_ref.census_dx(rng, t.pv, t.mng, t.flags, t.rs_sat))
    if n > 1:
        assert (t.mng != case["meaning"]).any()

"""wells.StandardWells(arithmetic="stated") - the well equations in an order a kernel can follow, the comparator of the device-resident
wells (tests/test_gpu_std_wells_device.py) - against the NumPy form it restates, on the CPU over the oracle.

Measured here (numpy 2.2.6), stated against NumPy form on one state, largest relative difference; the tests assert 100 x these (the margin
allows for D's condition number growing during a run; cond(D) is 2e9 / 6e8 on these states) and equality where the measured value is 0:

                          decks.spe9_shaped_wells     decks.spe1_wells
    r_w                   2.9e-15                     0
    D^-1, per row         2.9e-16                     9.0e-17
    D^-1, per entry       3.1e-16                     0
    B, C                  0                           0
    source, dsource       0                           0
    x after the wells alone (solve_well_equations)
                          3.4e-16                     0

Entries are compared one by one, relative to the larger of the two, except D^-1: an entry of D^-1 that is a cancelled 1 - 1 (1e-16 beside
entries of 1 and 1e8) has no relative accuracy of its own in either form, so D^-1 is compared relative to the largest |entry| of its row
- and, so that a wrong small-but-meaningful entry cannot hide behind a 1e8 neighbour, entry by entry on every entry above that row's
rounding floor of 16 eps x its largest |entry| (230 of 256 non-zero entries on SPE9's wells, 12 of 14 on SPE1's).
(SPE1's wells have one completion each: no sum to reorder.)"""
import numpy as np
import pytest

import oracle_bind

MEASURED = {"spe9": dict(res_well=2.9e-15, Dinv=2.9e-16, Dinv_entries=3.1e-16, B=0.0, C=0.0, source=0.0, dsource=0.0, solved_x=3.4e-16),
            "spe1": dict(res_well=0.0, Dinv=9.0e-17, Dinv_entries=0.0, B=0.0, C=0.0, source=0.0, dsource=0.0, solved_x=0.0)}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    d, s = np.abs(a - b), np.maximum(np.abs(a), np.abs(b))
    m = s > 0
    return float((d[m] / s[m]).max()) if m.any() else 0.0


def rel_rows(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float((np.abs(a - b) / np.abs(a).max(axis=-1, keepdims=True)).max())


def rel_entries_above_the_floor(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    m = np.abs(a) > 16 * np.finfo(float).eps * np.abs(a).max(axis=-1, keepdims=True)
    assert 3 * m.sum() > 2 * np.count_nonzero(a)
    return float((np.abs(a - b)[m] / np.abs(a)[m]).max())


@pytest.fixture(scope="module")
def decks(pkg, orc):
    spe9 = pkg.decks.cartesian_case(24, 25, 15, dx=91.44, dy=91.44, dz=6.0, heterogeneous=True, state="mixed")
    spe1 = pkg.decks.spe1_case(props=oracle_bind.OracleFluid(orc, pkg.fluid.spe1_fluid()[0]))
    out = {}
    for name, case, make in (("spe9", spe9, pkg.decks.spe9_shaped_wells), ("spe1", spe1, pkg.decks.spe1_wells)):
        om = oracle_bind.OracleModel(orc, case)
        om.set_state(case["pv"], case["meaning"])
        out[name] = (case, make, om.iq())
    return out


def pair(pkg, case, make):
    return make(case), pkg.wells.StandardWells(make(case).wells, case["depth"], arithmetic="stated")


@pytest.mark.parametrize("name", ["spe9", "spe1"])
def test_stated_form_against_the_numpy_form(pkg, decks, name):
    case, make, iq = decks[name]
    wn, ws = pair(pkg, case, make)
    assert wn.arithmetic == "numpy" and ws.arithmetic == "stated"
    wn.solve_well_equations(iq)
    ws.solve_well_equations(iq)
    got = dict(solved_x=rel(wn.x, ws.x))
    # one state for both, away from the solved one: the residuals are not zero
    x0 = wn.x.copy()
    x0[:, :3] *= 1.02
    x0[:, 3] += np.where([w.producer for w in wn.wells], -2e5, 3e5)
    wn.x, ws.x = x0.copy(), x0.copy()
    an, a_s = wn.assemble(iq), ws.assemble(iq)
    got["res_well"] = rel(an["res_well"], a_s["res_well"])
    got["Dinv"] = rel_rows(an["wells"]["Dnnzs"].reshape(-1, 4, 4), a_s["wells"]["Dnnzs"].reshape(-1, 4, 4))
    got["Dinv_entries"] = rel_entries_above_the_floor(an["wells"]["Dnnzs"].reshape(-1, 4, 4), a_s["wells"]["Dnnzs"].reshape(-1, 4, 4))
    got["B"], got["C"] = rel(an["wells"]["Bnnzs"], a_s["wells"]["Bnnzs"]), rel(an["wells"]["Cnnzs"], a_s["wells"]["Cnnzs"])
    got["source"], got["dsource"] = rel(an["source_cells"], a_s["source_cells"]), rel(an["dsource_cells"], a_s["dsource_cells"])
    print(name, "stated against numpy:", {k: "%.2e" % v for k, v in got.items()})
    assert 2 * np.count_nonzero(an["res_well"]) > an["res_well"].size and np.any(an["source_cells"] != 0.0)
    for k, v in got.items():
        bound = 100.0 * MEASURED[name][k]
        assert v <= bound, (k, v, bound)          # a measured 0 asks for equality


def test_invert4_stated(pkg, decks):
    """D D^-1 = I to 16 eps cond(D) on the D matrices of the two cases and on a row-scaled one; a singular D is reported"""
    inv = pkg.wells.invert4_stated
    eps = np.finfo(float).eps
    mats = []
    for name in ("spe9", "spe1"):
        case, make, iq = decks[name]
        w = make(case)
        w.solve_well_equations(iq)
        _, D, *_ = w._assemble_wells(iq)
        mats += list(D)
    mats.append(np.diag([1.0, 1e7, 1e-5, 3.0]) @ mats[1])          # row-scaled: the pivot search has something to choose
    mats.append(mats[1][[3, 0, 1, 2]])                             # and rows out of order
    for D in mats:
        Di = inv(D)
        err = np.abs(D @ Di - np.eye(4)).max()
        assert err <= 16 * eps * np.linalg.cond(D), (err, np.linalg.cond(D))
    assert np.array_equal(inv(np.eye(4)), np.eye(4))
    # ties go to the lowest row: rows 0 and 3 are equal in column 0, row 0 stays the pivot row and column 3 ends without a pivot
    S = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, -2e-9], [0, 0, 1.0, 0], [1.0, 0, 0, 0]])
    with pytest.raises(pkg.wells.SingularWellEquations) as e:
        inv(S)
    assert e.value.column == 3
    with pytest.raises(pkg.wells.SingularWellEquations) as e:
        inv(np.zeros((4, 4)))
    assert e.value.column == 0
    with pytest.raises(ValueError):
        pkg.wells.StandardWells([], [], arithmetic="fast")


def test_loop_sums_of_a_long_and_a_short_well(pkg):
    """a well of 150 perforations and one of 1: the per-well sums of the stated form carry the bits of a plain left-to-right loop (this
    guards the order, not the accuracy) - and np.add.reduceat, which reduces pairwise, does not"""
    rng = np.random.default_rng(7)
    a = rng.standard_normal((151, 3)) * 10.0 ** rng.integers(-6, 3, (151, 3))
    vp = np.array([0, 150, 151], np.int32)
    got = pkg.wells.sequential_sums(a, vp)
    want = np.zeros((2, 3))
    for k in range(2):
        for c in range(3):
            s = float(a[vp[k], c])
            for j in range(int(vp[k]) + 1, int(vp[k + 1])):
                s = s + float(a[j, c])
            want[k, c] = s
    assert np.array_equal(got, want) and np.array_equal(got[1], a[150])
    assert not np.array_equal(np.add.reduceat(a, vp[:-1], axis=0), want)
    r = rng.standard_normal(4)
    M = rng.standard_normal((4, 4))
    assert np.array_equal(pkg.wells.row_times_vector(M, r), [((M[i, 0] * r[0] + M[i, 1] * r[1]) + M[i, 2] * r[2]) + M[i, 3] * r[3] for i in range(4)])
    # the same through the class: the 150-completion well's residual is x - (that loop's sum)
    W = pkg.wells
    wells = [W.Well("LONG", np.arange(150), np.ones(150), 0.0, True, ("rate", W.OIL, 1.0), 1e5), W.Well("ONE", [150], [1.0], 0.0, True, ("rate", W.OIL, 1.0), 1e5)]
    sw = W.StandardWells(wells, np.zeros(151), arithmetic="stated")
    pr = np.zeros((151, 3, 5))
    pr[:, :, 0], pr[:, :, 4] = a, a[::-1]
    sw._perf_rates = lambda iq, bhp: pr
    r_w, D, *_ = sw._assemble_wells(None)
    assert np.array_equal(r_w[:, :3], -want) and np.array_equal(D[0, :3, 3], -pkg.wells.sequential_sums(a[::-1], vp)[0])

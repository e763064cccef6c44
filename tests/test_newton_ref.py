"""The numpy statements of tests/newton_ref.py against the CPU oracle (no GPU): the chopped Newton update and the
primary-variable switch bit for bit over four successive updates that are seen to reach every branch, the convergence
numbers and the relative change to the rounding of a sequential sum.  The oracle's update() / adapt() carries the mark
"UNVERIFIED vs upstream" and is a sibling of the kernel; the numpy statement was written from the rules in SURVEY.md
App. B.7, so the three now hold one another."""
import math

import numpy as np
import pytest

import newton_ref
import oracle_bind

U = 2.0 ** -52


def run_census(pkg, orc, case, steps=4, seed=5):
    """the shared run: `steps` updates of the census case on the oracle and on the numpy statement, the update vectors drawn
    from the oracle's state -> per step (dx, oracle state, oracle count, numpy result)"""
    rs_sat = lambda p: pkg.decks.rs_sat(case["fluid"], p)
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    rng = np.random.default_rng(seed)
    pv, mng, flags = case["pv"].reshape(-1, 3), case["meaning"], np.zeros(case["Nb"], np.uint8)
    out = []
    for step in range(steps):
        dx = newton_ref.census_dx(rng, pv, mng, flags, rs_sat)
        ref = newton_ref.update(pv, mng, flags, dx, 1.0, rs_sat, case.get("rsmax"))
        n_o = o.update(dx.reshape(-1))
        pv_o, m_o = o.get_state()
        out.append(dict(dx=dx, pv_o=pv_o.reshape(-1, 3).copy(), m_o=m_o.copy(), n_o=n_o, ref=ref))
        pv, mng, flags = ref[0], ref[1], ref[2]
    return o, out


@pytest.fixture(scope="module")
def census(pkg, orc):
    case = newton_ref.census_case(pkg)
    o, steps = run_census(pkg, orc, case)
    return case, o, steps


def test_update_equals_the_oracle_bit_for_bit(census):
    case, o, steps = census
    for k, s in enumerate(steps):
        pv, mng, flags, n, lab, margin = s["ref"]
        assert np.all((margin == 0.0) | (margin >= 1e-9)), (k, margin[(margin > 0) & (margin < 1e-9)])
        assert n == s["n_o"], k
        assert np.array_equal(mng, s["m_o"]), k
        assert np.array_equal(pv, s["pv_o"]), (k, np.flatnonzero((pv != s["pv_o"]).any(axis=1)))
    assert np.isfinite(o.iq()).all()          # the run stays where the property tables are defined


def test_census_reaches_every_branch(census):
    case, o, steps = census
    n = newton_ref.census_counts([s["ref"][4] for s in steps])
    print(n)
    assert all(v >= 8 for v in n.values()), n
    assert len(n) == len(newton_ref.BRANCHES) + len(newton_ref.SAT_PHASES) + 6


def test_update_statement_at_hand_made_cells():
    """the rules once more on numbers small enough to do by hand (RsSat = 100 everywhere)"""
    sat = lambda p: 100.0
    SG, RS = newton_ref.SW_PO_SG, newton_ref.SW_PO_RS
    pv = np.array([[0.5, 1e7, 0.25], [0.875, 1e7, 50.0], [0.5, 1e7, 0.0625], [0.5, 1e7, 90.0], [0.5, 1e7, 50.0]])
    mng = np.array([SG, RS, SG, RS, RS], np.uint8)
    dx = np.array([[0.25, 5e6, 0.25],       # dSo = -0.5: chopped by 0.4; |dp| above 0.3 p: chopped to 3e6
                   [-0.125, -1e6, 75.0],    # Sw lands on 1.0: water only; (Rs delta clamped on the way)
                   [0.0, 0.0, 0.125],       # Sg -> -0.0625: the gas phase disappears, Rs = RsSat
                   [0.0, 0.0, -20.0],       # Rs -> 110 > 100: the gas phase appears
                   [0.0, 0.0, 50.0]])       # delta == Rs: not clamped, Rs -> +0.0
    out, m, fl, n, lab, margin = newton_ref.update(pv, mng, np.zeros(5, np.uint8), dx, 1.0, sat)
    assert out[0].tolist() == [0.5 - 0.25 * (0.2 / 0.5), 1e7 - 0.3 * 1e7, 0.25 - 0.25 * (0.2 / 0.5)] and m[0] == SG
    assert out[1].tolist() == [1.0, 1.1e7, 0.0] and m[1] == SG and lab["rs_clamp"][1]
    assert out[2].tolist() == [0.5, 1e7, 100.0] and m[2] == RS
    assert out[3].tolist() == [0.5, 1e7, 0.0] and m[3] == SG
    assert out[4].tolist() == [0.5, 1e7, 0.0] and m[4] == RS and not lab["rs_clamp"][4] and margin[4] == 0.0
    assert n == 3 and fl.tolist() == [0, 1, 1, 1, 0]
    assert [newton_ref.BRANCHES[b] for b in lab["branch"]] == ["stays", "water_only_from_rs", "gas_disappears", "gas_appears", "stays"]
    # the band: the cells that switched stay for a step of 5e-6 past the threshold, and switch once the flag is gone
    dx2 = np.zeros((5, 3))
    dx2[2, 2] = 100.0 - 100.0 * (1.0 + 5e-6)
    dx2[3, 2] = 5e-6
    out2, m2, fl2, n2, lab2, _ = newton_ref.update(out, m, fl, dx2, 1.0, sat)
    assert n2 == 0 and m2[2] == RS and m2[3] == SG and out2[3, 2] == -5e-6
    assert [newton_ref.BRANCHES[b] for b in lab2["branch"][[2, 3]]] == ["stays_band", "stays_band"]
    out3, m3, fl3, n3, _, _ = newton_ref.update(out2, m2, fl2, np.zeros((5, 3)), 1.0, sat)
    assert n3 == 2 and m3[2] == SG and m3[3] == RS
    # relax: the relaxed update is formed first, then chopped; RsMax caps both directions
    quarter, _, _, _, labq, _ = newton_ref.update(pv, mng, np.zeros(5, np.uint8), dx, 0.25, sat)
    assert not labq["sat_chop"][0] and labq["p_chop"][0] == 0 and quarter[0].tolist() == [0.4375, 8.75e6, 0.1875]
    cap, mc, _, _, _, _ = newton_ref.update(pv, mng, np.zeros(5, np.uint8), dx, 1.0, sat, rs_max=np.full(5, 80.0))
    assert cap[2, 2] == 80.0 and mc[3] == SG and mc[4] == RS


def test_convergence_and_relative_change_against_the_oracle(pkg, census):
    """maxima are equal; a sum of the oracle's, taken sequentially over Nb terms, lies within Nb 2^-52 sum|x| of fsum (the
    bound of a sequential sum, (Nb - 1) u sum|x| to first order, with a factor 2 and more in hand)"""
    case, o, steps = census
    Nb, dt, tol = case["Nb"], 86400.0, 1e-2
    pv0, m0 = steps[1]["pv_o"], steps[1]["m_o"]
    _, r = o.assemble(dt, 0)
    co = o.convergence(dt, tol)
    inv_b = o.iq()[:, 6:9, 0]
    c, violated, dist = newton_ref.convergence(r, case["poro"], case["volume"], inv_b, dt, tol, b_avg=co[6:9])
    r = r.reshape(-1, 3)
    assert np.array_equal(co[3:6], c[3:6])
    assert np.all(np.abs(co[0:3] - c[0:3]) <= Nb * U * np.abs(r).sum(axis=0))
    for ph, e in enumerate(newton_ref.EQ_OF_PHASE):
        assert abs(co[6 + e] - c[6 + e]) <= Nb * U * math.fsum(1.0 / inv_b[:, ph]) / Nb
    pvv = case["poro"] * case["volume"]
    assert abs(co[9] - c[9]) <= Nb * U * pvv.sum()
    assert dist.min() >= 1e-9 and 0 < violated.sum()
    assert abs(co[10] - c[10]) <= Nb * U * pvv[violated].sum()
    # CNV and MB as the reference forms them from the oracle's own sums and averages
    assert np.array_equal(co[11:14], co[6:9] * dt * co[3:6])
    assert np.array_equal(co[14:17], np.abs(co[6:9] * co[0:3]) * dt / co[9])
    # the relative change of the last state against the state after the second update; every term is >= 0, so the bound on
    # each sum is relative and the ratio lies within twice that (plus the division's own rounding)
    pn, mn = o.get_state()
    delta, denom, ratio, d, q = newton_ref.relative_change(pn, mn, pv0, m0)
    assert (mn != m0).any() and ratio > 0.0
    assert abs(o.relative_change(pv0.reshape(-1), m0) - ratio) <= 3 * Nb * U * ratio
    assert o.relative_change(pn, mn) == 0.0 and newton_ref.relative_change(pn, mn, pn, mn)[2] == 0.0


def test_convergence_statement_drops_nan_from_the_maximum_only():
    """std::max(m, NaN) keeps m: a NaN residual shows in R_sum and MB of its component alone; an infinite one shows in both"""
    r = np.array([[1.0, -2.0, 0.5], [0.25, 4.0, -8.0], [2.0, 1.0, 1.0]])
    one, inv_b = np.ones(3), np.full((3, 3), 0.5)
    base, _, _ = newton_ref.convergence(r, one, one, inv_b, 2.0, 1.0)
    assert base[0:3].tolist() == [3.25, 3.0, -6.5] and base[3:6].tolist() == [2.0, 4.0, 8.0] and base[6:9].tolist() == [2.0] * 3
    assert base[11:14].tolist() == [8.0, 16.0, 32.0] and base[14:17].tolist() == [2.0 * 3.25 * 2 / 3, 2.0 * 3.0 * 2 / 3, 2.0 * 6.5 * 2 / 3]
    r2 = r.copy()
    r2[1, 1] = np.nan
    c, violated, _ = newton_ref.convergence(r2, one, one, inv_b, 2.0, 1.0)
    assert np.isnan(c[1]) and np.isnan(c[15]) and c[4] == 2.0 and c[12] == 8.0
    assert np.array_equal(c[[0, 2, 3, 5, 11, 13, 14, 16]], base[[0, 2, 3, 5, 11, 13, 14, 16]])
    assert newton_ref.failure(c) == "NaN residual found!" and newton_ref.failure(base) is None
    for v in (np.inf, -np.inf):
        r3 = r.copy()
        r3[2, 0] = v
        c, _, _ = newton_ref.convergence(r3, one, one, inv_b, 2.0, 1.0)
        assert c[0] == v and c[3] == np.inf and c[11] == np.inf and c[14] == np.inf
        assert newton_ref.failure(c) == "Too large residual found!"
    r3[0, 0] = np.inf                       # +inf and -inf in one component: the sum is NaN
    assert newton_ref.failure(newton_ref.convergence(r3, one, one, inv_b, 2.0, 1.0)[0]) == "NaN residual found!"

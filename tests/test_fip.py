"""Fluids in place and region pressures per FIP region on the CPU side (opm-autodiff_amd/fip.py): the arithmetic the device's
opmhip_fluid_in_place is compared with, pinned by the reference's own numbers (tests/test_ecl_output.cc:192-225, through
helpers.summary_deck_expectations), by an error bound that is derived and not measured, by a literal walk through the chunks of the
stated order, and by the region rules of regionSum / update / pressureAverage_."""
import math

import numpy as np
import pytest

import helpers
import oracle_bind
from test_oracle_ecl_output import check

U = 2.0 ** -53
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 513, 65537)   # the last needs three levels: 65 537 -> 257 -> 2 -> 1


def _records(orc, case):
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    return o.iq()


@pytest.fixture(scope="module")
def deck(pkg, orc):
    case, fipnum = helpers.summary_deck_case(pkg)
    return case, fipnum, pkg.fip.cell_terms(_records(orc, case), case["volume"], case["poro"])


def _metric(s):
    """the summary in the deck's units: pressures in bar (unit conversion is the caller's)"""
    return {k: (v / 1e5 if k.startswith(("FPR", "RPR")) else v) for k, v in s.items()}


@pytest.mark.parametrize("arithmetic", ["sequential", "stated"])
def test_summary_deck_meets_the_references_numbers(pkg, deck, arithmetic):
    case, fipnum, terms = deck
    got = _metric(pkg.fip.summary(pkg.fip.inplace(terms, fipnum, arithmetic)))
    check(got)
    assert set(helpers.summary_deck_expectations()) <= set(got)
    # region 3 exists beside the two the reference looks at; the field is the three regions' sum
    assert got["ROIP:3"] > 0.0 and got["FOIP"] == (got["ROIP:1"] + got["ROIP:2"]) + got["ROIP:3"]


def _check_bound(pkg, terms, region):
    """u = 2^-53: any order of additions of n terms lies within (n - 1) u sum |x_i| of the exact sum, to first order in u (the standard
    bound, whatever the order); math.fsum is the exact sum rounded once, another u |sum| <= u sum |x_i|: n u sum |x_i| in all.  Nothing
    is measured into it."""
    for arithmetic in ("sequential", "stated"):
        regions, field = pkg.fip.region_sums(terms, region, arithmetic)
        for r in range(regions.shape[0] + 1):
            m = (region == r + 1) if r < regions.shape[0] else (region >= 1)
            n = int(m.sum())
            for t in range(terms.shape[0]):
                x = terms[t, m]
                got = regions[r, t] if r < regions.shape[0] else field[t]
                assert abs(got - math.fsum(x)) <= n * U * math.fsum(np.abs(x)), (arithmetic, r, t, got)


def test_derived_error_bound_on_the_summary_deck(pkg, deck):
    case, fipnum, terms = deck
    _check_bound(pkg, terms, fipnum)


def test_derived_error_bound_on_three_phases_with_vaporised_oil(pkg, orc):
    case = helpers.wetgas_case(pkg, 5, 4, 8, heterogeneous=True)
    o = oracle_bind.OracleModel(orc, case)
    o.set_state(case["pv"], case["meaning"])
    iq = o.iq()
    assert iq.shape[1] == 19 and np.any(iq[:, 16, 0] > 0.0)     # the 19-field record, Rv != 0
    terms = pkg.fip.cell_terms(iq, case["volume"], case["poro"])
    assert np.any(terms[pkg.fip.T["OilInGasPhase"]] > 0.0)
    i = np.arange(case["Nb"])
    _check_bound(pkg, terms, i % 3 + 1)
    _check_bound(pkg, terms, np.where(i < 7, 0, i // 40 + 1))
    # any model with iq(): the oracle binding
    a, b = pkg.fip.model_inplace(o, case["volume"], case["poro"], i % 3 + 1, "stated"), pkg.fip.inplace(terms, i % 3 + 1, "stated")
    assert np.array_equal(a["regions"], b["regions"]) and np.array_equal(a["field"], b["field"]) and a["regions"].shape == (3, 14)


def _literal_reduce256(xs):
    """the stated order, chunk by chunk and lane by lane, in Python floats"""
    xs = [float(v) for v in xs]
    while True:
        res = []
        for c0 in range(0, len(xs), 256):
            ch = xs[c0:c0 + 256]
            ch = ch + [0.0] * (256 - len(ch))
            v = [(((0.0 + ch[l]) + ch[l + 64]) + ch[l + 128]) + ch[l + 192] for l in range(64)]
            o = 32
            while o:
                for l in range(o):           # lanes l < o read lanes >= o, which this round leaves alone
                    v[l] = v[l] + v[l + o]
                o //= 2
            res.append(v[0])
        xs = res
        if len(xs) == 1:
            return xs[0]


@pytest.mark.parametrize("n", LENGTHS)
def test_stated_order_equals_the_literal_walk(pkg, n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)    # magnitudes apart: another order gives other bits
    want = _literal_reduce256(x)
    assert pkg.fip.reduce256(x) == want
    terms = np.stack([x, -x, x * x])                               # and through region_sums, several rows at once, other cells between
    region = np.zeros(n + 5, int)
    region[2:n + 2] = 4
    t2 = np.zeros((3, n + 5))
    t2[:, 2:n + 2] = terms
    t2[:, [0, 1, n + 2]] = 1e300
    regions, field = pkg.fip.region_sums(t2, region, "stated")
    assert regions.shape == (4, 3) and regions[3, 0] == want and regions[3, 1] == -want and regions[3, 2] == _literal_reduce256(x * x)
    assert np.all(regions[:3] == 0.0) and np.array_equal(field, ((0.0 + regions[0]) + regions[1] + regions[2]) + regions[3])


def test_region_rules(pkg, orc):
    case, fipnum = helpers.summary_deck_case(pkg)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[fipnum == 2, 0] = 1.0                                   # region 2 filled with water: S_o = S_g = 0, HydroCarbonPV = 0 <= 1e-10
    case["pv"] = np.ascontiguousarray(pv.reshape(-1))
    F, T = pkg.fip, pkg.fip.T
    terms = F.cell_terms(_records(orc, case), case["volume"], case["poro"])
    region = fipnum.copy()
    region[:50] = 0                                            # no region
    region[50:60] = -3                                         # neither
    region[region == 3] = 5                                    # ids 3 and 4 are carried by no cell
    for arithmetic in ("sequential", "stated"):
        ip = F.inplace(terms, region, arithmetic)
        reg, field = ip["regions"], ip["field"]
        assert reg.shape == (5, 14)
        # ids <= 0 are in no region and in no field total
        full = F.inplace(terms, np.where(region >= 1, region, 7), arithmetic)
        assert np.array_equal(full["regions"][:5], reg, equal_nan=True) and np.all(full["field"][:12][[0, 1, 3]] > field[:12][[0, 1, 3]])
        assert np.array_equal(field[:12], (((0.0 + reg[0, :12]) + reg[1, :12]) + reg[2, :12] + reg[3, :12]) + reg[4, :12])
        # a missing id: zeros and the reference's 0.0 / 0.0
        assert np.all(reg[2:4, :12] == 0.0) and np.all(np.isnan(reg[2:4, 12:]))
        # a region without hydrocarbons takes the pore-volume average, both ways
        assert reg[1, T["HydroCarbonPV"]] <= 1e-10 and reg[1, T["PoreVolume"]] > 0.0
        assert reg[1, 12] == reg[1, 13] == reg[1, T["PressurePV"]] / reg[1, T["PoreVolume"]]
        # one with hydrocarbons: the two averages are different numbers, each its own quotient
        assert reg[0, 12] == reg[0, T["PressureHydroCarbonPV"]] / reg[0, T["HydroCarbonPV"]]
        assert reg[0, 13] == reg[0, T["PressurePV"]] / reg[0, T["PoreVolume"]] and reg[0, 12] != reg[0, 13]
        assert field[12] == field[T["PressureHydroCarbonPV"]] / field[T["HydroCarbonPV"]]
    s = F.summary(ip, initial=dict(field=2.0 * ip["field"], regions=ip["regions"]))
    assert s["FOE"] == 0.5 and s["FOIP"] == ip["field"][T["OIL"]] and s["RPRP:2"] == ip["regions"][1, 13] and math.isnan(s["RPR:3"])
    assert "FOE" not in F.summary(ip)
    # no cell in any region: no rows, a field of zeros and NaNs
    none = F.inplace(terms, np.zeros(case["Nb"], int))
    assert none["regions"].shape == (0, 14) and np.all(none["field"][:12] == 0.0) and np.all(np.isnan(none["field"][12:]))
    with pytest.raises(ValueError):
        F.region_sums(terms, region, "pairwise")
    with pytest.raises(ValueError):
        F.region_sums(terms, region[:-1])


def test_relation_to_the_reservoir_averages(pkg, orc):
    """wells.reservoir_averages (RateConverter's defineState) weights a cell's pressure by pv (1 - S_w), the report by pv (S_o + S_g):
    the same weight to a rounding each (S_o is formed as 1 - S_w - S_g), over the same cells where no cell is filled with water (there
    every weight is > 0).  Both are quotients of two sums of n positive terms, each sum within n u of its exact value, the weights within
    2 u of each other: the two pressures agree to (4 n + 8) u."""
    case = pkg.decks.cartesian_case(5, 4, 8, state="mixed", heterogeneous=True)
    iq = _records(orc, case)
    assert np.all(iq[:, 0, 0] < 1.0)
    n = case["Nb"]
    avg = pkg.wells.reservoir_averages(iq, case["volume"])
    assert avg[4] == 1.0
    terms = pkg.fip.cell_terms(iq, case["volume"], case["poro"])
    for arithmetic in ("sequential", "stated"):
        f = pkg.fip.inplace(terms, np.ones(n, int), arithmetic)["field"]
        assert abs(f[12] - avg[0]) <= (4 * n + 8) * U * avg[0]
        assert abs(f[pkg.fip.T["HydroCarbonPV"]] - avg[3]) <= (2 * n + 4) * U * avg[3]

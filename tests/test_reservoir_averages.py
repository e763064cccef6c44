"""wells.reservoir_averages - RateConverter::SurfaceToReservoirVoidage::defineState (wells/RateConverter.hpp:433-554) over the whole field by a
sequential loop - on the oracle-backed model against math.fsum of the same per-cell products.  The summands are non-negative, so the
sequential sums of n of them stay within (n - 1) half-ulps of the exact ones; with the quotient's rounding |delta| <= (n + 2) 2^-53 |value|."""
import math

import numpy as np
import pytest

import helpers
import oracle_bind


def model_iq(orc, case, pv=None):
    om = oracle_bind.OracleModel(orc, case)
    om.set_state(case["pv"] if pv is None else pv, case["meaning"])
    return om.iq()


def by_fsum(iq, volume):
    nf = iq.shape[1]
    pv_cell = volume * iq[:, nf - 1, 0]
    hpv = pv_cell * (1.0 - iq[:, 0, 0])
    rv = iq[:, 16, 0] if nf == 19 else np.zeros(len(hpv))
    hc = math.fsum(hpv[hpv > 0.0]) > 0.0
    w, sel = (hpv, hpv > 0.0) if hc else (pv_cell, pv_cell > 0.0)
    s = math.fsum(w[sel])
    return np.array([math.fsum((iq[:, 4, 0] * w)[sel]) / s, math.fsum((iq[:, 15, 0] * w)[sel]) / s, math.fsum((rv * w)[sel]) / s, s, float(hc)])


def close(got, want, n):
    assert got[4] == want[4]
    assert np.all(np.abs(got[:4] - want[:4]) <= (n + 2) * 2.0 ** -53 * np.abs(want[:4])), (got, want)


def test_dry_gas_record(pkg, orc):
    case = pkg.decks.cartesian_case(7, 5, 6, state="mixed", heterogeneous=True)
    iq = model_iq(orc, case)
    got = pkg.wells.reservoir_averages(iq, case["volume"])
    close(got, by_fsum(iq, case["volume"]), case["Nb"])
    assert iq.shape[1] == 17 and got[2] == 0.0 and got[4] == 1.0 and iq[:, 4, 0].min() < got[0] < iq[:, 4, 0].max()


def test_wet_gas_record(pkg, orc):
    case = helpers.wetgas_case(pkg, 5, 4, 8, heterogeneous=True)
    iq = model_iq(orc, case)
    got = pkg.wells.reservoir_averages(iq, case["volume"])
    close(got, by_fsum(iq, case["volume"]), case["Nb"])
    assert iq.shape[1] == 19 and got[2] > 0.0


def test_the_pore_volume_fallback_and_cells_left_out(pkg, orc):
    case = pkg.decks.cartesian_case(6, 5, 4, state="undersaturated")
    pv = case["pv"].reshape(-1, 3).copy()
    pv[::3, 0] = 1.0                              # some cells without hydrocarbon pore volume: left out of the hydrocarbon sums
    iq = model_iq(orc, case, np.ascontiguousarray(pv.reshape(-1)))
    got = pkg.wells.reservoir_averages(iq, case["volume"])
    close(got, by_fsum(iq, case["volume"]), case["Nb"])
    assert got[4] == 1.0 and got[3] < math.fsum(case["volume"] * iq[:, 16, 0] * 0.9)
    pv[:, 0] = 1.0                                # none anywhere: the pore-volume weights
    iq = model_iq(orc, case, np.ascontiguousarray(pv.reshape(-1)))
    got = pkg.wells.reservoir_averages(iq, case["volume"])
    close(got, by_fsum(iq, case["volume"]), case["Nb"])
    assert got[4] == 0.0 and got[3] == pytest.approx(math.fsum(case["volume"] * iq[:, 16, 0]), rel=1e-13)


def test_a_field_without_pore_volume_is_refused(pkg, orc):
    case = pkg.decks.cartesian_case(3, 2, 2)
    iq = model_iq(orc, case)
    with pytest.raises(ValueError, match="pore volume"):
        pkg.wells.reservoir_averages(iq, np.zeros(case["Nb"]))

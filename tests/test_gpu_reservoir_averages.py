"""opmhip_reservoir_averages - RateConverter::SurfaceToReservoirVoidage::defineState (wells/RateConverter.hpp:433-554) for the whole field
as a two-stage reduction on the device - against math.fsum of the per-cell products, formed in float64 in the stated order from the
intensive quantities the device itself reports.

Tolerance, derived and not measured: all summands are non-negative, so any summation order of n of them stays within (n - 1) half-ulps of
the exact sum; with the quotient's rounding |delta| <= (n + 2) * 2^-53 * |value|.

Cell counts: 1, one short of / exactly / one past a workgroup of 256, one past RESV_FINAL_THREADS x 256 (the final stage's lanes take a
second pass over the partials) and one past RESV_MAX_PARTS x 256 (the first stage's lanes stride over the grid) - the constants of
csrc/internal.hpp."""
import math
import re
import os

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def kernel_constants():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "opm-autodiff_amd", "csrc", "internal.hpp")) as f:
        txt = f.read()
    return tuple(int(re.search(r"\b%s = (\d+)" % n, txt).group(1)) for n in ("RESV_MAX_PARTS", "RESV_FINAL_THREADS"))


MAX_PARTS, FINAL_THREADS = kernel_constants()
COUNTS = {1: (1, 1, 1), 255: (5, 3, 17), 256: (4, 8, 8), 257: (257, 1, 1), FINAL_THREADS * 256 + 1: (FINAL_THREADS * 256 + 1, 1, 1),
          MAX_PARTS * 256 + 1: (MAX_PARTS * 256 + 1, 1, 1)}


def expected(iq, volume):
    """(pressure, rs, rv, pv, weights) from math.fsum of the per-cell products"""
    nf = iq.shape[1]
    pv_cell = volume * iq[:, nf - 1, 0]
    hydrocarbon = 1.0 - iq[:, 0, 0]
    hpv = pv_cell * hydrocarbon
    po, rs = iq[:, 4, 0], iq[:, 15, 0]
    rv = iq[:, 16, 0] if nf == 19 else np.zeros(len(po))
    sel, w = (hpv > 0.0, hpv) if math.fsum(hpv[hpv > 0.0]) > 0.0 else (pv_cell > 0.0, pv_cell)
    s = math.fsum(w[sel])
    return np.array([math.fsum((po * w)[sel]) / s, math.fsum((rs * w)[sel]) / s, math.fsum((rv * w)[sel]) / s, s, 1.0 if w is hpv else 0.0])


def check(m, volume):
    got = m.reservoir_averages()
    want = expected(m.iq(), np.asarray(volume, float))
    n = len(volume)
    print("cells %d: got %r want %r relative %r" % (n, got.tolist(), want.tolist(), (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).tolist()))
    assert got[4] == want[4]
    assert np.all(np.abs(got[:4] - want[:4]) <= (n + 2) * 2.0 ** -53 * np.abs(want[:4]))
    assert np.array_equal(got, m.reservoir_averages())          # no atomics: the same bits from call to call
    return got


@pytest.mark.parametrize("cells", sorted(COUNTS))
def test_dry_gas_layout_at_the_size_edges(pkg, cells):
    case = pkg.decks.cartesian_case(*COUNTS[cells], state="mixed" if cells in (255, 256) else "undersaturated", heterogeneous=False)
    assert case["Nb"] == cells
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    got = check(m, case["volume"])
    assert got[2] == 0.0 and got[4] == 1.0 and got[1] > 0.0 and 200e5 < got[0] < 300e5


@pytest.mark.parametrize("dims", [(7, 6, 9), (257, 1, 1)])
def test_wet_gas_layout(pkg, dims):
    case = helpers.wetgas_case(pkg, *dims, heterogeneous=True)
    m = pkg.capi.HipModel(case)
    m.set_state(case["pv"], case["meaning"])
    assert m.iq().shape[1] == 19
    got = check(m, case["volume"])
    assert got[2] > 0.0 and got[4] == 1.0      # (undersaturated oil cells carry Rv too: the saturated value)


def test_water_filled_field_takes_the_pore_volume_weights(pkg):
    case = pkg.decks.cartesian_case(9, 7, 5, state="undersaturated")
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 0] = 1.0
    m = pkg.capi.HipModel(case)
    m.set_state(np.ascontiguousarray(pv.reshape(-1)), case["meaning"])
    got = check(m, case["volume"])
    assert got[4] == 0.0 and got[3] > 0.0


def test_cells_without_hydrocarbon_pore_volume_are_left_out(pkg):
    case = pkg.decks.cartesian_case(9, 7, 5, state="mixed")
    pv = case["pv"].reshape(-1, 3).copy()
    wet = np.arange(case["Nb"]) % 3 == 0
    pv[wet, 0] = 1.0
    pv[wet & (case["meaning"] == 0), 2] = 0.0
    m = pkg.capi.HipModel(case)
    m.set_state(np.ascontiguousarray(pv.reshape(-1)), case["meaning"])
    got = check(m, case["volume"])
    iq = m.iq()
    hpv = case["volume"] * iq[:, 16, 0] * (1.0 - iq[:, 0, 0])
    assert got[4] == 1.0 and (hpv == 0.0).sum() == wet.sum() and got[3] < math.fsum(case["volume"] * iq[:, 16, 0])


def test_refusals(pkg):
    import ctypes as C
    capi = pkg.capi
    case = pkg.decks.cartesian_case(4, 3, 3, state="mixed")
    m = capi.HipModel(case)
    with pytest.raises(capi.OpmHipError) as e:
        m.reservoir_averages()
    assert e.value.code == capi.NOT_READY
    m.set_state(case["pv"], case["meaning"])
    assert capi.lib().opmhip_reservoir_averages(m._h, None) == capi.INVALID_ARGUMENT
    # a field without pore volume: refused with the reason, nothing divided, the caller's array untouched
    empty = dict(case)
    empty["poro"] = np.zeros(case["Nb"])
    z = capi.HipModel(empty)
    z.set_state(case["pv"], case["meaning"])
    out = np.full(5, 7.0)
    assert capi.lib().opmhip_reservoir_averages(z._h, out.ctypes.data_as(C.c_void_p)) == capi.INVALID_ARGUMENT
    assert b"pore volume" in capi.lib().opmhip_last_error(z._h) and np.all(out == 7.0)
    # a subdomain with ghost cells: the sums over the ranks are not formed
    part = pkg.ras.cartesian_subdomain_case(4, 2, 0, state="mixed")
    d = capi.HipModel(part)
    d.set_state(part["pv"], part["meaning"])
    with pytest.raises(capi.OpmHipError) as e:
        d.reservoir_averages()
    assert e.value.code == capi.INVALID_ARGUMENT and "decomposed" in str(e.value)

"""k_relative_change_part / k_relative_change_final at their size edges, against the numpy statement of
tests/newton_ref.py (per-cell terms in the reference's order, the cells by math.fsum).  A lane of the first kernel
walks the cells with a stride of 256 x 256, so only a grid of more than 65 536 cells makes it take a second step."""
import math

import numpy as np
import pytest

import newton_ref

pytestmark = pytest.mark.gpu

SIZES = {1: (1, 1, 1), 255: (1, 1, 255), 256: (1, 1, 256), 257: (1, 1, 257), 65536: (64, 32, 32), 67240: (41, 41, 40)}
U = 2.0 ** -52


def bound(n):
    """relative bound on the numerator and on the denominator (all terms are >= 0): a lane's own additions (4 per cell and one per
    stride), the 256-wide tree (8), the final sequential sum over 256 partials (255), and a factor 2 over the unit roundoff;
    the ratio lies within twice that"""
    return (270 + math.ceil(n / 65536)) * U


class Ctx:
    def __init__(self, pkg, n):
        self.Nb = n
        self.case = case = newton_ref.census_case(pkg, *SIZES[n], seed=n)
        self.rs_sat = lambda p: pkg.decks.rs_sat(case["fluid"], p)
        self.m = pkg.capi.HipModel(case, reorder="graph_coloring_greedy")
        self.to, self.fr, _ = self.m.ordering()

    def old_level(self):
        self.m.set_state(self.case["pv"], self.case["meaning"])
        self.m.advance_time_level()
        return self.case["pv"].reshape(-1, 3), self.case["meaning"]


@pytest.fixture(scope="module", params=list(SIZES))
def ctx(pkg, request):
    return Ctx(pkg, request.param)


def test_equal_levels_give_zero(ctx):
    ctx.old_level()
    assert ctx.m.relative_change() == 0.0


def test_relative_change_after_an_update(ctx):
    """the new level comes from a drawn Newton update that makes cells change their meaning in each direction"""
    n = ctx.Nb
    po, mo = ctx.old_level()
    rng = np.random.default_rng(7000 + n)
    dx = newton_ref.census_dx(rng, po, mo, np.zeros(n, np.uint8), ctx.rs_sat)
    ctx.m.update(dx.reshape(-1), 1.0)
    pn, mn = ctx.m.get_state()
    if n > 1:
        assert ((mn == 0) & (mo == 1)).any() and ((mn == 1) & (mo == 0)).any()
    delta, denom, ratio, d, q = newton_ref.relative_change(pn, mn, po, mo)
    got = ctx.m.relative_change()
    print(n, got, ratio, abs(got - ratio) / (U * ratio))
    assert ratio > 0.0 and abs(got - ratio) <= 2.0 * bound(n) * ratio
    ctx.m.update_failed()                     # a rolled-back step compares equal levels again
    assert ctx.m.relative_change() == 0.0


def test_one_changed_cell_at_a_chosen_internal_index(ctx):
    """one cell alone carries the change; at internal index 65 536 it is the first cell a lane reaches in its second stride, so
    a missing stride shows as a ratio of 0, not as a rounding difference"""
    n = ctx.Nb
    for at in sorted(set(p for p in (0, 255, 256, n - 1, 65536) if p < n)):
        po, mo = ctx.old_level()
        cell = int(ctx.fr[at])
        dx = np.zeros((n, 3))
        dx[cell, 1] = 0.25 * po[cell, 1]
        ctx.m.update(dx.reshape(-1), 1.0)
        pn, mn = ctx.m.get_state()
        delta, denom, ratio, d, q = newton_ref.relative_change(pn, mn, po, mo)
        assert np.flatnonzero(d).tolist() == [cell] and d[cell] > 0.0
        got = ctx.m.relative_change()
        assert got > 0.0 and abs(got - ratio) <= 2.0 * bound(n) * ratio, (at, got, ratio)

"""opmhip_vfp_probe - the VFP functions the well kernels call - against vfp.py bit for bit, and against the reference's own numbers
(tests/golden/vfp_expected.json: the 4096 BHP values of tests/test_vfpproperties.cpp for tests/VFPPROD2, within its own two bounds)."""
import numpy as np
import pytest

import vfp_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    """one context holding every table of this module (set_vfp_tables needs no fluid, static data or state)"""
    vfp = pkg.vfp
    e = vfp_cases.expected()
    tables = dict(prod2=vfp_cases.vfpprod2(vfp), line=vfp_cases.line_table(vfp, e), axis6=vfp_cases.axis6_table(vfp), rnd=vfp_cases.random_table(vfp),
                  inj=vfp_cases.inj_table(vfp), inj_gas=vfp_cases.inj_table(vfp, num=4, flo_type="GAS"), wavy=vfp_cases.nonmonotone_table(vfp),
                  flat=vfp_cases.flat_table(vfp))
    s = pkg.capi.HipSolver()
    s.set_vfp_tables(list(tables.values()))
    yield s, tables, e
    s.close()


def both(pkg, s, t, *args, **kw):
    dev = s.vfp_probe(t.kind, t.table_num, *args, **kw)
    host = pkg.vfp.probe(t, *args, **kw)
    return dev, host


def test_vfpprod2_all_4096_points_in_one_launch(pkg, ctx):
    s, tables, e = ctx
    t = tables["prod2"]
    aq, li, va, thp, skipped, ref = vfp_cases.realistic_points(e)
    assert len(aq) == 4096 and skipped.sum() == 512
    target = pkg.vfp.bhp(t, aq, li, va, thp, 0.0)[:, 0] * np.where(np.arange(4096) % 3 == 0, 1.0, 0.9 + 0.05 * (np.arange(4096) % 7))
    dev, host = both(pkg, s, t, aq, li, va, thp, 0.0, bhp_target=target)
    assert np.array_equal(dev, host)
    assert np.all(np.isfinite(dev))                      # the 512 skipped points included
    d = np.abs(dev[~skipped, 0] * 10.0e-6 - ref[~skipped])
    print("largest difference %.3e bar, summed %.3e bar over %d points" % (d.max(), d.sum(), len(d)))
    assert len(d) == 3584 and d.max() <= e["max_d_tol"] and d.sum() <= e["sad_tol"]


def test_parse_interpolate_line_four_singleton_axes(pkg, ctx):
    s, tables, e = ctx
    aq, li, va, thp, alq = vfp_cases.line_points(e)
    dev, host = both(pkg, s, tables["line"], aq, li, va, thp, alq, bhp_target=thp)
    assert len(aq) == 3125 and np.array_equal(dev, host)
    for col in (0, 9):                                   # bhp == thp and thp(bhp) == thp, the reference test's bounds in Pa
        d = np.abs(dev[:, col] - thp)
        assert d.max() <= e["max_d_tol"] and d.sum() <= e["sad_tol"]


def test_six_entry_axis_and_the_cap(pkg, ctx):
    s, tables, e = ctx
    t = tables["axis6"]
    flo = np.array([9.0, 6.0, -1.0, 19.0, 1.0, 15.0, 1000.0])     # exact, inside, left (taken as 0), right, first, last, far right (factor capped at 3)
    dev, host = both(pkg, s, t, -0.3 * flo, -flo, -50.0 * flo, 12.0e5, 0.0, bhp_target=40.0e5)
    assert np.array_equal(dev, host) and np.all(np.isfinite(dev))
    f = [pkg.vfp.find_interp_data(v, t.flo_axis) for v in flo]
    assert [(a, b) for a, b, _, _ in f] == [(2, 3), (1, 2), (0, 1), (4, 5), (0, 1), (4, 5), (4, 5)] and f[-1][3] == 3.0 and f[2][3] == -0.25
    # the cap shows in the value: 1000 and 23 = 11 + 3 * 4 give the same BHP
    assert dev[6, 0] == s.vfp_probe(t.kind, t.table_num, -6.9, -23.0, -1150.0, 12.0e5)[0, 0]


@pytest.mark.parametrize("name", ["inj", "inj_gas"])
def test_injector_table(pkg, ctx, name):
    s, tables, e = ctx
    q = np.array([0.0, 0.001, 0.002, 0.0049, 0.02, 0.03, 0.2, -0.01])
    thp = np.array([40.0, 50.0, 75.0, 100.0, 150.0, 200.0, 260.0, 1000.0]) * 1e5
    Q, T = (a.ravel() for a in np.meshgrid(q, thp, indexing="ij"))
    dev, host = both(pkg, s, tables[name], Q, 0.25 * Q, 100.0 * Q, T, bhp_target=180.0e5 + 0.3 * T)
    assert np.array_equal(dev, host) and np.all(np.isfinite(dev))
    assert np.any(dev[:, 5] != 0.0) and np.all(dev[:, 2:5] == 0.0)


@pytest.mark.parametrize("name", ["prod2", "rnd", "axis6", "line"])
def test_zero_rates_and_injecting_rates_into_a_producer_table(pkg, ctx, name):
    s, tables, e = ctx
    t = tables[name]
    thp = float(t.thp_axis[0] + 0.3 * (t.thp_axis[-1] - t.thp_axis[0]))
    aq = np.array([0.0, 0.01, 0.0, 0.0, 0.02, -0.0, -0.01, 0.0])
    li = np.array([0.0, 0.02, 0.03, 0.0, -0.02, 0.0, 0.01, -0.0])
    va = np.array([0.0, 3.0, 0.0, 5.0, 1.0, -0.0, 0.0, 0.0])
    dev, host = both(pkg, s, t, aq, li, va, thp, 10.0, bhp_target=float(t.values.mean()))
    assert np.array_equal(dev, host) and np.all(np.isfinite(dev))
    # injecting into a producer table: every chop binds, so nothing is left of d/dq but the flo term (getFlo itself is not chopped)
    assert np.array_equal(dev[1, 6:9], 0.0 - dev[1, 5] * pkg.vfp.flo(t, aq[1], li[1], va[1])[1][:, 0])
    assert dev[0, 9] == pkg.vfp.thp(t, 0.0, 0.0, 0.0, float(t.values.mean()), 10.0)


def test_find_thp_branches_through_a_table_not_monotone_in_thp(pkg, ctx):
    s, tables, e = ctx
    bar = 1e5
    # at the lowest rate the BHP along THP is 10, 30, 20, 20, 40 bar: below, inside (first rising interval), on a node, in the flat, above, NaN
    target = np.array([5.0, 10.0, 25.0, 30.0, 20.0, 35.0, 40.0, 45.0, np.nan]) * bar
    dev, host = both(pkg, s, tables["wavy"], -0.1, -0.002, -0.001, 25.0e5, 0.0, bhp_target=target)
    assert np.array_equal(dev, host, equal_nan=True)
    assert dev[-1, 9] == -1e100 and np.all(np.isfinite(dev[:-1, 9]))
    assert dev[2, 9] == 10.0e5 + (25.0 - 10.0) * bar * (10.0 * bar / (20.0 * bar))
    # sorted with dy == 0 in the first interval: below takes x1, above extrapolates, inside interpolates
    target = np.array([10.0, 15.0, 20.0, 25.0, 30.0]) * bar
    dev, host = both(pkg, s, tables["flat"], -0.01, -0.002, -0.5, 15.0e5, 0.0, bhp_target=target)
    assert np.array_equal(dev, host)
    assert dev[0, 9] == 20.0e5 and dev[1, 9] == 20.0e5


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes_around_the_block(pkg, ctx, n):
    s, tables, e = ctx
    t = tables["rnd"]
    rng = np.random.default_rng(n)
    aq, li, va = -rng.uniform(0.0, 0.8, n), -rng.uniform(0.0, 1.5, n), -rng.uniform(0.0, 0.5, n)
    thp, alq = rng.uniform(0.0, 2.0, n), rng.uniform(-5.0, 60.0, n)
    dev, host = both(pkg, s, t, aq, li, va, thp, alq, bhp_target=rng.uniform(0.0, 5.0, n))
    assert dev.shape == (n, 10) and np.array_equal(dev, host)


def test_round_trip_on_the_device(pkg, ctx):
    s, tables, e = ctx
    t = tables["rnd"]
    b = s.vfp_probe(t.kind, t.table_num, -0.5, -0.9, -0.1, 0.5, 32.9)[0, 0]
    back = s.vfp_probe(t.kind, t.table_num, -0.5, -0.9, -0.1, 0.5, 32.9, bhp_target=b)[0, 9]
    assert abs(back - 0.5) <= 1e-10 * 0.5


def test_refusals_leave_the_previous_set_in_force(pkg, ctx):
    s, tables, e = ctx
    vfp = pkg.vfp
    before = s.vfp_probe(0, 6, -3.0, -6.0, -100.0, 12.0e5)
    dup = [tables["axis6"], tables["axis6"]]
    with pytest.raises(pkg.capi.OpmHipError, match="duplicate"):
        s.set_vfp_tables(dup)
    bad = vfp_cases.axis6_table(vfp)
    bad.values = bad.values.copy()
    bad.values[1, 0, 0, 0, 2] = np.inf
    with pytest.raises(pkg.capi.OpmHipError, match="not finite"):
        s.set_vfp_tables([bad])
    bad = vfp_cases.axis6_table(vfp)
    bad.axes[0] = bad.axes[0][::-1].copy()
    with pytest.raises(pkg.capi.OpmHipError, match="decreases"):
        s.set_vfp_tables([bad])
    with pytest.raises(pkg.capi.OpmHipError, match="no table"):
        s.vfp_probe(1, 6, 1.0, 0.0, 0.0, 1e5)
    assert np.array_equal(s.vfp_probe(0, 6, -3.0, -6.0, -100.0, 12.0e5), before)

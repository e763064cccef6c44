"""vfp.py - the host statement of the VFP look-ups - against the reference's own numbers (tests/golden/vfp_expected.json, taken from
tests/test_vfpproperties.cpp; the table of tests/VFPPROD2 in tests/golden/vfpprod2_table.json) and against itself where the reference
pins nothing: the derivatives by the rates (central differences) and every branch of findTHP on hand-made arrays."""
import numpy as np
import pytest

import vfp_cases


@pytest.fixture(scope="module")
def e():
    return vfp_cases.expected()


def test_the_six_find_interp_data_cases(pkg, e):
    axis = e["find_interp_data"]["axis"]
    assert axis == [1.0, 5.0, 7.0, 9.0, 11.0, 15.0] and len(e["find_interp_data"]["cases"]) == 6
    for c in e["find_interp_data"]["cases"]:
        i0, i1, inv, fac = pkg.vfp.find_interp_data(c["value"], axis)
        assert (i0, i1, fac) == (c["i0"], c["i1"], c["factor"]), c
        assert inv == 1.0 / (axis[i1] - axis[i0])
    # the array form gives the same, and the rules the reference's test does not reach
    v = np.array([c["value"] for c in e["find_interp_data"]["cases"]])
    i0, i1, inv, fac = pkg.vfp.find_interp_data(v, axis)
    assert list(i0) == [c["i0"] for c in e["find_interp_data"]["cases"]] and list(fac) == [c["factor"] for c in e["find_interp_data"]["cases"]]
    assert pkg.vfp.find_interp_data(3.0, [2.0]) == (0, 0, 0.0, 0.0)
    assert pkg.vfp.find_interp_data(1000.0, axis) == (4, 5, 0.25, 3.0)                    # the cap
    assert pkg.vfp.find_interp_data(6.0, [1.0, 5.0, 5.0, 7.0]) == (2, 3, 0.5, 0.5)
    assert pkg.vfp.find_interp_data(5.0, [1.0, 5.0, 5.0, 7.0]) == (0, 1, 0.25, 1.0)       # the first i with axis[i] >= value
    assert pkg.vfp.find_interp_data(7.0, [1.0, 7.0, 7.0]) == (1, 2, 0.0, 0.0)             # end == start: both 0


def test_vfpprod2_sweep_against_the_reference_values(pkg, e):
    t = vfp_cases.vfpprod2(pkg.vfp)
    assert t.values.shape == (7, 9, 9, 1, 12)
    aq, li, va, thp, skipped, ref = vfp_cases.realistic_points(e)
    assert len(ref) == 4096 and skipped.sum() == 512 and np.array_equal(skipped, np.tile(np.repeat(np.arange(8) == 7, 64), 8))   # wct == 1
    b = pkg.vfp.bhp(t, aq, li, va, thp, 0.0)
    assert np.all(np.isfinite(b))
    d = np.abs(b[~skipped, 0] * 10.0e-6 - ref[~skipped])
    print("largest difference %.3e bar, summed %.3e bar over %d points" % (d.max(), d.sum(), len(d)))
    assert len(d) == 3584 and d.max() <= e["max_d_tol"] == 1e-10 and d.sum() <= e["sad_tol"] == 1e-8
    # floats in, floats out: the scalar form is the array form
    k = 1234
    assert np.array_equal(pkg.vfp.bhp(t, float(aq[k]), float(li[k]), float(va[k]), float(thp[k]), 0.0), b[k])


def test_parse_interpolate_line(pkg, e):
    t = vfp_cases.line_table(pkg.vfp, e)
    assert [len(a) for a in t.axes] == [1, 2, 1, 1, 1] and t.thp_axis[1] == 6894.757293168361
    aq, li, va, thp, alq = vfp_cases.line_points(e)
    assert len(aq) == 3125 and thp.max() == 4 * 456.78
    b = pkg.vfp.bhp(t, aq, li, va, thp, alq)[:, 0]
    back = pkg.vfp.thp(t, aq, li, va, thp, alq)
    for got in (b, back):
        d = np.abs(got - thp)
        assert d.max() <= e["max_d_tol"] and d.sum() <= e["sad_tol"]


def test_round_trip_on_a_seeded_random_table(pkg):
    """THPToBHPAndBackNonTrivial (tests/test_vfpproperties.cpp:537-552): thp recovered to 1e-10 relative"""
    vfp = pkg.vfp
    for seed in (7, 8, 9):
        t = vfp_cases.random_table(vfp, seed)
        b = vfp.bhp(t, -0.5, -0.9, -0.1, 0.5, 32.9)[0]
        assert abs(vfp.thp(t, -0.5, -0.9, -0.1, b, 32.9) - 0.5) <= 1e-10 * 0.5
    t = vfp_cases.inj_table(vfp)
    b = vfp.bhp(t, 0.004, 0.0, 0.0, 120e5)[0]
    assert abs(vfp.thp(t, 0.004, 0.0, 0.0, b) - 120e5) <= 1e-10 * 120e5


@pytest.mark.parametrize("types", [("OIL", "WOR", "GOR"), ("LIQ", "WCT", "GLR"), ("GAS", "WGR", "OGR")])
def test_rate_derivatives_against_central_differences(pkg, types):
    """Away from the kinks bhp is multilinear in (flo, wfr, gfr) - the product of three linear functions at most - and those are rational
    in the rates.  Step h = 1e-6 * |q| on each rate: the central difference's truncation error is h^2 / 6 * |f'''|, and with f a smooth
    function of q / scale whose derivatives are O(|f'| / |q|^2) at these points that is about 1e-12 relative; its rounding error is
    eps * |bhp| / h relative to |f'| = |bhp| / |q| scale, that is 2e-16 / 1e-6 = 2e-10 relative to |bhp| / |q|.  Bound: 1e-8 * |bhp| / |q|
    absolute - fifty times the rounding term, a wrong sign or a missing term is orders above it."""
    vfp = pkg.vfp
    base = vfp_cases.random_table(vfp, 11)
    ax = [base.axes[0], base.axes[1], base.axes[2] * (1.0 if types[1] == "WCT" else 3.0), base.axes[3] * 5.0, base.axes[4]]
    t = vfp.VFPTable(vfp.PROD, 1, 0.0, types[0], ax, base.values, types[1], types[2])
    rng = np.random.default_rng(3)
    done = 0
    for _ in range(200):
        q = -rng.uniform(0.2, 1.0, 3)
        # away from the kinks: the point and its two neighbours per rate lie in the same cell of the table, and nothing is chopped
        def cell(qq):
            f, w, g = vfp.flo(t, *qq)[0][0], vfp.wfr(t, *qq)[0][0], vfp.gfr(t, *qq)[0][0]
            found = [vfp.find_interp_data(v, a) for v, a in ((-f, t.flo_axis), (w, t.wfr_axis), (g, t.gfr_axis))]
            return tuple(i[:2] for i in found) + (any(i[3] >= 3.0 for i in found),)
        h = 1e-6 * np.abs(q)
        pts = [q + s * h[j] * np.eye(3)[j] for j in range(3) for s in (-1.0, 1.0)]
        cells = {cell(p) for p in pts + [q]}
        if len(cells) != 1 or cells.pop()[3]:       # (the cap at 3.0 is a kink too: the value stops moving, the reference's derivative does not)
            continue
        out = vfp.bhp(t, q[0], q[1], q[2], 0.6, 25.0)
        for j in range(3):
            num = (vfp.bhp(t, *pts[2 * j + 1], 0.6, 25.0)[0] - vfp.bhp(t, *pts[2 * j], 0.6, 25.0)[0]) / (2.0 * h[j])
            assert abs(out[6 + j] - num) <= 1e-8 * abs(out[0]) / abs(q[j]), (types, q, j, out[6 + j], num)
        done += 1
    assert done >= 50
    # a chop that binds has derivative zero: injecting rates leave the flo term alone
    out = vfp.bhp(t, 0.3, 0.4, 0.5, 0.6, 25.0)
    assert np.array_equal(out[6:9], 0.0 - out[5] * vfp.flo(t, 0.3, 0.4, 0.5)[1][:, 0])


def test_injector_bhp_and_its_derivative(pkg):
    vfp = pkg.vfp
    t = vfp_cases.inj_table(vfp)
    q, thp = 0.0035, 80e5
    out = vfp.bhp(t, q, 0.0, 0.0, thp)
    f = lambda x: 1e5 * (150.0 - 4.0e3 * x - 2.0e5 * x * x)
    want = f(0.002) + (f(0.005) - f(0.002)) * (q - 0.002) / 0.003 + thp
    assert abs(out[0] - want) <= 1e-12 * want and np.all(out[2:5] == 0.0) and out[7] == 0.0 and out[8] == 0.0
    assert abs(out[6] - (f(0.005) - f(0.002)) / 0.003) <= 1e-9 * abs(out[6]) and abs(out[1] - 1.0) <= 1e-12
    assert vfp.bhp(vfp_cases.inj_table(vfp, flo_type="GAS"), 1.0, 2.0, q, thp)[0] == out[0]


def test_every_find_thp_branch_on_hand_made_arrays(pkg):
    f = pkg.vfp.find_thp
    t = [1.0, 2.0, 3.0, 4.0]
    up = [10.0, 20.0, 40.0, 80.0]
    assert f(up, t, 5.0) == 1.0 + (5.0 - 10.0) * (1.0 / 10.0)            # sorted, below: the first interval, extrapolated
    assert f(up, t, 10.0) == 1.0                                          # ... "<=": on the first node
    assert f(up, t, 100.0) == 3.0 + (100.0 - 40.0) * (1.0 / 40.0)        # sorted, above: the last interval
    assert f(up, t, 30.0) == 2.0 + (30.0 - 20.0) * (1.0 / 20.0)          # sorted, inside
    assert f(up, t, 40.0) == 2.0 + (40.0 - 20.0) * (1.0 / 20.0) == 3.0   # y0 < bhp <= y1: the interval that ends at the node
    wavy = [10.0, 30.0, 20.0, 40.0]
    assert f(wavy, t, 25.0) == 1.0 + (25.0 - 10.0) * (1.0 / 20.0)        # unsorted and found: the first rising interval that holds it
    assert f(wavy, t, 35.0) == 3.0 + (35.0 - 20.0) * (1.0 / 20.0)
    assert f(wavy, t, 5.0) == 1.0 + (5.0 - 10.0) * (1.0 / 20.0)          # unsorted, extrapolated below
    assert f(wavy, t, 50.0) == 3.0 + (50.0 - 20.0) * (1.0 / 20.0)        # unsorted, extrapolated above
    down = [40.0, 30.0, 20.0, 10.0]
    assert f(down, t, 25.0) == 1.0 + (25.0 - 40.0) * (1.0 / -10.0)       # unsorted, nothing rises: bhp <= the first value, the first interval
    assert f(down, t, 45.0) == 3.0 + (45.0 - 20.0) * (1.0 / -10.0)       # ... and above the last value: the last interval
    flat = [15.0, 15.0, 25.0]
    assert f(flat, [1.0, 2.0, 3.0], 10.0) == 2.0 and f(flat, [1.0, 2.0, 3.0], 15.0) == 2.0      # dy == 0: x1
    assert f([5.0, 5.0], [1.0, 2.0], 7.0) == 2.0
    assert f(up, t, float("nan")) == -1e100                                                     # where the reference would throw
    assert f([40.0, 30.0], [1.0, 2.0], float("nan")) == -1e100
    with pytest.raises(ValueError):
        f([1.0], [1.0], 1.0)
    single = pkg.vfp.VFPTable(0, 1, 0.0, "OIL", [[1.0], [2.0], [0.0], [0.0], [0.0]], [3.0], "WOR", "GOR")
    with pytest.raises(ValueError, match="fewer than two"):
        pkg.vfp.thp(single, -1.0, -1.0, -1.0, 3.0)
    assert np.array_equal(pkg.vfp.probe(single, -1.0, -1.0, -1.0, 2.0, 0.0, bhp_target=3.0)[0], [3.0, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def test_zero_rates_in_the_inverse_look_up(pkg):
    """a producer with all-zero rates takes the first entry of the flo axis and zero fractions (VFPProdProperties.cpp:49-53)"""
    vfp = pkg.vfp
    t = vfp_cases.random_table(vfp, 5)
    col = t.values[:, 0, 0, 0, 0]                       # wfr = gfr = alq = 0 all lie below their axes: extrapolated, but the same for both
    fi, wi, gi, ai = (vfp.find_interp_data(v, a) for v, a in ((t.flo_axis[0], t.flo_axis), (0.0, t.wfr_axis), (0.0, t.gfr_axis), (0.0, t.alq_axis)))
    arr = [vfp.interpolate_prod(t, fi, vfp.find_interp_data(x, t.thp_axis), wi, gi, ai)[0][0] for x in t.thp_axis]
    assert vfp.thp(t, 0.0, 0.0, 0.0, 2.5, 0.0) == vfp.find_thp(arr, t.thp_axis, 2.5)
    assert np.array_equal(vfp.bhp_of_thp_axis(t, 0.0, 0.0, 0.0, 0.0)[:, 0], arr) and col.shape == (4,)


def test_table_refusals(pkg):
    V = pkg.vfp.VFPTable
    ok = dict(kind=0, table_num=1, datum_depth=0.0, flo_type="OIL", axes=[[1.0, 2.0], [1.0, 2.0], [0.0], [0.0], [0.0]], values=np.ones(4), wfr_type="WOR", gfr_type="GOR")
    V(**ok)
    for change in (dict(kind=2), dict(flo_type=3), dict(axes=[[2.0, 1.0], [1.0, 2.0], [0.0], [0.0], [0.0]]), dict(axes=[[1.0, np.nan], [1.0, 2.0], [0.0], [0.0], [0.0]]),
                   dict(axes=[[], [1.0, 2.0], [0.0], [0.0], [0.0]]), dict(values=[1.0, 2.0, np.inf, 4.0]), dict(values=np.ones(5)), dict(axes=[[1.0, 2.0], [1.0, 2.0]])):
        with pytest.raises((ValueError, KeyError)):
            V(**dict(ok, **change))

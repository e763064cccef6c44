"""tests/std_wells_harness.py's comparison without a device: a shared comparator must not silently compare less.  Every key compare_wells
can name - the base keys and every extra's - fails on one element one ulp off and says which key; so do a shape, a NaN and a key that is
not there."""
import numpy as np
import pytest

import std_wells_harness as H

KEYS = H.BASE + tuple(k for keys in H.EXTRAS.values() for k in keys)


def arrays():
    rng = np.random.default_rng(1)
    out = {k: rng.uniform(1.0, 2.0, (3, 4, 3)) for k in KEYS}
    out["ctl"] = [0, 1, 8]                                    # compare_wells hands the controls over as a list of codes
    return out


def test_keys_are_distinct_and_equal_dicts_pass():
    assert len(set(KEYS)) == len(KEYS) and set(H.BASE) == {"x", "head", "rw", "Dinv", "B", "C", "ctl"}
    assert H.keys_of(()) == H.BASE and H.keys_of(("D", "thp")) == H.BASE + ("D", "thp", "thp_dp", "bhp_from_thp")
    H.assert_same_keys(arrays(), arrays(), KEYS, "equal")
    H.same(arrays()["x"], arrays()["x"], "equal")
    with pytest.raises(AssertionError):
        H.keys_of(("D", "no such extra"))


@pytest.mark.parametrize("key", KEYS)
def test_one_ulp_in_one_element_fails_and_names_the_key(key):
    got, want = arrays(), arrays()
    if key == "ctl":
        got[key][1] += 1
    else:
        got[key][2, 3, 1] = np.nextafter(got[key][2, 3, 1], np.inf)
    with pytest.raises(AssertionError) as e:
        H.assert_same_keys(got, want, KEYS, "ulp")
    assert e.value.args[0][:2] == ("ulp", key), e.value.args
    H.assert_same_keys(got, want, tuple(k for k in KEYS if k != key), "the others")


def test_shape_nan_and_a_missing_key_fail():
    want = arrays()
    got = arrays()
    got["rw"] = got["rw"].reshape(3, 12)                      # the same numbers in another shape
    with pytest.raises(AssertionError) as e:
        H.assert_same_keys(got, want, KEYS, "shape")
    assert e.value.args[0][:2] == ("shape", "rw")
    got, want = arrays(), arrays()
    got["head"][0, 0, 0] = want["head"][0, 0, 0] = np.nan     # on both sides
    with pytest.raises(AssertionError) as e:
        H.assert_same_keys(got, want, KEYS, "nan")
    assert e.value.args[0][:2] == ("nan", "head")
    for side in (0, 1):
        pair = [arrays(), arrays()]
        del pair[side]["dq"]
        with pytest.raises(AssertionError) as e:
            H.assert_same_keys(pair[0], pair[1], KEYS, "missing")
        assert e.value.args[0][:3] == ("missing", "dq", "missing")
    with pytest.raises(AssertionError):
        H.same([1.0, np.inf], [1.0, np.inf], "equal and not finite")
    with pytest.raises(AssertionError):
        H.same([1.0, np.nan], [1.0, np.nan], "nan")


# ---- compare_wells over stand-ins for the two sides: what a call site names is what is compared ---------------------------------------------------
NW, NPERF = 2, 3
DEVICE_OF = dict(x="x", rw="rw", ctl="ctl", dq="dq", thp="thp:thp", thp_dp="thp:dp", bhp_from_thp="thp:bhp_from_thp", resv_coeff="resv:coeff",
                 resv_current="resv:resv_current", resv_averages="resv:averages", group_mode="groups:mode", group_rates="groups:rates",
                 group_voidage="groups:voidage", group_reduction="groups:reduction", group_guide_sum="groups:guide_sum", nupcol_rates="groups:nupcol_rates",
                 perf_pressure="wellbore:perf_pressure", perf_rates="wellbore:perf_rates")      # the others are std_wells_blocks()'s


class Namespace:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def two_sides():
    """-> a device stand-in, its arrays by getter, a host stand-in and its assembled dict, equal in every array"""
    rng = np.random.default_rng(2)
    u = lambda *shape: rng.uniform(1.0, 2.0, shape)
    dev = dict(blocks=dict(head=u(NPERF), D=u(NW, 4, 4), Dinv=u(NW, 4, 4), B=u(NPERF, 4, 3), C=u(NPERF, 4, 3), rates=u(NPERF, 3, 5), xw=u(NW, 4)),
               x=u(NW, 4), ctl=np.array([0, 8]), rw=u(NW, 4), dq=u(NPERF, 3, 3), thp=dict(thp=u(NW), dp=u(NW), bhp_from_thp=u(NW)),
               resv=dict(averages=u(5), coeff=u(NW, 3), resv_current=u(NW)),
               groups=dict(mode=np.array([1]), rates=u(1, 3), voidage=u(1), reduction=u(1, 3), guide_sum=u(1), nupcol_rates=u(NW, 3)),
               wellbore=dict(perf_pressure=u(NPERF), perf_rates=u(NPERF, 3)))
    copy = lambda d: {k: v.copy() for k, v in d.items()}
    md = Namespace(get_std_wells=lambda: (dev["x"], dev["ctl"], dev["rw"]), std_wells_blocks=lambda: copy(dev["blocks"]), std_wells_rate_dq=lambda: dev["dq"],
                   std_wells_thp=lambda: copy(dev["thp"]), std_wells_resv=lambda: copy(dev["resv"]), std_wells_groups=lambda: copy(dev["groups"]),
                   std_wells_wellbore=lambda: copy(dev["wellbore"]))
    b, g = copy(dev["blocks"]), copy(dev["groups"])           # the host's own
    wh = Namespace(cells=np.arange(NPERF), x=dev["x"].copy(), head=b["head"].copy(), wells=[Namespace(control=("rate", 0, 1.0)), Namespace(control=("grup",))],
                   rate_dq=dev["dq"].copy(), thp_current=dev["thp"]["thp"].copy(), thp_dp=dev["thp"]["dp"].copy(), bhp_from_thp=dev["thp"]["bhp_from_thp"].copy(),
                   resv_coeff=dev["resv"]["coeff"].copy(), resv_current=dev["resv"]["resv_current"].copy(), resv_averages=dev["resv"]["averages"].copy(), has_resv=True,
                   group_rates=lambda: {k: v for k, v in g.items() if k != "nupcol_rates"}, nupcol_rates=g["nupcol_rates"],
                   perf_pressure=dev["wellbore"]["perf_pressure"].copy(), perf_rates=dev["wellbore"]["perf_rates"].copy(),
                   records=lambda model: "records",
                   _assemble_wells=lambda iq: (None, b["D"].copy(), None, None, b["rates"][:, :, 0].copy(), b["rates"][:, :, 1:4].copy()),
                   _perf_rates=lambda iq, bhp: b["rates"].copy())
    wa = dict(res_well=dev["rw"].reshape(-1).copy(), wells=dict(Dnnzs=b["Dinv"].reshape(-1).copy(), Bnnzs=b["B"].reshape(-1).copy(), Cnnzs=b["C"].reshape(-1).copy()))
    return md, dev, wh, wa


PKG = Namespace(wells=Namespace(control_code=lambda control: 8 if control[0] == "grup" else 0))


def device_array(dev, key):
    where = DEVICE_OF.get(key, "blocks:" + {"source": "rates", "dsource": "rates"}.get(key, key))
    for part in where.split(":"):
        dev = dev[part]
    return dev


def test_compare_wells_passes_on_equal_sides_with_every_extra():
    md, dev, wh, wa = two_sides()
    got = H.compare_wells(PKG, md, wh, wa, "equal", extra=tuple(H.EXTRAS), mh="model", all_finite=True)
    assert set(KEYS) <= set(got) and "xw" in got


@pytest.mark.parametrize("extra,key", [((), k) for k in H.BASE] + [((e,), k) for e, keys in H.EXTRAS.items() for k in keys])
def test_compare_wells_compares_what_the_call_site_names(extra, key):
    md, dev, wh, wa = two_sides()
    a = device_array(dev, key)
    if a.dtype.kind == "i":
        a[-1] += 1
    else:
        a.reshape(-1)[{"dsource": 1}.get(key, 0)] = np.nextafter(a.reshape(-1)[{"dsource": 1}.get(key, 0)], np.inf)
    with pytest.raises(AssertionError) as e:
        H.compare_wells(PKG, md, wh, wa, "ulp", extra=extra, mh="model")
    assert e.value.args[0][:2] == ("ulp", key), e.value.args
    if extra and key not in ("source", "dsource"):           # not named, not compared (the rates' values are "rates" and "source" both)
        H.compare_wells(PKG, md, wh, wa, "not named", mh="model")


def test_compare_wells_averages_only_with_a_resv_limit_and_finiteness():
    md, dev, wh, wa = two_sides()
    dev["resv"]["averages"][0] += 1.0
    wh.has_resv = False
    H.compare_wells(PKG, md, wh, wa, "no RESV limit", extra=("resv",))
    wh.has_resv = True
    with pytest.raises(AssertionError):
        H.compare_wells(PKG, md, wh, wa, "a RESV limit", extra=("resv",))
    md, dev, wh, wa = two_sides()
    dev["x"][0, 0] = wh.x[0, 0] = np.inf
    with pytest.raises(AssertionError):
        H.compare_wells(PKG, md, wh, wa, "x not finite")
    md, dev, wh, wa = two_sides()
    dev["blocks"]["head"][0] = wh.head[0] = np.inf
    H.compare_wells(PKG, md, wh, wa, "the head is compared, not looked at otherwise")
    with pytest.raises(AssertionError):
        H.compare_wells(PKG, md, wh, wa, "every compared array", all_finite=True)

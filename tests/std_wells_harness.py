"""What the device-against-host tests of the standard wells share (tests/test_gpu_std_wells_*.py): two HipModel contexts in one state -
DeviceStandardWells on one, StandardWells(arithmetic="stated") on the other -, newton.py's host branch, and the comparison of what an
assembly leaves on the device with the host form, bit for bit.

What such a test proves rests on the compared keys.  compare_wells always compares BASE; a call site names what it compares beyond that
(EXTRAS), so that the list can be read at the call.  assert_same_keys is the comparison itself: a function of two dicts of arrays and a
tuple of keys (tests/test_std_wells_harness.py holds it to account without a device)."""
import numpy as np

DAY = 86400.0
OMIT = object()      # pair: a keyword left at OMIT is not handed to the constructors; None is a value some call sites hand over

BASE = ("x", "head", "rw", "Dinv", "B", "C", "ctl")
EXTRAS = {"D": ("D",),                                         # D itself, formed once more on the host: a pure function of the state
          "rates": ("rates",),                                 # the connection rates with all their derivatives (_perf_rates)
          "source": ("source", "dsource"),                     # ... their values and cell derivatives alone (_assemble_wells' src, dsrc)
          "dq": ("dq",),                                       # crossflow: d rate / d q
          "thp": ("thp", "thp_dp", "bhp_from_thp"),
          "resv": ("resv_coeff", "resv_averages"),             # (the averages where the list has a RESV limit)
          "resv_current": ("resv_current",),
          "groups": ("group_mode", "group_rates", "group_voidage", "group_reduction", "group_guide_sum", "nupcol_rates"),
          "wellbore": ("perf_pressure", "perf_rates")}


# ---- cases and states ----------------------------------------------------------------------------------------------------------------------
def make_case(pkg, ext):
    """2 x 2 x 150; ext: a fluid with pc_scaling - the extended (19-field) intensive-quantity record"""
    if ext:
        import helpers
        return helpers.hysteresis_case(pkg, 2, 2, 150, heterogeneous=True, dz=1.0)
    return pkg.decks.cartesian_case(2, 2, 150, state="mixed", heterogeneous=True, dz=1.0)


def column(nx, ny):
    """-> column(i, j, ks): the cells (i, j, k) of an nx x ny x . grid, cell = i + nx (j + ny k)"""
    return lambda i, j, ks: [i + nx * (j + ny * k) for k in ks]


def moved(case, seed, dp=2.0e5):
    rng = np.random.default_rng(seed)
    pv = case["pv"].reshape(-1, 3).copy()
    pv[:, 1] -= dp * rng.uniform(0.0, 1.0, len(pv))
    pv[:, 0] += rng.uniform(-0.01, 0.01, len(pv))
    return pv.reshape(-1)


def pair(pkg, case, make, *, head_model=OMIT, vfp=OMIT, vaporised_oil=OMIT, groups=OMIT, nupcol=OMIT, matrix_add=OMIT, props=None, pvtnum=OMIT,
         model_kw=None):
    """(device model, its wells), (host model, stated wells): two contexts in the same state.  make(): a fresh list of Well objects;
    groups(): a fresh list of Group objects.  head_model, vfp, vaporised_oil, groups and nupcol go to both constructors, matrix_add to the
    device's, props and pvtnum to the host's - each only where the call site names it (the launch-count tests hold "a list without X makes
    the calls it made before" to account: nothing is handed over on a call site's behalf).  props: None - no keyword; "wellbore" - the
    device's property functions (capi.HipFluid) under head_model="wellbore", else props=None; "always" - capi.HipFluid"""
    given = lambda **kw: {k: v for k, v in kw.items() if v is not OMIT}
    assert props in (None, "wellbore", "always"), props
    fluid = pkg.capi.HipFluid(case["fluid"]) if props == "always" or (props == "wellbore" and head_model == "wellbore") else None
    out = []
    for form in ("device", "host"):
        m = pkg.capi.HipModel(case, **(model_kw or {}))
        m.set_state(case["pv"], case["meaning"])
        wl = make()
        both = given(head_model=head_model, vfp=vfp, vaporised_oil=vaporised_oil, groups=OMIT if groups is OMIT else groups(), nupcol=nupcol)
        if form == "device":
            w = pkg.wells.DeviceStandardWells(wl, case["depth"], m, **both, **given(matrix_add=matrix_add))
        else:
            w = pkg.wells.StandardWells(wl, case["depth"], arithmetic="stated", **both, **given(pvtnum=pvtnum, props=OMIT if props is None else fluid))
        out.append((m, w))
    return out


# ---- newton.py's host branch ------------------------------------------------------------------------------------------------------------------
def host_begin(mh, wh, iteration, *, pass_iteration=False):
    """records down, the explicit quantities and the wells alone at iteration 0, the controls -> the records.  pass_iteration: the
    controls are told the iteration (group control: NUPCOL)"""
    iq = wh.records(mh)
    if iteration == 0:
        wh.calculate_explicit_quantities(iq)
        wh.solve_well_equations(iq)
    if pass_iteration:
        wh.update_well_controls(iteration)
    else:
        wh.update_well_controls()
    return iq


def host_assemble(mh, wh, iq):
    """the wells' equations, rates up -> the assembled dict"""
    wa = wh.assemble(iq)
    mh.set_source_cells(wa["cells"], wa["source_cells"], wa["dsource_cells"])
    return wa


def host_begin_and_assemble(mh, wh, iteration, *, pass_iteration=False):
    return host_assemble(mh, wh, host_begin(mh, wh, iteration, pass_iteration=pass_iteration))


def begin(wd, mh, wh, iteration):
    """beginIteration on both sides -> the host's records"""
    iq = host_begin(mh, wh, iteration)
    wd.begin_iteration(iteration)
    return iq


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------------
def assert_same_keys(got, want, keys, what):
    """got[k] == want[k] in shape and in every element, for every k of keys: a key missing on either side, a NaN on either side and a
    difference of one ulp all fail; the message names the key, the first eight differing indices and the values there"""
    for k in keys:
        assert k in got and k in want, (what, k, "missing")
        g, w = np.asarray(got[k], float), np.asarray(want[k], float)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(-1))
        assert bad.size == 0, (what, k, bad[:8], g.reshape(-1)[bad[:8]], w.reshape(-1)[bad[:8]])


def same(got, want, what):
    """one array against another, bit for bit and finite"""
    assert_same_keys({"": got}, {"": want}, ("",), what)
    assert np.all(np.isfinite(np.asarray(got, float))), (what, "not finite")


def same_state(a, b):
    (pa, ma), (pb, mb) = a.get_state(), b.get_state()
    return np.array_equal(ma, mb) and np.array_equal(pa, pb)


def keys_of(extra):
    unknown = [e for e in extra if e not in EXTRAS]
    assert not unknown, unknown
    return BASE + tuple(k for e in extra for k in EXTRAS[e])


def compare_wells(pkg, md, wh, wa, what, *, extra=(), mh=None, iq=None, all_finite=False):
    """after an assembly on both sides (wa: the host's assembled dict): BASE and the named EXTRAS of the device against the host form ->
    the device's arrays (std_wells_blocks() and what was read for the comparison), under the keys' names.  "D", "rates" and "source" form
    the host's side once more from iq, or from the records of mh.  The well unknowns and D^-1 are finite; all_finite: every compared array"""
    keys = keys_of(extra)
    x, ctl, rw = md.get_std_wells()
    got = dict(md.std_wells_blocks(), x=x, rw=rw, ctl=list(ctl))
    nperf, lists = len(wh.cells), wa["wells"]
    want = dict(x=wh.x, head=wh.head, rw=wa["res_well"].reshape(-1, 4), Dinv=lists["Dnnzs"].reshape(-1, 4, 4), B=lists["Bnnzs"].reshape(nperf, 4, 3),
                C=lists["Cnnzs"].reshape(nperf, 4, 3), ctl=[pkg.wells.control_code(w.control) for w in wh.wells])
    if iq is None and {"D", "rates", "source"} & set(extra):
        iq = wh.records(mh)
    if "D" in extra or "source" in extra:
        _, want["D"], _, _, want["source"], want["dsource"] = wh._assemble_wells(iq)
        got.update(source=got["rates"][:, :, 0], dsource=got["rates"][:, :, 1:4])
    if "rates" in extra:
        want["rates"] = wh._perf_rates(iq, wh.x[:, 3])
    if "dq" in extra:
        want["dq"], got["dq"] = wh.rate_dq, md.std_wells_rate_dq()
    if "thp" in extra:
        t = md.std_wells_thp()
        got.update(thp=t["thp"], thp_dp=t["dp"], bhp_from_thp=t["bhp_from_thp"])
        want.update(thp=wh.thp_current, thp_dp=wh.thp_dp, bhp_from_thp=wh.bhp_from_thp)
    if "resv" in extra or "resv_current" in extra:
        r = md.std_wells_resv()
        got.update(resv_coeff=r["coeff"], resv_current=r["resv_current"], resv_averages=r["averages"])
        want.update(resv_coeff=wh.resv_coeff, resv_current=wh.resv_current)
        if wh.has_resv:
            want["resv_averages"] = wh.resv_averages
        else:
            keys = tuple(k for k in keys if k != "resv_averages")
    if "groups" in extra:
        g, h = md.std_wells_groups(), wh.group_rates()
        for k in ("mode", "rates", "voidage", "reduction", "guide_sum"):
            got["group_" + k], want["group_" + k] = g[k], h[k]
        got["nupcol_rates"], want["nupcol_rates"] = g["nupcol_rates"], wh.nupcol_rates
    if "wellbore" in extra:
        wb = md.std_wells_wellbore()
        got.update(perf_pressure=wb["perf_pressure"], perf_rates=wb["perf_rates"])
        want.update(perf_pressure=wh.perf_pressure, perf_rates=wh.perf_rates)
    assert_same_keys(got, want, keys, what)
    for k in (keys if all_finite else ("x", "Dinv")):
        assert np.all(np.isfinite(np.asarray(got[k], float))), (what, k, "not finite")
    return got


def lockstep(pkg, case, make, states, dt=5.0 * DAY, *, extra, pass_iteration=False, **pair_kw):
    """iteration 0 at the case's state, then one more iteration per further state: the wells (BASE and extra) and the reservoir's J, r
    equal on both sides -> the two pairs, the host's last assembled dict, the device's arrays of the last comparison"""
    (md, wd), (mh, wh) = pair(pkg, case, make, **pair_kw)
    for it, state in enumerate([None] + list(states)):
        if state is not None:
            for m in (md, mh):
                m.set_state(state, case["meaning"])
        wa = host_begin_and_assemble(mh, wh, it, pass_iteration=pass_iteration)
        jh, rh = mh.assemble(dt, it)
        wd.begin_iteration(it)
        jd, rd = md.assemble(dt, it)
        blk = compare_wells(pkg, md, wh, wa, it, extra=extra, mh=mh)
        assert np.array_equal(jd, jh) and np.array_equal(rd, rh), it
    return (md, wd), (mh, wh), wa, blk


# ---- profile_get's launch counts ---------------------------------------------------------------------------------------------------------------
def launch_counts(m):
    return {k: v[0] for k, v in m.profile().items()}


def minus(a, b):
    return {k: a[k] - b[k] for k in a}

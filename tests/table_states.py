"""States that sit where a property-table lookup or a branch of the intensive-quantity update changes its answer, with a label
each, and an exact statement of the lookups to hold both the CPU oracle and the device against.

  tables(fluid)        the samples build_fluid_tables (csrc/fluid_tables.cpp) stores, restated in Python floats (IEEE double, the
                       builder's order of operations), region by region
  blob_doubles(fluid)  the length of the double blob those samples make (the layout of fluid_tables.cpp)
  states(fluid, ...)   one row per cell (Sw, p, third variable, meaning, pvtnum, satnum), a label per row, per-cell extras
  case_of(...)         the rows as an N x 1 x 1 case for capi.HipModel / oracle_bind.OracleModel
  exact(...)           1/B, viscosities, relative permeabilities, capillary pressures, RsSat and the mobilities of the cache in
                       fractions.Fraction, from the samples above and the conventions below
  two_row_fluid, equal_bubble_point_fluid, padded_fluid     the fluids the edge tests are cut for

Notation: for a double v, v- = nextafter(v, -inf), v+ = nextafter(v, +inf); a "triple" is v-, v, v+ and carries the suffixes
"-", "0", "+" in its labels.

Conventions (csrc/fluid_device.hpp):
  seg_right / tab1     linear, extrapolating with the end segments; a value on an interior node belongs to the segment on its RIGHT;
                       on the last node (the right end of the last segment) the value is the sample itself
  tab2g / tab2wg       bilinear over per-column y grids, the columns found with seg_right
  pwlin                constant outside the table; a value on a node belongs to the segment on its LEFT

The exact statement takes the decisions of a lookup (which segment, which branch) from the doubles the code compares - they are
what the states are made of - and does the arithmetic of the chosen branch without rounding.  Where a lookup's argument is itself
computed (a phase pressure, Sw + Sg), the argument is the double the code forms and the lookup is exact from there on."""
import copy
import math
from fractions import Fraction as Fr

import numpy as np

SW_PO_SG, SW_PO_RS, SW_PG_RV = 0, 1, 2
TAB_LDS_DBL = 3072            # assemble.hip: the largest double blob the per-cell kernels copy into LDS
EPS_COUNT = 18
NO_CAP = 1e30
# the largest distance (relative_distance below) between the CPU oracle and the exact statement over every finite state of the six
# fluids of tests/test_table_states.py, measured there; the tests hold the oracle and the device to four times it - the room for
# another order of the same few operations
ORACLE_TO_EXACT = 2.2951300889133675e-13
BOUND = 4.0 * ORACLE_TO_EXACT


def below(v):
    return float(np.nextafter(v, -np.inf))


def above(v):
    return float(np.nextafter(v, np.inf))


def triple(v):
    return [("-", below(v)), ("0", float(v)), ("+", above(v))]


# ---- the builder's samples ------------------------------------------------------------------------------------------------------
def _extend(last_p, last_b, last_mu, Mp, Mb, Mmu):
    """LiveOilPvt::extendPvtoTable_ / the PVTG twin as fluid_tables.cpp states them: the next complete node's steps, one by one"""
    ps, bs, mus = [last_p], [last_b], [last_mu]
    for q in range(1, len(Mp)):
        newp = ps[-1] + (Mp[q] - Mp[q - 1])
        B1, B2 = Mb[q], Mb[q - 1]
        x = (B1 - B2) / ((B1 + B2) / 2.0)
        newb = bs[-1] * (1.0 + x / 2.0) / (1.0 - x / 2.0)
        m1, m2 = Mmu[q], Mmu[q - 1]
        xm = (m1 - m2) / ((m1 + m2) / 2.0)
        newmu = mus[-1] * (1.0 + xm / 2.0) / (1.0 - xm / 2.0)
        ps.append(newp)
        bs.append(newb)
        mus.append(newmu)
    return ps, bs, mus


def tables(fluid):
    """-> dict(pvt=[...], sat=[...], rock=[...]) of plain float lists: what the device interpolates in"""
    out = dict(pvt=[], sat=[], rock=[])
    for r in fluid.pvt:
        D = dict(water=[float(v) for v in r["pvtw"]], density=[float(v) for v in r["density"]], wet=bool(r.get("pvtg")))
        if D["wet"]:
            gn = r["pvtg"]
            D["wg_xs"], D["gcols"], D["wgs_rv"], D["wgs_invB"], D["wgs_invBMu"] = [], [], [], [], []
            for i, g in enumerate(gn):
                rv, bg, mu = [float(v) for v in g["rv"]], [float(v) for v in g["bg"]], [float(v) for v in g["mu"]]
                extended = len(rv) < 2
                if extended:
                    M = next(m for m in gn[i + 1:] if len(m["rv"]) >= 2)
                    rv, bg, mu = _extend(rv[-1], bg[-1], mu[-1], [float(v) for v in M["rv"]], [float(v) for v in M["bg"]], [float(v) for v in M["mu"]])
                ib = [1.0 / b for b in bg]
                col = dict(y=rv[::-1], invB=ib[::-1], invBMu=[(1.0 / b) / m for b, m in zip(bg, mu)][::-1], extended=extended)
                D["wg_xs"].append(float(g["pg"]))
                D["gcols"].append(col)
                D["wgs_rv"].append(float(g["rv"][0]))
                D["wgs_invB"].append(col["invB"][-1])
                D["wgs_invBMu"].append(col["invBMu"][-1])
        else:
            rows = [[float(v) for v in q] for q in r["pvdg"]]
            D["gas_p"] = [q[0] for q in rows]
            D["gas_invB"] = [1.0 / q[1] for q in rows]
            D["gas_invBMu"] = [(1.0 / q[1]) / q[2] for q in rows]
        nodes = r["pvto"]
        D["o_xs"], D["cols"] = [], []
        for i, n in enumerate(nodes):
            p, bo, mu = [float(v) for v in n["p"]], [float(v) for v in n["bo"]], [float(v) for v in n["mu"]]
            ib = [1.0 / b for b in bo]
            extended = len(p) < 2
            if extended:
                M = next(m for m in nodes[i + 1:] if len(m["p"]) > 1)
                p, bx, mu = _extend(p[-1], bo[-1], mu[-1], [float(v) for v in M["p"]], [float(v) for v in M["bo"]], [float(v) for v in M["mu"]])
                ib = ib + [1.0 / b for b in bx[1:]]
            D["o_xs"].append(float(n["rs"]))
            D["cols"].append(dict(y=p, invB=ib, invBMu=[a / m for a, m in zip(ib, mu)], extended=extended, deck_bo=[float(v) for v in n["bo"]]))
        D["sat_p"] = [c["y"][0] for c in D["cols"]]
        D["sat_rs"] = list(D["o_xs"])
        D["sat_invB"] = [c["invB"][0] for c in D["cols"]]
        D["sat_invBMu"] = [c["invBMu"][0] for c in D["cols"]]
        out["pvt"].append(D)
    for s in fluid.sat:
        w = [[float(v) for v in q] for q in s["swof"]]
        g = [[float(v) for v in q] for q in s["sgof"]]
        swco = w[0][0]
        S = dict(swco=swco, sw=[q[0] for q in w], krw=[q[1] for q in w], krow=[q[2] for q in w], pcow=[q[3] for q in w],
                 so=[(1.0 - swco) - q[0] for q in g[::-1]], krg=[q[1] for q in g[::-1]], krog=[q[2] for q in g[::-1]], pcgo=[q[3] for q in g[::-1]],
                 sg_deck=[q[0] for q in g])
        out["sat"].append(S)
    for t in fluid.rocktab:
        out["rock"].append(dict(p=[float(q[0]) for q in t], poroMult=[float(q[1]) for q in t], transMult=[float(q[2]) for q in t]))
    return out


def blob_doubles(fluid):
    """the length of FluidTables::dbl: per PVT region water (5), densities (3), PVTG (pressure nodes, 3 arrays over the columns' samples,
    3 saturated arrays) or PVDG (3 arrays), PVTO (Rs nodes, 3 arrays over the columns' samples - single-sample nodes at the next
    complete node's length -, 4 saturated arrays); per saturation region 4 SWOF and 4 SGOF arrays, Swco, 18 end points; per ROCKTAB
    region 3 arrays"""
    T = tables(fluid)
    n = 0
    for D in T["pvt"]:
        n += 5 + 3
        if D["wet"]:
            n += len(D["wg_xs"]) + 3 * sum(len(c["y"]) for c in D["gcols"]) + 3 * len(D["wg_xs"])
        else:
            n += 3 * len(D["gas_p"])
        n += len(D["o_xs"]) + 3 * sum(len(c["y"]) for c in D["cols"]) + 4 * len(D["o_xs"])
    for S in T["sat"]:
        n += 4 * len(S["sw"]) + 4 * len(S["so"]) + 1 + EPS_COUNT
    for R in T["rock"]:
        n += 3 * len(R["p"])
    return n


def write_fluid_binary(fluid, path):
    """Fluid.arrays as the flat file tests/san/fluid_blob_size.cpp reads: int32 header (num_pvt, num_sat, num_rock, wet, then the
    element count of each array in the order below), then the arrays"""
    order = ("pvtw", "density", "pvdg_ptr", "pvdg", "pvto_node_ptr", "pvto_rs", "pvto_row_ptr", "pvto", "swof_ptr", "swof", "sgof_ptr", "sgof",
             "pvtg_node_ptr", "pvtg_pg", "pvtg_row_ptr", "pvtg", "rocktab_ptr", "rocktab")
    a = fluid.arrays
    arrs = [a.get(k, np.zeros(0, np.int32 if k.endswith("_ptr") else np.float64)) for k in order]
    head = np.array([len(fluid.pvt), len(fluid.sat), len(fluid.rocktab), int(fluid.wet_gas)] + [x.size for x in arrs], np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for x in arrs:
            f.write(np.ascontiguousarray(x).tobytes())


# ---- lookups: decisions on doubles, arithmetic in `num` (float: the code's own order; Fraction: exact) -----------------------------
def seg_right(x, xv):
    n = len(x)
    if xv <= x[0]:
        return 0
    if xv >= x[n - 1]:
        return n - 2
    lo, hi = 0, n - 1
    while lo + 1 < hi:
        mid = (lo + hi) >> 1
        if x[mid] <= xv:
            lo = mid
        else:
            hi = mid
    return lo


def tab1(x, y, xv, num=float):
    s = seg_right(x, xv)
    x0, x1, y0, y1 = num(x[s]), num(x[s + 1]), num(y[s]), num(y[s + 1])
    if xv == x[s + 1]:          # the last node: the sample itself
        return y1
    return y0 + (y1 - y0) * (num(xv) - x0) / (x1 - x0)


def tab2(xs, cols, key, xv, yv, num=float):
    i = seg_right(xs, xv)
    alpha = (num(xv) - num(xs[i])) / (num(xs[i + 1]) - num(xs[i]))
    s = []
    for c in (cols[i], cols[i + 1]):
        y, v = c["y"], c[key]
        j = seg_right(y, yv)
        beta = (num(yv) - num(y[j])) / (num(y[j + 1]) - num(y[j]))
        s.append(num(v[j]) * (1 - beta) + num(v[j + 1]) * beta)
    return s[0] * (1 - alpha) + s[1] * alpha


def tab2wg(xs, cols, key, xv, yv, num=float):
    """the wet-gas table: the columns' last samples guide the interpolation; the segments of the shifted arguments are found on
    the doubles the code forms (float statement first), the arithmetic then follows in `num`"""
    i = seg_right(xs, xv)
    c1, c2 = cols[i], cols[i + 1]

    def shifted(n):
        alpha = (n(xv) - n(xs[i])) / (n(xs[i + 1]) - n(xs[i]))
        e0, e1 = n(c1["y"][-1]), n(c2["y"][-1])
        yEnd = e0 * (1 - alpha) + e1 * alpha
        lo = up = n(yv)
        if yEnd > 0:
            shift = (e1 - e0) * n(yv) / yEnd
            lo = n(yv) - alpha * shift
            up = n(yv) + shift - alpha * shift
        return alpha, lo, up
    _, lo_f, up_f = shifted(float)
    alpha, lo, up = shifted(num)
    s = []
    for c, yf, yn in ((c1, lo_f, lo), (c2, up_f, up)):
        y, v = c["y"], c[key]
        j = seg_right(y, yf)
        beta = (yn - num(y[j])) / (num(y[j + 1]) - num(y[j]))
        s.append(num(v[j]) * (1 - beta) + num(v[j + 1]) * beta)
    return s[0] * (1 - alpha) + s[1] * alpha


def pwlin(x, y, xv, num=float):
    n = len(x)
    if xv <= x[0]:
        return num(y[0])
    if xv >= x[n - 1]:
        return num(y[n - 1])
    lo, hi = 0, n - 1
    while lo + 1 < hi:
        mid = (lo + hi) >> 1
        if x[mid] < xv:
            lo = mid
        else:
            hi = mid
    m = (num(y[lo + 1]) - num(y[lo])) / (num(x[lo + 1]) - num(x[lo]))
    return num(y[lo]) + (num(xv) - num(x[lo])) * m


def rs_sat(D, p, num=float):
    return tab1(D["sat_p"], D["sat_rs"], p, num)


def rv_sat(D, p, num=float):
    return tab1(D["wg_xs"], D["wgs_rv"], p, num)


# ---- the exact statement -------------------------------------------------------------------------------------------------------------
PROBE_COLUMNS = ("invBw", "invBg", "invBo", "rsSat", "pcow", "pcgo", "muo", "mug")     # capi.HipFluid.COLUMNS
SAT_COLUMNS = ("krw", "kro", "krg", "pcow", "pcgo")
IQ_COLUMNS = ("invB_w", "invB_o", "invB_g", "mob_w", "mob_o", "mob_g")


def _water(D, pw, num):
    pref, bw, cw, muref, cv = (num(v) for v in D["water"])
    X = cw * (num(pw) - pref)
    ib = (1 + X * (1 + X / 2)) / bw
    Y = (cw - cv) * (num(pw) - pref)
    return ib, (muref * bw) * ib / (1 + Y * (1 + Y / 2))


def _oil(D, po, rs, saturated, num):
    if saturated:
        ib = tab1(D["sat_p"], D["sat_invB"], po, num)
        return ib, ib / tab1(D["sat_p"], D["sat_invBMu"], po, num)
    ib = tab2(D["o_xs"], D["cols"], "invB", rs, po, num)
    return ib, ib / tab2(D["o_xs"], D["cols"], "invBMu", rs, po, num)


def _gas(D, pg, rv, saturated, num):
    if not D["wet"]:
        ib = tab1(D["gas_p"], D["gas_invB"], pg, num)
        return ib, ib / tab1(D["gas_p"], D["gas_invBMu"], pg, num)
    if saturated:
        ib = tab1(D["wg_xs"], D["wgs_invB"], pg, num)
        return ib, ib / tab1(D["wg_xs"], D["wgs_invBMu"], pg, num)
    ib = tab2wg(D["wg_xs"], D["gcols"], "invB", pg, rv, num)
    return ib, ib / tab2wg(D["wg_xs"], D["gcols"], "invBMu", pg, rv, num)


def _rel_perms(S, sw, sg, num):
    """EclDefaultMaterial with the 1e-5 band of the oil relative permeability (update_iq / rel_perms_eps without scaling)"""
    swco = S["swco"]
    krw = pwlin(S["sw"], S["krw"], sw, num)
    krg = pwlin(S["so"], S["krg"], 1.0 - swco - sg, num)
    swm = swco if swco > sw else sw                  # emax(Swco, Sw): (a > b) ? a : b
    sw_ow = sg + swm
    so_go = 1.0 - sw_ow
    kro_ow = pwlin(S["sw"], S["krow"], sw_ow, num)
    kro_go = pwlin(S["so"], S["krog"], so_go, num)
    d = sw_ow - swco                                 # the double the band reads
    eps = 1e-5
    nd = num(sw_ow) - num(swco)
    if d < eps:
        kro2 = (kro_ow + kro_go) / 2
        if d > eps / 2.0:
            kro1 = (num(sg) * kro_go + (num(swm) - num(swco)) * kro_ow) / nd
            alpha = (num(eps) - nd) / (num(eps) / 2)
            kro = kro2 * alpha + kro1 * (1 - alpha)
        else:
            kro = kro2
    else:
        kro = (num(sg) * kro_go + (num(swm) - num(swco)) * kro_ow) / nd
    return krw, kro, krg


def exact(fluid, rows, extras=None, num=Fr, T=None, sat_law=None):
    """-> (probe (N, 8), sat (N, 5), iq (N, 6), mu) as arrays of `num` objects (None where the exact statement divides by zero):
    the columns of capi.HipFluid.probe(p, x3 as Rs, Sw, Sg), of sat_probe(Sw, Sg), and 1/B and the mobilities of the cache; mu: per
    cell the three exact viscosities behind the mobilities.
    sat_law: another law of relative permeability and capillary pressure (tests/sat_states.py: scaled end points, hysteresis):
    sat_law(cell, S, sw, sg, num) -> (krw, kro, krg, pcow, pcgo) in `num`; asked with num = float for the capillary pressures behind
    the phase pressures, which are doubles the code forms"""
    T = T or tables(fluid)
    rows = np.asarray(rows, np.float64)
    N = len(rows)
    extras = extras or {}
    rsmax = extras.get("rsmax")
    rvmax = extras.get("rvmax")
    P = np.empty((N, 8), object)
    Sx = np.empty((N, 5), object)
    Q = np.empty((N, 6), object)
    MU = [[1, 1, 1] for _ in range(N)]

    memo = {}

    def guard(f, *key):
        """f(*key, num), None where it divides by zero; computed once per argument list"""
        k = (f.__name__,) + tuple(id(a) if isinstance(a, dict) else a for a in key)
        if k not in memo:
            try:
                memo[k] = f(*key, num)
            except ZeroDivisionError:
                memo[k] = None
        return memo[k]
    for c in range(N):
        sw, p, x3 = (float(v) for v in rows[c, :3])
        m, pr, sr = (int(v) for v in rows[c, 3:6])
        D, S = T["pvt"][pr], T["sat"][sr]
        swco = S["swco"]
        sg_probe = x3 if m == SW_PO_SG else 0.0
        rs_probe = x3 if m == SW_PO_RS else 0.0
        # -- the probes: one pressure for every phase --
        w_ = guard(_water, D, p)
        P[c, 0] = None if w_ is None else w_[0]
        gas = guard(_gas, D, p, 0.0, True)
        P[c, 1], P[c, 7] = (None, None) if gas is None else gas
        try:
            sat_f = rs_probe >= rs_sat(D, p)
        except ZeroDivisionError:
            sat_f = None
        P[c, 3] = guard(rs_sat, D, p)
        oil = None if sat_f is None else guard(_oil, D, p, rs_probe, bool(sat_f))
        P[c, 2], P[c, 6] = (None, None) if oil is None else oil
        if sat_law is None:
            P[c, 4] = pwlin(S["sw"], S["pcow"], sw, num)
            P[c, 5] = pwlin(S["so"], S["pcgo"], 1.0 - swco - sg_probe, num)
            kr = guard(_rel_perms, S, sw, sg_probe)
        else:
            law = sat_law(c, S, sw, sg_probe, num)
            kr, P[c, 4], P[c, 5] = law[:3], law[3], law[4]
        Sx[c, :3] = kr
        Sx[c, 3], Sx[c, 4] = P[c, 4], P[c, 5]
        # -- the cache: update_iq's own decisions, on the doubles it forms --
        if m == SW_PO_SG:
            sg = x3
        elif m == SW_PG_RV:
            sg = 1.0 - sw
        else:
            sg = 0.0
        so = 1.0 - sw - sg
        if sat_law is None:
            pcw_f = pwlin(S["sw"], S["pcow"], sw)
            pcg_f = pwlin(S["so"], S["pcgo"], 1.0 - swco - sg)
        else:
            pcw_f, pcg_f = (float(v) for v in sat_law(c, S, sw, sg, float)[3:5])
        pC = (-pcw_f, 0.0, pcg_f)
        ref = 2 if m == SW_PG_RV else 1
        pph = [p + (pC[k] - pC[ref]) for k in range(3)]
        cap = float(rsmax[c]) if rsmax is not None else float(np.finfo(np.float64).max) / 2.0
        try:
            if m == SW_PO_RS:
                rs = cap if cap < x3 else x3         # emin(RsMax, Rs): (a < b) ? a : b
            else:
                r = rs_sat(D, pph[1])
                rs = cap if cap < r else r
            saturated = sg > 0.0 and rs >= (1.0 - 1e-10) * rs_sat(D, pph[1])
            rv, gsat = 0.0, False
            if D["wet"]:
                vcap = float(rvmax[c]) if rvmax is not None else float(np.finfo(np.float64).max) / 2.0
                if m == SW_PG_RV:
                    rv = vcap if vcap < x3 else x3
                else:
                    r = rv_sat(D, pph[2])
                    rv = vcap if vcap < r else r
                gsat = so > 0.0 and rv >= (1.0 - 1e-10) * rv_sat(D, pph[2])
        except ZeroDivisionError:
            Q[c, :] = None
            continue
        krc = guard(_rel_perms, S, sw, sg) if sat_law is None else sat_law(c, S, sw, sg, num)[:3]
        w = guard(_water, D, pph[0])
        o = guard(_oil, D, pph[1], rs, bool(saturated)) if math.isfinite(rs) else None
        g = guard(_gas, D, pph[2], rv, bool(gsat))
        for k, ph in enumerate((w, o, g)):
            Q[c, k] = None if ph is None else ph[0]
            Q[c, 3 + k] = None if ph is None or ph[1] == 0 else krc[k] / ph[1]
            if ph is not None and ph[1] != 0:
                MU[c][k] = ph[1]
    return P, Sx, Q, MU


def scales(fluid, pvt=0, sat=0, T=None):
    """per column of exact()'s three arrays, the largest magnitude among the samples the quantity is interpolated from (for a mobility:
    the relative permeability's, which relative_distance puts over the cell's own viscosity)"""
    T = T or tables(fluid)
    D, S = T["pvt"][pvt], T["sat"][sat]
    mx = lambda v: max(abs(float(x)) for x in v)
    oib = mx([x for c in D["cols"] for x in c["invB"]])
    omu = mx([a / b for c in D["cols"] for a, b in zip(c["invB"], c["invBMu"])])
    if D["wet"]:
        gib = mx([x for c in D["gcols"] for x in c["invB"]])
        gmu = mx([a / b for c in D["gcols"] for a, b in zip(c["invB"], c["invBMu"])])
    else:
        gib, gmu = mx(D["gas_invB"]), mx([a / b for a, b in zip(D["gas_invB"], D["gas_invBMu"])])
    kr = (mx(S["krw"]), max(mx(S["krow"]), mx(S["krog"])), mx(S["krg"]))
    probe = (1.0 / D["water"][1], gib, oib, mx(D["sat_rs"]), mx(S["pcow"]), mx(S["pcgo"]), omu, gmu)
    return probe, kr + (mx(S["pcow"]), mx(S["pcgo"])), (1.0 / D["water"][1], oib, gib) + kr


def relative_distance(got, want, scale, mu=None):
    """max over the entries with an exact value of |got - want| / max(|want|, s): s = scale[column], the largest sample of the curves
    the column is interpolated from (for a mobility, with mu given: that of the relative permeability over the cell's exact
    viscosity).  Relative to the result alone where the result is of the samples' size; relative to the operands where the
    interpolation cancels - one ulp beyond a node at which a relative permeability is zero the value is 1e-19 and carries the rounding
    of operands of size 1.  -> (the maximum as a float, (row, column) where)"""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, object)
    worst, where = 0.0, None
    for c in range(got.shape[0]):
        for k in range(got.shape[1]):
            w = want[c, k]
            if w is None:
                continue
            g = float(got[c, k])
            if not math.isfinite(g):
                return math.inf, (c, k)
            wf = float(w)
            sf = float(scale[k]) if mu is None or k < 3 else float(scale[k]) / abs(float(mu[c][k - 3]))
            if max(abs(wf), sf) > 0.0 and abs(g - wf) / max(abs(wf), sf) + 4.5e-16 <= worst:
                continue                              # (cannot be the maximum: the doubles themselves say so)
            d = abs(Fr(g) - Fr(w))
            if d == 0:
                continue
            s = Fr(float(scale[k]))
            if mu is not None and k >= 3:
                s = s / abs(mu[c][k - 3])
            r = float(d / max(abs(Fr(w)), s)) if max(abs(Fr(w)), s) != 0 else math.inf
            if r > worst:
                worst, where = r, (c, k)
    return worst, where


# ---- the states --------------------------------------------------------------------------------------------------------------------
class _Rows:
    def __init__(self, pr, sr):
        self.rows, self.labels, self.rsmax, self.rvmax = [], [], [], []
        self.pr, self.sr = pr, sr

    def add(self, label, sw, p, x3, meaning, rsmax=NO_CAP, rvmax=NO_CAP):
        self.rows.append((float(sw), float(p), float(x3), float(meaning), float(self.pr), float(self.sr)))
        self.labels.append(label)
        self.rsmax.append(float(rsmax))
        self.rvmax.append(float(rvmax))


def _spread(values, least=8):
    """how many companions each of `values` needs for its label to reach `least` cells"""
    return max(2, -(-least // max(1, len(values))))


def _position(i, n):
    return "first" if i == 0 else "last" if i == n - 1 else "interior"


def _sg_for(swco, target):
    """an Sg at which the double (1 - Swco) - Sg, the argument of the gas-oil tables, is `target`; None if no double does it"""
    g = (1.0 - swco) - target
    for k in range(-4, 5):
        c = g
        for _ in range(abs(k)):
            c = above(c) if k > 0 else below(c)
        if (1.0 - swco) - c == target:
            return c
    return None


def _diff_neighbours(swco, target):
    """doubles s near swco + target: -> {"-": the s whose (s - swco) is the largest below target, "0": the s with (s - swco) == target
    if there is one, "+": the smallest above}.  (The difference of two doubles this close is exact, so the double the band reads
    moves in steps of ulp(s): the target itself is met only where it is such a step.)"""
    out = {}
    s = swco + target
    cand = [s]
    for _ in range(3):
        cand = [below(cand[0])] + cand + [above(cand[-1])]
    lo = [c for c in cand if c - swco < target]
    hi = [c for c in cand if c - swco > target]
    eq = [c for c in cand if c - swco == target]
    out["-"] = max(lo)
    out["+"] = min(hi)
    if eq:
        out["0"] = eq[0]
    return out


def states(fluid, pvt=0, sat=0, kind="full"):
    """-> (rows (N, 6), labels [N], extras dict(rsmax (N,), rvmax (N,) - wet gas only -, rocknum (N,) - with ROCKTAB only))
    kind = "full": every label of the module docstring of tests/test_table_states.py that the fluid's tables offer;
    kind = "equal_bubble_point": the states about the shared bubble point of a fluid whose first two PVTO nodes have one."""
    T = tables(fluid)
    D, S = T["pvt"][pvt], T["sat"][sat]
    R = _Rows(pvt, sat)
    swco = S["swco"]
    wet = D["wet"]
    rsat = lambda p: rs_sat(D, p)
    p_mid = 0.5 * (D["sat_p"][0] + D["sat_p"][-1])
    if kind == "equal_bubble_point":
        pb = D["sat_p"][0]
        assert D["sat_p"][1] == pb
        for name, p in [("half", 0.5 * pb)] + [("at" + s, v) for s, v in triple(pb)] + [("twice", 2.0 * pb), ("above", 5.0 * pb)]:
            for k in range(8):
                sw = 0.2 + 0.05 * k
                R.add("eqbp:%s:rs" % name, sw, p, D["o_xs"][0] + (D["o_xs"][1] - D["o_xs"][0]) * k / 8.0, SW_PO_RS)
                R.add("eqbp:%s:sg" % name, sw, p, 0.02 * k, SW_PO_SG)
        return _finish(fluid, R)
    # companions of a pressure: (Sw, what the third variable is, its size)
    comp = [(0.2, "rs", 0.5), (0.35, "sg", 0.1), (0.3, "rs", 0.0), (0.5, "sg", 0.3), (0.25, "rs", 1.0), (0.3, "sg", 0.0), (0.6, "rs", 0.9), (0.45, "sg", 0.25)]
    if wet:
        comp = comp[:4] + [(0.2, "rv", 0.5), (0.3, "rv", 1.0), (0.4, "rv", 0.0), (0.15, "rv", 0.8)]

    def at_pressure(label, p, k):
        for sw, what, f in comp[:k]:
            if what == "rs":
                R.add(label, sw, p, f * rsat(p), SW_PO_RS)
            elif what == "sg":
                R.add(label, sw, p, f, SW_PO_SG)
            else:
                R.add(label, sw, p, f * rv_sat(D, p), SW_PG_RV)

    # ---- pressure ----
    ptabs = [("sat_p", D["sat_p"])]
    ptabs.append(("pvtg", D["wg_xs"]) if wet else ("pvdg", D["gas_p"]))
    for t, Rk in enumerate(T["rock"]):
        ptabs.append(("rocktab%d" % t, Rk["p"]))
    for name, nodes in ptabs:
        n = len(nodes)
        k_int = _spread(nodes[1:-1])
        for i, v in enumerate(nodes):
            pos = _position(i, n)
            for suf, pv_ in triple(v):
                at_pressure("p:%s:%s%s" % (name, pos, suf), pv_, 8 if pos != "interior" else k_int)
        at_pressure("p:%s:half_first" % name, 0.5 * nodes[0], 8)
        at_pressure("p:%s:twice_last" % name, 2.0 * nodes[-1], 8)
    ncol = len(D["cols"])
    for i, c in enumerate(D["cols"]):
        n = len(c["y"])
        for j, v in enumerate(c["y"]):
            pos = _position(j, n)
            for suf, pv_ in triple(v):
                for sw in (0.2, 0.4, 0.3, 0.5)[:max(1, -(-4 // ncol))]:
                    for f in (1.0, 0.999):                   # on the column and a little to its left
                        R.add("p:pvto_col:%s%s" % (pos, suf), sw + 0.05 * (f < 1.0), pv_, D["o_xs"][i] * f, SW_PO_RS)
        for sw in (0.2, 0.3, 0.4, 0.5):
            R.add("p:pvto_col:half_first", sw, 0.5 * c["y"][0], D["o_xs"][i], SW_PO_RS)
            R.add("p:pvto_col:twice_last", sw, 2.0 * c["y"][-1], D["o_xs"][i], SW_PO_RS)
    # ---- Rs ----
    xs = D["o_xs"]
    for i, v in enumerate(xs):
        pos = _position(i, len(xs))
        k = 8 if pos != "interior" else _spread(xs[1:-1])
        for suf, r in triple(v):
            for q in range(k):
                R.add("rs:node:%s%s" % (pos, suf), 0.2 + 0.04 * q, D["sat_p"][i] * (1.05 + 0.15 * q), r, SW_PO_RS)
    for q in range(8):
        p = D["sat_p"][0] + (D["sat_p"][-1] - D["sat_p"][0]) * (q + 0.37) / 8.0
        sw = 0.15 + 0.05 * q
        sat_rs = rsat(p)
        R.add("rs:zero", sw, p, 0.0, SW_PO_RS)
        R.add("rs:1.5last", sw, p, 1.5 * xs[-1], SW_PO_RS)
        R.add("rs:rssat", sw, p, sat_rs, SW_PO_RS)
        thr = (1.0 - 1e-10) * sat_rs
        for suf, r in triple(thr):
            R.add("rs:threshold%s" % suf, sw, p, r, SW_PO_RS)
            # the threshold of `saturated` is read only with gas present, where Rs = min(RsMax, RsSat): the cap puts Rs on it
            R.add("rsmax:threshold%s:sg" % suf, sw, p, 0.05 + 0.02 * q, SW_PO_SG, rsmax=r)
        R.add("rsmax:above", sw, p, 0.8 * sat_rs, SW_PO_RS, rsmax=0.6 * sat_rs)
        R.add("rsmax:on", sw, p, 0.6 * sat_rs, SW_PO_RS, rsmax=0.6 * sat_rs)
        R.add("rsmax:below_rssat:sg", sw, p, 0.1, SW_PO_SG, rsmax=0.6 * sat_rs)
    # ---- pairs (Rs node i, sample j of its column): alpha = 0 and beta1 = 0 (or 1) exactly ----
    for i, c in enumerate(D["cols"]):
        for j, v in enumerate(c["y"]):
            for sw in (0.2, 0.45, 0.7, 0.95):
                R.add("pair:%s_column" % ("extended" if c["extended"] else "deck"), sw, v, xs[i], SW_PO_RS)
    # ---- Sw ----
    nodes = S["sw"]
    p0 = p_mid
    scomp = [("rs", 0.5), ("sg", 0.1), ("sg", 0.0), ("rs", 1.0), ("sg", 0.3), ("rs", 0.0), ("sg", 0.05), ("rs", 0.8)]
    if wet:
        scomp = scomp[:5] + [("rv", 0.5), ("rv", 1.0), ("rv", 0.0)]

    def at_sw(label, sw, k):
        for q, (what, f) in enumerate(scomp[:k]):
            p = p0 * (0.8 + 0.05 * q)
            if what == "rs":
                R.add(label, sw, p, f * rsat(p), SW_PO_RS)
            elif what == "sg":
                R.add(label, sw, p, f, SW_PO_SG)
            else:
                R.add(label, sw, p, f * rv_sat(D, p), SW_PG_RV)
    for i, v in enumerate(nodes):
        pos = "swco" if i == 0 else _position(i, len(nodes))
        for suf, s in triple(v):
            at_sw("sw:%s%s" % (pos, suf), s, 8 if pos != "interior" else _spread(nodes[1:-1]))
    at_sw("sw:negative", -0.05, 8)
    at_sw("sw:one", 1.0, 8)
    at_sw("sw:above_one", 1.07, 8)
    # ---- Sg: the argument (1 - Swco) - Sg of the gas-oil tables on every node ----
    nodes = S["so"]
    for i, v in enumerate(nodes):
        pos = _position(i, len(nodes))
        k = 8 if pos != "interior" else _spread(nodes[1:-1])
        for suf, t in triple(v):
            sg = _sg_for(swco, t)
            if sg is None:      # (no double lands there: the neighbour on that side of the node does)
                continue
            for q in range(k):
                R.add("sg:node:%s%s" % (pos, suf), (0.1, 0.2, swco, 0.3, 0.05, 0.4, 0.25, 0.15)[q], p0 * (0.8 + 0.05 * q), sg, SW_PO_SG)
    for name, sg in (("zero", 0.0), ("smallest_positive", 5e-324), ("negative_zero", -0.0), ("negative", -0.03)):
        for q in range(8):
            R.add("sg:%s" % name, 0.15 + 0.07 * q, p0 * (0.8 + 0.05 * q), sg if name != "negative" else sg * (1 + q), SW_PO_SG)
    # ---- the band of the oil relative permeability: (Sg + max(Swco, Sw)) - Swco about 1e-5 and 0.5e-5 ----
    for tname, target in (("eps", 1e-5), ("half_eps", 0.5e-5), ("mid", 0.75e-5)):
        by_sw = _diff_neighbours(swco, target)                 # Sg = 0: Sw = Swco + target
        for suf, s in by_sw.items():
            if tname == "mid" and suf != "0" and "0" in by_sw:
                continue
            for q in range(8):
                R.add("band:%s%s:sg_zero" % (tname, suf if tname != "mid" else ""), s, p0 * (0.8 + 0.05 * q), 0.0 if q % 2 else 0.5 * rsat(p0 * (0.8 + 0.05 * q)),
                      SW_PO_SG if q % 2 else SW_PO_RS)
        for suf, s in by_sw.items():                                  # Sg > 0 under Sw <= Swco: Sg + Swco rounds to the same doubles
            if tname == "mid" and suf != "0" and "0" in by_sw:
                continue
            sg = s - swco
            if sg + swco != s:
                cands = [c for c in (below(sg), above(sg)) if c + swco == s]
                if not cands:
                    continue
                sg = cands[0]
            for q in range(8):
                R.add("band:%s%s:sg_positive" % (tname, suf if tname != "mid" else ""), swco * (1.0 - 0.1 * q), p0 * (0.8 + 0.05 * q), sg, SW_PO_SG)
    # ---- wet gas: Rv, RvSat, the third meaning ----
    if wet:
        gx = D["wg_xs"]
        for i, c in enumerate(D["gcols"]):
            pos_i = _position(i, len(gx))
            for j, v in enumerate(c["y"]):
                pos = _position(j, len(c["y"]))
                for suf, r in triple(v):
                    for sw in (0.2, 0.5):
                        R.add("rv:node:%s%s" % (pos, suf), sw, gx[i], r, SW_PG_RV)
                        R.add("rv:node:%s%s" % (pos, suf), sw, gx[i] * 1.003 if pos_i != "last" else gx[i] * 0.997, r, SW_PG_RV)
        for q in range(8):
            p = gx[0] + (gx[-1] - gx[0]) * (q + 0.37) / 8.0
            sw = 0.15 + 0.05 * q
            sat_rv = rv_sat(D, p)
            R.add("rv:zero", sw, p, 0.0, SW_PG_RV)
            R.add("rv:1.5last", sw, p, 1.5 * max(D["wgs_rv"]), SW_PG_RV)
            R.add("rv:rvsat", sw, p, sat_rv, SW_PG_RV)
            for suf, r in triple((1.0 - 1e-10) * sat_rv):
                R.add("rv:threshold%s" % suf, sw, p, r, SW_PG_RV)
                R.add("rvmax:threshold%s:sg" % suf, sw, p, 0.05 + 0.02 * q, SW_PO_SG, rvmax=r)
            R.add("rvmax:above", sw, p, 0.8 * sat_rv, SW_PG_RV, rvmax=0.6 * sat_rv)
            R.add("rvmax:on", sw, p, 0.6 * sat_rv, SW_PG_RV, rvmax=0.6 * sat_rv)
    return _finish(fluid, R)


def _finish(fluid, R):
    rows = np.array(R.rows, np.float64).reshape(-1, 6)
    extras = dict(rsmax=np.array(R.rsmax))
    if fluid.wet_gas:
        extras["rvmax"] = np.array(R.rvmax)
    if fluid.rocktab:      # a cell on a ROCKTAB node reads that table, the others take turns
        own = [int(l.split(":")[1][len("rocktab"):]) if l.startswith("p:rocktab") else c % len(fluid.rocktab) for c, l in enumerate(R.labels)]
        extras["rocknum"] = np.array(own, np.int32)
    return rows, list(R.labels), extras


def census(labels):
    n = {}
    for l in labels:
        n[l] = n.get(l, 0) + 1
    return n


def case_of(pkg, fluid, rows, extras=None, pvtnum=None, satnum=None):
    """the rows as the cells of an N x 1 x 1 grid (a case dict for capi.HipModel / oracle_bind.OracleModel)"""
    rows = np.asarray(rows, np.float64)
    N = len(rows)
    with np.errstate(divide="ignore", invalid="ignore"):
        case = pkg.decks.cartesian_case(N, 1, 1, state="undersaturated", perturb=False, fluid=fluid)
    case["pv"] = np.ascontiguousarray(rows[:, :3].reshape(-1))
    case["meaning"] = rows[:, 3].astype(np.uint8)
    case["pvtnum"] = np.ascontiguousarray(rows[:, 4].astype(np.int32) if pvtnum is None else pvtnum, np.int32)
    case["satnum"] = np.ascontiguousarray(rows[:, 5].astype(np.int32) if satnum is None else satnum, np.int32)
    for k, v in (extras or {}).items():
        case[k] = np.ascontiguousarray(v)
    return case


# ---- fluids ------------------------------------------------------------------------------------------------------------------------
def two_row_fluid(pkg):
    """the least the builder accepts: SWOF, SGOF, PVDG and ROCKTAB of two rows each, PVTO of two Rs nodes (the first with its saturated
    sample alone).  Swco = 0, so that (Sg + Sw) - Swco can be 1e-5 to the bit; a capillary pressure between oil and water"""
    bar = 1e5
    pvt = [dict(pvtw=[250 * bar, 1.03, 4.5e-10, 0.35e-3, 1e-10], density=[850.0, 1030.0, 0.9],
                pvdg=[[50 * bar, 0.02, 1.4e-5], [400 * bar, 0.004, 2.6e-5]],
                pvto=[dict(rs=10.0, p=[60 * bar], bo=[1.1], mu=[1.2e-3]),
                      dict(rs=150.0, p=[280 * bar, 450 * bar], bo=[1.5, 1.45], mu=[0.5e-3, 0.6e-3])])]
    sat = [dict(swof=[[0.0, 0.0, 0.9, 0.4 * bar], [1.0, 0.7, 0.0, 0.0]], sgof=[[0.0, 0.0, 0.9, 0.0], [0.8, 0.85, 0.0, 0.0]])]
    return pkg.fluid.Fluid(pvt, sat, rock_pref=1 * bar, rock_cr=4e-10, rocktab=[[[100 * bar, 0.95, 0.9], [400 * bar, 1.02, 1.05]]])


def uneven_columns_fluid(pkg):
    """the SPE1 fluid with PVTO columns of different lengths: the last Rs node with four samples, the one before with three (the
    seven single-sample nodes before it then take its length); the added samples continue the columns' last steps"""
    fl = pkg.fluid.spe1_fluid()[0]
    pvt = copy.deepcopy(fl.pvt)
    for n, extra in zip(pvt[0]["pvto"][-2:], (1, 2)):
        for _ in range(extra):
            n["p"].append(n["p"][-1] + 0.8 * (n["p"][-1] - n["p"][-2]))
            n["bo"].append(n["bo"][-1] * (1.0 - 0.7 * (1.0 - n["bo"][-1] / n["bo"][-2])))
            n["mu"].append(n["mu"][-1] * (1.0 + 0.9 * (n["mu"][-1] / n["mu"][-2] - 1.0)))
    return pkg.fluid.Fluid(pvt, fl.sat, rock_pref=fl.rock_pref, rock_cr=fl.rock_cr)


def equal_bubble_point_fluid(pkg):
    """the fluid of the reference's tests/SUMMARY_DECK_NON_CONSTANT_POROSITY.DATA (helpers.summary_deck_case): Rs = 0 and Rs = 1 both
    saturated at 1 bar"""
    import helpers
    return helpers.summary_deck_case(pkg)[0]["fluid"]


def _resampled(rows, n, scale):
    """a table of n rows on an even grid over the first column's range, the other columns interpolated and scaled"""
    a = np.asarray(rows, float)
    x = np.linspace(a[0, 0], a[-1, 0], n)
    x[0], x[-1] = a[0, 0], a[-1, 0]
    cols = [x] + [np.interp(x, a[:, 0], a[:, k]) * scale[k - 1] for k in range(1, a.shape[1])]
    return np.stack(cols, axis=1).tolist()


def sat_region_copy(s0, k, nw=None, ng=None):
    """saturation region number k of a padding: the curves of s0, scaled a little differently for every k; nw / ng: other row counts"""
    f = 1.0 - 0.002 * (1 + k % 89)
    sc = (f, 1.0 - 0.5 * (1.0 - f), 1.0 + 0.01 * (k % 7))
    if nw is None and ng is None:
        return dict(swof=[[r[0], sc[0] * r[1], sc[1] * r[2], sc[2] * r[3]] for r in s0["swof"]],
                    sgof=[[r[0], sc[1] * r[1], sc[0] * r[2], sc[2] * r[3]] for r in s0["sgof"]])
    return dict(swof=_resampled(s0["swof"], nw, sc), sgof=_resampled(s0["sgof"], ng, (sc[1], sc[0], sc[2])))


def pvt_region_copy(p0, k, ng=None):
    """PVT region number k of a padding: region p0 with other densities, water and gas; ng: PVDG resampled to that many rows"""
    p1 = copy.deepcopy(p0)
    f = 1.0 + 0.01 * (1 + k % 13)
    p1["density"] = [p0["density"][0] * f, p0["density"][1] / f, p0["density"][2] * f]
    p1["pvtw"] = [p0["pvtw"][0], p0["pvtw"][1] * f, p0["pvtw"][2] / f, p0["pvtw"][3] * f, p0["pvtw"][4]]
    if "pvdg" in p1:
        p1["pvdg"] = [[r[0], r[1] * f, r[2] / f] for r in p0["pvdg"]] if ng is None else _resampled(p0["pvdg"], ng, (f, 1.0 / f))
    for n in p1["pvto"]:
        n["bo"] = [b * f for b in n["bo"]]
        n["mu"] = [m / f for m in n["mu"]]
    return p1


def padded_fluid(pkg, base, target=None, sat_regions=None, where="after"):
    """`base` with further regions, each a scaled copy of region 0's curves.
    target: the double blob is to have exactly this many entries: whole copies of saturation region 0 first, then one PVT region whose
            PVDG has the row count, and one saturation region with the row counts, that meet the number exactly;
    sat_regions: instead, that many saturation regions in all (whole copies only).
    where = "after": the regions of `base` keep their numbers; "before": they come LAST, behind the padding, so that a cell which keeps
            `base`'s curves has the largest region numbers and the largest offsets into the blob."""
    p0, s0 = base.pvt[0], base.sat[0]
    kw = dict(rock_pref=base.rock_pref, rock_cr=base.rock_cr, rocktab=base.rocktab or None, pc_scaling=base.pc_scaling)
    mk = lambda pv, sa: pkg.fluid.Fluid((list(base.pvt) + pv) if where == "after" else (pv + list(base.pvt)),
                                        (list(base.sat) + sa) if where == "after" else (sa + list(base.sat)), **kw)
    if sat_regions is not None:
        return mk([], [sat_region_copy(s0, k) for k in range(sat_regions - len(base.sat))])
    have = blob_doubles(base)
    one_sat = blob_doubles(mk([], [sat_region_copy(s0, 0)])) - have
    pvt_fixed = blob_doubles(mk([pvt_region_copy(p0, 0, ng=2 if "pvdg" in p0 else None)], [])) - have - (6 if "pvdg" in p0 else 0)
    dry = "pvdg" in p0
    for copies in range((target - have) // one_sat, -1, -1):
        rest = target - have - copies * one_sat - pvt_fixed - (4 * 0 + 1 + EPS_COUNT)
        # rest = 3 ng (PVDG rows, dry gas only) + 4 (nw + ng_s)
        for ng in (range(2, 40) if dry else [0]):
            r = rest - 3 * ng
            if r >= 16 and r % 4 == 0 and r // 4 <= 150:
                nw = r // 8 if r // 8 >= 2 else 2
                sa = [sat_region_copy(s0, k) for k in range(copies)] + [sat_region_copy(s0, copies, nw=nw, ng=r // 4 - nw)]
                fl = mk([pvt_region_copy(p0, 0, ng=ng if dry else None)], sa)
                assert blob_doubles(fl) == target, (blob_doubles(fl), target)
                return fl
    raise ValueError("no padding of %d doubles reaches %d" % (have, target))


def edge_fluids(pkg):
    """every fluid tests/test_table_states.py and tests/test_gpu_table_edges.py use -> {name: (fluid, doubles its blob is cut to or None)}"""
    import helpers
    from test_gpu_assembly import two_region_fluid
    spe1 = pkg.fluid.spe1_fluid()[0]
    wet = helpers.wetgas_fluid(pkg, helpers.ROCKTAB_2)
    out = {"spe1": (spe1, None), "two_region": (two_region_fluid(pkg), None), "wet_rocktab": (wet, None), "two_row": (two_row_fluid(pkg), None), "uneven_columns": (uneven_columns_fluid(pkg), None),
           "equal_bubble_point": (equal_bubble_point_fluid(pkg), None)}
    for where in ("after", "before"):
        for n in (TAB_LDS_DBL, TAB_LDS_DBL + 1):
            out["spe1_%d_%s" % (n, where)] = (padded_fluid(pkg, spe1, n, where=where), n)
    out["wet_rocktab_%d_before" % (TAB_LDS_DBL + 1)] = (padded_fluid(pkg, wet, TAB_LDS_DBL + 1, where="before"), TAB_LDS_DBL + 1)
    for where in ("after", "before"):
        out["norne_sized_%s" % where] = (padded_fluid(pkg, out["two_region"][0], sat_regions=100, where=where), None)
    return out


EDGE_FLUIDS = ("spe1", "two_region", "wet_rocktab", "two_row", "uneven_columns", "equal_bubble_point")


def edge_states(pkg, name, fluids=None):
    """the labelled states of one of EDGE_FLUIDS (the two-region fluid: in its second PVT and saturation region)
    -> dict(fluid, pvt, sat, rows, labels, extras, case)"""
    fl = (fluids or edge_fluids(pkg))[name][0]
    pr, sr = (1, 1) if name == "two_region" else (0, 0)
    rows, labels, extras = states(fl, pr, sr, kind="equal_bubble_point" if name == "equal_bubble_point" else "full")
    return dict(fluid=fl, pvt=pr, sat=sr, rows=rows, labels=labels, extras=extras, case=case_of(pkg, fl, rows, extras))


def probe_arguments(rows):
    """(p, rs, sw, sg) of the rows for HipFluid.probe / sat_probe: the third variable where it is an Rs or an Sg, else 0"""
    m = rows[:, 3]
    return rows[:, 1], np.where(m == SW_PO_RS, rows[:, 2], 0.0), rows[:, 0], np.where(m == SW_PO_SG, rows[:, 2], 0.0)


def cache_values(iq):
    """the columns IQ_COLUMNS of intensive-quantity records (N, fields, 4)"""
    return np.concatenate([iq[:, 6:9, 0], iq[:, 9:12, 0]], axis=1)


def distances(e, probe, sat_probe, iq):
    """the three distances to the exact statement of one fluid's states: the probes', the saturation probes', the cache's"""
    P, S, Q, MU = e["exact"]
    sc = scales(e["fluid"], e["pvt"], e["sat"])
    return [relative_distance(probe, P, sc[0]), relative_distance(sat_probe, S, sc[1]), relative_distance(cache_values(iq), Q, sc[2], MU)]


def on_node_checks(e, probe, last):
    """the statements that hold to the bit, for any source of probe values (the oracle's here, the device's on the GPU): 1/Bg on a
    PVDG node is the builder's sample (last = False: the first and the interior nodes, which tab1 reads as the left end of a segment;
    last = True: the last node, the right end of the last segment, where tab1 returns the sample in place of the interpolated sum), 1/Bo at (Rs node, sample of its column) is the builder's sample and, on a
    deck row, 1.0 / bo of that row.  -> (comparisons made on PVDG nodes, on deck rows, the mismatches)"""
    T = tables(e["fluid"])
    D = T["pvt"][e["pvt"]]
    raw = e["fluid"].pvt[e["pvt"]]
    rows, labels = e["rows"], e["labels"]
    ng = no = 0
    wrong = []
    if not D["wet"]:
        sample = {float(r[0]): 1.0 / float(r[1]) for r in raw["pvdg"]}
        for c, l in enumerate(labels):
            if l.startswith("p:pvdg:") and l.endswith("0") and (l == "p:pvdg:last0") == last:
                ng += 1
                if probe[c, 1] != sample[rows[c, 1]]:
                    wrong.append((l, rows[c, 1], probe[c, 1], sample[rows[c, 1]]))
    if last:
        return ng, 0, wrong
    deck = {}
    for i, n in enumerate(raw["pvto"]):
        for pj, bj in zip(n["p"], n["bo"]):
            deck[(float(n["rs"]), float(pj))] = 1.0 / float(bj)
    built = {(D["o_xs"][i], y): v for i, c in enumerate(D["cols"]) for y, v in zip(c["y"], c["invB"])}
    for c, l in enumerate(labels):
        if l.startswith("pair:"):
            key = (rows[c, 2], rows[c, 1])
            if probe[c, 2] != built[key] or probe[c, 2] != deck.get(key, built[key]):
                wrong.append((l, key, probe[c, 2], built[key]))
            no += key in deck
            assert key in deck or l == "pair:extended_column"
    return ng, no, wrong


def node_slope_checks(e, iq):
    """which segment a node belongs to shows in the derivatives alone: on an interior PVDG node, and one double to its right,
    d(1/Bg)/dp of the cache is the slope of the segment on the RIGHT of the node, one double to its left that of the segment on the
    left, to the bit (tab1); on an interior SWOF node, and one double to its left, d(krw/mu_w)/dSw is the slope of the segment on the
    LEFT over the viscosity, one double to its right that of the right one (pwlin; the tables here have no oil-water capillary
    pressure, so the viscosity does not move with Sw).  Only nodes at which the two slopes differ count.
    -> (comparisons on PVDG nodes, on SWOF nodes, the mismatches); e needs "exact" """
    T = tables(e["fluid"])
    D, S = T["pvt"][e["pvt"]], T["sat"][e["sat"]]
    rows, labels = e["rows"], e["labels"]
    MU = e["exact"][3]
    ng = nw = 0
    wrong = []
    for c, l in enumerate(labels):
        if l.startswith("p:pvdg:interior") and not D["wet"]:
            x, y = D["gas_p"], D["gas_invB"]
            i = int(np.argmin(np.abs(np.array(x) - rows[c, 1])))
            left, right = (y[i] - y[i - 1]) / (x[i] - x[i - 1]), (y[i + 1] - y[i]) / (x[i + 1] - x[i])
            want = left if l.endswith("-") else right
            if left != right:
                ng += 1
                if iq[c, 8, 2] != want:
                    wrong.append((l, rows[c, 1], iq[c, 8, 2], want))
        if l.startswith("sw:interior") and not any(S["pcow"]):
            x, y = S["sw"], S["krw"]
            i = int(np.argmin(np.abs(np.array(x) - rows[c, 0])))
            left, right = (y[i] - y[i - 1]) / (x[i] - x[i - 1]), (y[i + 1] - y[i]) / (x[i + 1] - x[i])
            want, other = (right, left) if l.endswith("+") else (left, right)
            if left != right:
                nw += 1
                got = iq[c, 9, 1] * float(MU[c][0])
                if not (abs(got - want) <= 1e-13 * abs(want) and abs(got - want) < abs(got - other)):
                    wrong.append((l, rows[c, 0], got, want, other))
    return ng, nw, wrong

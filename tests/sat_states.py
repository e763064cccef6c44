"""States that sit where the two layers above the plain saturation-table lookups change their answer - saturation end-point scaling
(eps_*, cap_pressures_eps, rel_perms_eps of csrc/assemble.hip) and relative-permeability hysteresis (sat_curve, pwlin_inv,
sat_curve_inv, rel_perms_hyst, k_hyst_update) - with a label each, and an exact statement of both layers to hold the CPU oracle and
the device against.  Built on tests/table_states.py: its notation (v-, v, v+ = a "triple", suffixes "-", "0", "+"), its samples
(tables), its PVT half (exact, through the sat_law hook), its distance (relative_distance).

  sat_fluids(pkg)          the fluids: name -> (fluid, drainage region, imbibition region); every one with pc_scaling
  table_end_points(S)      the end points build_fluid_tables extracts from a region's samples, restated in Python floats
  point_sets(u) / imb_point_set(u)   the per-cell scaled end points, chosen (dyadic, so that the sums the code forms are exact)
  states(...)              end-point scaling: one row per cell, a label per row, the point set of every row
  hyst_states(...)         hysteresis: rows, labels, the turning points handed in, the imbibition region of every row
  exact_sat(...)           krw, kro, krg, pcow, pcgo, the cache's 1/B and mobilities per row; under hysteresis the (turning point,
                           shift) of both systems after opmhip_set_hysteresis_params - all in fractions.Fraction
  census(labels)           rows per kind of edge;  KINDS / HYST_KINDS: the kinds that must be there

Conventions read from the code (csrc/assemble.hip, csrc/fluid_device.hpp):
  pwlin              constant outside the table; a value on a node belongs to the segment on its LEFT
  two-point map      unscaled = u0 + (S - s0) * ((u2 - u0) / (s2 - s0)), no clamp: it extrapolates, pwlin then clamps
  three-point map    S <= s0 -> u0;  S <= s1 -> first segment;  u1 == u2 (UNSCALED points) -> u1;  S <= s2 -> second segment;  else u2.
                     A value on a scaled point belongs to the piece on its LEFT (`<=`).
  inverse three-point map (sat_curve_inv)   Su <= u0 -> s0;  Su < u1 -> first segment;  Su < u2 -> second segment;  else s2.
                     A value on u1 or u2 belongs to the piece on its RIGHT (`<`): the asymmetry with the forward map is the code's.
  vertical scaling   mode 1: kr * (scaled max / table max).  Mode 2, wetting curve (krw, krog), sr = min(s1, s2): !(S > sr) ->
                     kr * (scaled value at sr / table value there);  else, table max > table value at the displacing critical
                     saturation -> linear in kr between the two scaled values;  else sr < s2 -> linear in S;  else the scaled max.
                     Non-wetting curve (krow, krg): mirrored, sr = max(s1, s0), !(S < sr).  S on sr belongs to the lower piece.
  kro blend          d = Sw_ow - SwcoS with SwcoS the CELL's scaled SWL (the table's Swco without saturation scaling): d < 1e-5 ->
                     blend, d > 0.5e-5 -> ramp; both comparisons strict
  rel_perms_hyst     S <= turning point -> drainage curve, else the imbibition curve at S + shift
  k_hyst_update      s < turning point (strict) -> the turning point moves to s and the shift is recomputed; Sg clamped to [0, 1]
  pwlin_inv          decreasing curve (y[0] > y[n-1]): yv >= y[0] -> x[0];  yv <= y[n-1] -> x[n-1] - the value 0 of a curve with
                     trailing zeros inverts to the table's LAST node, not to the critical saturation;  inside, the segment is the
                     last one whose left sample is >= yv: a value on a node gives the node, a value on a plateau the plateau's
                     RIGHT end.  Any other curve (y[0] <= y[n-1], a curve that is zero everywhere included) takes the increasing
                     form: yv <= y[0] -> x[0];  yv >= y[n-1] -> x[n-1];  inside, the last segment whose left sample is <= yv: a
                     plateau's RIGHT end again.

The exact statement takes every decision from the doubles the code compares and does the arithmetic of the chosen branch without
rounding.  Arguments the code computes from the state (1 - SwcoS - Sg, Sg + Sw, 1 - Sw_ow, S + shift, 1 - So) and the end points it
computes from the cell's (1 - SOWCR - SGL, ...) enter as the doubles the code forms; everything after them - the maps, the lookup,
the vertical scaling, the blend, the inversion - is exact.  Both run side by side in a Dual: .f the double, .n the exact value."""
from fractions import Fraction as Fr

import numpy as np

import table_states as ts
from table_states import triple, below, above, pwlin, tables, case_of, relative_distance, _Rows, _sg_for, _diff_neighbours, SW_PO_SG

(SWL, SWCR, SWU, SOWCR, SGL, SGCR, SGU, SOGCR, MAXPCOW, MAXPCGO, MAXKRW, MAXKROW, MAXKRG, MAXKROG, KRWR, KRORW, KRGR, KRORG) = range(18)
KRW_OW, KRN_OW, KRW_GO, KRN_GO = range(4)
CURVES = ("krw_ow", "krn_ow", "krw_go", "krn_go", "pc_ow", "pc_go")
P_STATE = 200e5
# the largest distance (table_states.relative_distance) between the CPU oracle and exact_sat over every row of every fluid and
# configuration of tests/test_sat_states.py, measured there (test_the_recorded_bound_is_the_measured_one prints it: a mobility of oil
# of the plateau fluid one ulp above the second point of krog's map, two-point scaling with vertical mode 2); the tests hold the
# oracle to it and the device to four times it - the room for another order of the same few operations
ORACLE_TO_EXACT = 5.1571675729676312e-16
BOUND = 4.0 * ORACLE_TO_EXACT


# ---- numbers that carry the double the code forms and the exact value side by side ----------------------------------------------
class Dual:
    __slots__ = ("f", "n")

    def __init__(self, f, n):
        self.f, self.n = f, n

    def _o(self, o):
        return o if isinstance(o, Dual) else Dual(float(o), type(self.n)(float(o)))

    def __add__(self, o):
        o = self._o(o)
        return Dual(self.f + o.f, self.n + o.n)

    def __sub__(self, o):
        o = self._o(o)
        return Dual(self.f - o.f, self.n - o.n)

    def __rsub__(self, o):
        return self._o(o) - self

    def __mul__(self, o):
        o = self._o(o)
        return Dual(self.f * o.f, self.n * o.n)

    def __truediv__(self, o):
        o = self._o(o)
        return Dual(self.f / o.f, self.n / o.n)

    __radd__, __rmul__ = __add__, __mul__

    def __neg__(self):
        return Dual(-self.f, -self.n)


def K(v, num):
    """a double the code holds: exact as it stands"""
    return Dual(float(v), num(float(v)))


# ---- the end points -----------------------------------------------------------------------------------------------------------------
def table_end_points(S):
    """build_fluid_tables' end points of a region (csrc/fluid_tables.cpp; S: one entry of tables(fluid)["sat"]): connate = first row,
    maximum = last row, critical = the last saturation at which the phase's relative permeability is still zero"""
    sw, krw, krow = S["sw"], S["krw"], S["krow"]
    sg, krg, krog = S["sg_deck"], S["krg"][::-1], S["krog"][::-1]
    u = [0.0] * 18
    u[SWL], u[SWU], u[SGL], u[SGU] = sw[0], sw[-1], sg[0], sg[-1]
    u[SWCR] = sw[0]
    for i in range(len(sw)):
        if not krw[i] <= 0.0:
            break
        u[SWCR] = sw[i]
    u[SGCR] = sg[0]
    for i in range(len(sg)):
        if not krg[i] <= 0.0:
            break
        u[SGCR] = sg[i]
    gone = sw[-1]
    for i in range(len(sw) - 1, -1, -1):
        if not krow[i] <= 0.0:
            break
        gone = sw[i]
    u[SOWCR] = 1.0 - gone - u[SGL]
    gone = sg[-1]
    for i in range(len(sg) - 1, -1, -1):
        if not krog[i] <= 0.0:
            break
        gone = sg[i]
    u[SOGCR] = 1.0 - gone - u[SWL]
    u[MAXPCOW], u[MAXPCGO] = S["pcow"][0], S["pcgo"][0]
    u[MAXKRW], u[MAXKROW], u[MAXKRG], u[MAXKROG] = krw[-1], krow[0], S["krg"][0], S["krog"][-1]
    u[KRWR] = pwlin(sw, krw, 1.0 - u[SOWCR] - u[SGL])
    u[KRORW] = pwlin(sw, krow, u[SWCR] + u[SGL])
    u[KRORG] = pwlin(S["so"], S["krog"], 1.0 - u[SGCR] - u[SWL])
    u[KRGR] = pwlin(S["so"], S["krg"], u[SOGCR])
    return u


def eps_triples(e):
    """the six EpsTriples of assemble.hip, as the doubles the code forms -> dict over CURVES"""
    return dict(pc_ow=[e[SWL], e[SWU], e[SWU]], krw_ow=[e[SWCR], 1.0 - e[SOWCR] - e[SGL], e[SWU]], krn_ow=[e[SWL] + e[SGL], e[SWCR] + e[SGL], 1.0 - e[SOWCR]],
                pc_go=[1.0 - e[SWL] - e[SGU], 1.0 - e[SWL] - e[SGL], 1.0 - e[SWL] - e[SGL]], krw_go=[e[SOGCR], 1.0 - e[SGCR] - e[SWL], 1.0 - e[SWL] - e[SGL]],
                krn_go=[1.0 - e[SWL] - e[SGU], e[SOGCR], 1.0 - e[SWL] - e[SGCR]])


def interval_ok(s):
    """the interval check of end_points_refusal (csrc/fluid_tables.cpp)"""
    return (s[SWL] < s[SWU] and s[SGL] < s[SGU] and s[SWCR] < s[SWU] and s[SGCR] < s[SGU] and s[SWL] + s[SGL] < 1.0 - s[SOWCR]
            and s[SOGCR] < 1.0 - s[SWL] - s[SGL])


SET_NAMES = ("generic", "swcr_is_swl", "sr_is_sm_ow", "sogcr_is_first_go", "sgcr_is_sgl")


def point_sets(u):
    """the scaled end points of the drainage curves, one list of 18 per SET_NAMES: dyadic saturations (every sum the code forms of
    them is exact), the vertical end values fixed fractions of the table's (max_krog = max_krow: KRO is one keyword)"""
    g = list(u)
    g[SWL], g[SWCR], g[SWU], g[SOWCR] = 0.1875, 0.25, 0.96875, 0.1875
    g[SGL], g[SGCR], g[SGU], g[SOGCR] = 0.03125, 0.09375, 0.78125, 0.15625
    g[MAXPCOW], g[MAXPCGO] = 1.25 * u[MAXPCOW], 0.75 * u[MAXPCGO]
    g[MAXKRW], g[MAXKROW], g[MAXKRG] = 0.8125 * u[MAXKRW], 0.875 * u[MAXKROW], 0.84375 * u[MAXKRG]
    g[MAXKROG] = g[MAXKROW]
    g[KRWR], g[KRORW], g[KRGR], g[KRORG] = 0.5 * g[MAXKRW], 0.625 * g[MAXKROW], 0.5625 * g[MAXKRG], 0.6875 * g[MAXKROG]
    out = [g]
    a = list(g); a[SWCR] = a[SWL]; out.append(a)                              # krn_ow: s0 == s1
    a = list(g); a[SOWCR], a[SWU] = 0.0625, 0.90625; out.append(a)            # krw_ow: 1 - SOWCR - SGL == SWU, s1 == s2 (sr == sm)
    a = list(g); a[SOGCR] = 0.03125; out.append(a)                            # krn_go: SOGCR == 1 - SWL - SGU, s0 == s1
    a = list(g); a[SGCR] = a[SGL]; out.append(a)                              # krw_go: 1 - SGCR - SWL == 1 - SWL - SGL, s1 == s2
    for s in out:
        assert interval_ok(s)
        t = eps_triples(s)
        assert all(t[k][0] <= t[k][1] <= t[k][2] for k in t)
    assert eps_triples(out[1])["krn_ow"][0] == eps_triples(out[1])["krn_ow"][1] and eps_triples(out[2])["krw_ow"][1] == eps_triples(out[2])["krw_ow"][2]
    assert eps_triples(out[3])["krn_go"][0] == eps_triples(out[3])["krn_go"][1] and eps_triples(out[4])["krw_go"][1] == eps_triples(out[4])["krw_go"][2]
    return out


def imb_point_set(u):
    """the scaled end points of the imbibition curves (one set): more oil and gas trapped than point_sets' generic one"""
    g = list(u)
    g[SWL], g[SWCR], g[SWU], g[SOWCR] = 0.1875, 0.28125, 0.96875, 0.25
    g[SGL], g[SGCR], g[SGU], g[SOGCR] = 0.03125, 0.15625, 0.78125, 0.1875
    g[MAXPCOW], g[MAXPCGO] = 1.125 * u[MAXPCOW], 0.875 * u[MAXPCGO]
    g[MAXKRW], g[MAXKROW], g[MAXKRG] = 0.75 * u[MAXKRW], 0.8125 * u[MAXKROW], 0.78125 * u[MAXKRG]
    g[MAXKROG] = g[MAXKROW]
    g[KRWR], g[KRORW], g[KRGR], g[KRORG] = 0.5625 * g[MAXKRW], 0.5 * g[MAXKROW], 0.625 * g[MAXKRG], 0.75 * g[MAXKROG]
    assert interval_ok(g)
    return g


def cfg_of(es):
    """EclEpsConfig bits of an end-point dict (assemble.hip CellStatic::epscfg)"""
    g = lambda k: int(es.get(k, 0))
    return (1 if g("sat_scaling") else 0) | (2 if g("three_point_kr") else 0) | (g("krw") << 2) | (g("kro") << 4) | (g("krg") << 6) | (256 if g("pcw") else 0) | (512 if g("pcg") else 0)


def config(sat_scaling=1, three=0, krw=0, kro=0, krg=0, pcw=1, pcg=1):
    return dict(sat_scaling=sat_scaling, three_point_kr=three, krw=krw, kro=kro, krg=krg, pcw=pcw, pcg=pcg)


# every option in both states, every vertical mode on every curve, the modes mixed
CONFIGS = {"two_v0": config(three=0), "two_v1": config(three=0, krw=1, kro=1, krg=1), "two_v2": config(three=0, krw=2, kro=2, krg=2),
           "three_v0": config(three=1), "three_v1": config(three=1, krw=1, kro=1, krg=1), "three_v2": config(three=1, krw=2, kro=2, krg=2),
           "three_v210_pcw": config(three=1, krw=2, kro=1, krg=0, pcw=1, pcg=0), "two_v021_pcg": config(three=0, krw=0, kro=2, krg=1, pcw=0, pcg=1),
           "three_v102_nopc": config(three=1, krw=1, kro=0, krg=2, pcw=0, pcg=0), "unscaled_sat_v2": config(sat_scaling=0, three=1, krw=2, kro=2, krg=2)}


def endscale_dict(pkg, es, pts):
    """the configuration and per-cell points (N, 18) as the dict capi.HipModel / oracle_bind.OracleModel take"""
    d = dict(es)
    pts = np.asarray(pts, np.float64)
    for f, name in enumerate(pkg.capi.EPS_FIELDS):
        d[name] = np.ascontiguousarray(pts[:, f])
    return d


# ---- the two layers, decisions on .f, arithmetic on both ----------------------------------------------------------------------------
def pwlin_d(x, y, xv, num):
    n = len(x)
    s = xv.f
    if s <= x[0]:
        return K(y[0], num)
    if s >= x[n - 1]:
        return K(y[n - 1], num)
    lo, hi = 0, n - 1
    while lo + 1 < hi:
        mid = (lo + hi) >> 1
        if x[mid] < s:
            lo = mid
        else:
            hi = mid
    m = (K(y[lo + 1], num) - K(y[lo], num)) / (K(x[lo + 1], num) - K(x[lo], num))
    return K(y[lo], num) + (xv - K(x[lo], num)) * m


def two_point(S, u, sc, num):
    return K(u[0], num) + (S - K(sc[0], num)) * ((K(u[2], num) - K(u[0], num)) / (K(sc[2], num) - K(sc[0], num)))


def three_point(S, u, sc, num):
    if S.f <= sc[0]:
        return K(u[0], num)
    if S.f <= sc[1]:
        return K(u[0], num) + (S - K(sc[0], num)) * ((K(u[1], num) - K(u[0], num)) / (K(sc[1], num) - K(sc[0], num)))
    if u[1] == u[2]:
        return K(u[1], num)
    if S.f <= sc[2]:
        return K(u[1], num) + (S - K(sc[1], num)) * ((K(u[2], num) - K(u[1], num)) / (K(sc[2], num) - K(sc[1], num)))
    return K(u[2], num)


def to_unscaled(cfg, S, u, sc, num):
    if not cfg & 1:
        return S
    return three_point(S, u, sc, num) if cfg & 2 else two_point(S, u, sc, num)


def vertical_krw(mode, S, kr, sc, fdisp, fmax, fr, fm, num):
    if mode == 0:
        return kr
    if mode == 1:
        return kr * (K(fm, num) / K(fmax, num))
    sm = sc[2]
    sr = sc[1] if sc[1] < sm else sm
    if not S.f > sr:
        return kr * (K(fr, num) / K(fdisp, num))
    if fmax > fdisp:
        t = (kr - K(fdisp, num)) / (K(fmax, num) - K(fdisp, num))
        return K(fr, num) + t * (K(fm, num) - K(fr, num))
    if sr < sm:
        t = (S - K(sr, num)) / (K(sm, num) - K(sr, num))
        return K(fr, num) + t * (K(fm, num) - K(fr, num))
    return K(fm, num)


def vertical_krn(mode, S, kr, sc, fdisp, fmax, fr, fm, num):
    if mode == 0:
        return kr
    if mode == 1:
        return kr * (K(fm, num) / K(fmax, num))
    sl = sc[0]
    sr = sc[1] if sc[1] > sl else sl
    if not S.f < sr:
        return kr * (K(fr, num) / K(fdisp, num))
    if fmax > fdisp:
        t = (kr - K(fdisp, num)) / (K(fmax, num) - K(fdisp, num))
        return K(fr, num) + t * (K(fm, num) - K(fr, num))
    if sr > sl:
        t = (K(sr, num) - S) / (K(sr, num) - K(sl, num))
        return K(fr, num) + t * (K(fm, num) - K(fr, num))
    return K(fm, num)


_XY = {KRW_OW: ("sw", "krw"), KRN_OW: ("sw", "krow"), KRW_GO: ("so", "krog"), KRN_GO: ("so", "krg")}
_TRI = {KRW_OW: "krw_ow", KRN_OW: "krn_ow", KRW_GO: "krw_go", KRN_GO: "krn_go"}
_VERT = {KRW_OW: (2, vertical_krw, KRWR, MAXKRW), KRN_OW: (4, vertical_krn, KRORW, MAXKROW), KRW_GO: (4, vertical_krw, KRORG, MAXKROG), KRN_GO: (6, vertical_krn, KRGR, MAXKRG)}


def sat_curve(S, kind, Sv, scaled, cfg, u, s, num):
    """sat_curve of assemble.hip: one relative-permeability curve of region S (samples) at the Dual saturation Sv"""
    x, y = S[_XY[kind][0]], S[_XY[kind][1]]
    if not scaled:
        return pwlin_d(x, y, Sv, num)
    ut, st = eps_triples(u)[_TRI[kind]], eps_triples(s)[_TRI[kind]]
    k = pwlin_d(x, y, to_unscaled(cfg, Sv, ut, st, num), num)
    shift, vert, fd, fmx = _VERT[kind]
    return vert((cfg >> shift) & 3, Sv, k, st, u[fd], u[fmx], s[fd], s[fmx], num)


def _blend(Sg, Sw, Sw_ow, SwcoS, kro_ow, kro_go, num):
    eps = 1e-5
    d = Sw_ow - K(SwcoS, num)
    plain = lambda: (Sg * kro_go + (Sw - K(SwcoS, num)) * kro_ow) / d
    if Sw_ow.f - SwcoS < eps:
        kro2 = (kro_ow + kro_go) / K(2.0, num)
        if Sw_ow.f - SwcoS > eps / 2.0:
            alpha = (K(eps, num) - d) / K(eps / 2.0, num)
            return kro2 * alpha + plain() * (K(1.0, num) - alpha)
        return kro2
    return plain()


def rel_perms(S, cfg, u, s, sw, sg, num, hyst=None):
    """rel_perms_eps (hyst None; cfg None: the plain functions) / rel_perms_hyst (hyst = dict(Si, uI, sI, model, h = the four stored
    doubles, scaled)) -> (krw, kro, krg) as Duals"""
    scaled = cfg is not None
    cfg = cfg or 0
    swco = S["swco"]
    SwcoS = s[SWL] if (scaled and cfg & 1) else swco
    Sw_in, Sg = K(sw, num), K(sg, num)
    SoP = K((1.0 - SwcoS) - sg, num)
    Sw = K(SwcoS, num) if SwcoS > sw else Sw_in
    Sw_ow = K(sg + Sw.f, num)
    So_go = K(1.0 - Sw_ow.f, num)
    if hyst is None:
        cur = lambda kind, Sv: sat_curve(S, kind, Sv, scaled, cfg, u, s, num)
        krw, krg, kro_ow, kro_go = cur(KRW_OW, Sw_in), cur(KRN_GO, SoP), cur(KRN_OW, Sw_ow), cur(KRW_GO, So_go)
    else:
        Si, uI, sI = hyst["Si"], hyst["uI"], hyst["sI"]
        mdcOw, dOw, mdcGo, dGo = hyst["h"]
        dr = lambda kind, Sv: sat_curve(S, kind, Sv, scaled, cfg, u, s, num)
        im = lambda kind, Sv: sat_curve(Si, kind, Sv, scaled, cfg, uI, sI, num)
        wet = im if hyst["model"] == 1 else dr
        krw = wet(KRW_OW, Sw_in)
        krg = dr(KRN_GO, SoP) if SoP.f <= mdcGo else im(KRN_GO, K(SoP.f + dGo, num))
        kro_ow = dr(KRN_OW, Sw_ow) if Sw_ow.f <= mdcOw else im(KRN_OW, K(Sw_ow.f + dOw, num))
        kro_go = wet(KRW_GO, So_go)
    return krw, _blend(Sg, Sw, Sw_ow, SwcoS, kro_ow, kro_go, num), krg


def cap_pressures(S, cfg, u, s, sw, sg, num):
    """cap_pressures_eps (cfg None: the plain functions) -> (pcow, pcgo) as Duals"""
    if cfg is None:
        return pwlin_d(S["sw"], S["pcow"], K(sw, num), num), pwlin_d(S["so"], S["pcgo"], K((1.0 - S["swco"]) - sg, num), num)
    Sw, SoP = K(sw, num), K((1.0 - s[SWL]) - sg, num)
    if cfg & 1:
        tu, tsc = eps_triples(u), eps_triples(s)
        swU, soU = two_point(Sw, tu["pc_ow"], tsc["pc_ow"], num), two_point(SoP, tu["pc_go"], tsc["pc_go"], num)
    else:
        swU, soU = Sw, K((1.0 - S["swco"]) - sg, num)
    pcw, pcg = pwlin_d(S["sw"], S["pcow"], swU, num), pwlin_d(S["so"], S["pcgo"], soU, num)
    if cfg & 256 and s[MAXPCOW] != u[MAXPCOW]:
        pcw = pcw * (K(s[MAXPCOW], num) / K(u[MAXPCOW], num))
    if cfg & 512 and s[MAXPCGO] != u[MAXPCGO]:
        pcg = pcg * (K(s[MAXPCGO], num) / K(u[MAXPCGO], num))
    return pcw, pcg


def pwlin_inv(x, y, yv, num):
    """PwLin::inv / pwlin_inv of assemble.hip at the Dual value yv -> Dual abscissa"""
    n = len(x)
    if y[0] > y[n - 1]:
        if yv.f >= y[0]:
            return K(x[0], num)
        if yv.f <= y[n - 1]:
            return K(x[n - 1], num)
        keep = lambda mid: y[mid] >= yv.f
    else:
        if yv.f <= y[0]:
            return K(x[0], num)
        if yv.f >= y[n - 1]:
            return K(x[n - 1], num)
        keep = lambda mid: y[mid] <= yv.f
    lo, hi = 0, n - 1
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        if keep(mid):
            lo = mid
        else:
            hi = mid
    m = (K(x[lo + 1], num) - K(x[lo], num)) / (K(y[lo + 1], num) - K(y[lo], num))
    return K(x[lo], num) + (yv - K(y[lo], num)) * m


def sat_curve_inv(S, kind, k, scaled, cfg, u, s, num):
    x, y = S[_XY[kind][0]], S[_XY[kind][1]]
    Su = pwlin_inv(x, y, k, num)
    if not scaled or not cfg & 1:
        return Su
    ut, st = eps_triples(u)[_TRI[kind]], eps_triples(s)[_TRI[kind]]
    Kn = lambda v: K(v, num)
    if cfg & 2:
        if Su.f <= ut[0]:
            return Kn(st[0])
        if Su.f < ut[1]:
            return Kn(st[0]) + (Su - Kn(ut[0])) * ((Kn(st[1]) - Kn(st[0])) / (Kn(ut[1]) - Kn(ut[0])))
        if Su.f < ut[2]:
            return Kn(st[1]) + (Su - Kn(ut[1])) * ((Kn(st[2]) - Kn(st[1])) / (Kn(ut[2]) - Kn(ut[1])))
        return Kn(st[2])
    return Kn(st[0]) + (Su - Kn(ut[0])) * ((Kn(st[2]) - Kn(st[0])) / (Kn(ut[2]) - Kn(ut[0])))


def hyst_see(S, Si, sOw, sGo, mdc, scaled, cfg, u, s, uI, sI, num):
    """k_hyst_update's two systems from the stored Duals mdc = [mdcOw, dOw, mdcGo, dGo] (2, 0, 2, 0: nothing seen) -> the four Duals
    after seeing the wetting saturations sOw, sGo (doubles), and (moved_ow, moved_go)"""
    out, moved = list(mdc), [False, False]
    for q, (kind, sv) in enumerate(((KRN_OW, sOw), (KRN_GO, sGo))):
        if sv < mdc[2 * q].f:
            moved[q] = True
            Sv = K(sv, num)
            k = sat_curve(S, kind, Sv, scaled, cfg or 0, u, s, num)
            out[2 * q], out[2 * q + 1] = Sv, sat_curve_inv(Si, kind, k, scaled, cfg or 0, uI, sI, num) - Sv
    return out, moved


# ---- the fluids ---------------------------------------------------------------------------------------------------------------------
def _fluid(pkg, regions):
    base = pkg.fluid.spe1_fluid()[0]
    return pkg.fluid.Fluid(base.pvt, regions, rock_pref=base.rock_pref, rock_cr=base.rock_cr, pc_scaling=True)


def corey_pair(pkg):
    """the Corey pair of tests/test_gpu_hysteresis.py::test_with_end_point_scaling_bitwise"""
    from test_oracle_endscale import corey_fluid
    d = corey_fluid(pkg).sat[0]
    swof, sgof = np.array(d["swof"]), np.array(d["sgof"])
    swi, sgi = swof.copy(), sgof.copy()
    sgi[:, 1] = (np.maximum(sgof[:, 0] - 0.15, 0.0) / 0.7) ** 1.5 * 0.8
    swi[:, 2] = np.where(swof[:, 0] >= 0.7, 0.0, ((0.7 - swof[:, 0]) / 0.55) ** 2 * 0.9)
    swi[:, 1] = swof[:, 1] * 0.85
    sgi[:, 2] = sgof[:, 2] * 0.9
    return _fluid(pkg, [d, dict(swof=swi.tolist(), sgof=sgi.tolist())])


_PSW = [0.125, 0.1875, 0.25, 0.375, 0.5, 0.625, 0.75, 0.8125, 0.875, 1.0]
_PSG = [0.0, 0.0625, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.8125, 0.875]
_PCOW = [40000.0, 30000.0, 24000.0, 16000.0, 10000.0, 6000.0, 3000.0, 2000.0, 1000.0, 0.0]
_PCGO = [0.0, 500.0, 1000.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0, 18000.0, 20000.0]


def _region(krw, krow, krg, krog):
    return dict(swof=[list(r) for r in zip(_PSW, krw, krow, _PCOW)], sgof=[list(r) for r in zip(_PSG, krg, krog, _PCGO)])


def plateau_fluid(pkg):
    """region 0 (drainage) and 1 (imbibition): krow and krg with an interior run of equal samples, a run of their maximum at one end
    and three or four zeros at the other; the imbibition curves are the drainage curves moved by a node, so that a drainage value
    on a node is an imbibition sample to the bit.  Region 2: imbibition curves whose krow and krg INCREASE with the wetting
    saturation (pwlin_inv's other form), with a run of equal samples.  Region 3: krow and krg zero everywhere."""
    krw = [0.0, 0.0, 0.0, 0.05, 0.1, 0.2, 0.35, 0.45, 0.55, 0.7]
    krog = [0.8, 0.7, 0.5, 0.3, 0.15, 0.05, 0.0, 0.0, 0.0, 0.0]
    d = _region(krw, [0.8, 0.8, 0.6, 0.4, 0.4, 0.4, 0.2, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.1, 0.3, 0.3, 0.3, 0.6, 0.9, 0.9], krog)
    kwi, kogi = [0.85 * v for v in krw], [0.9 * v for v in krog]
    i = _region(kwi, [0.8, 0.8, 0.6, 0.4, 0.4, 0.2, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, 0.6, 0.9, 0.9], kogi)
    inc = _region(kwi, [0.1, 0.1, 0.2, 0.4, 0.4, 0.4, 0.6, 0.7, 0.8, 0.8], [0.9, 0.9, 0.6, 0.3, 0.3, 0.3, 0.2, 0.1, 0.1, 0.1], kogi)
    zero = _region(kwi, [0.0] * 10, [0.0] * 10, kogi)
    return _fluid(pkg, [d, i, inc, zero])


def degenerate_fluid(pkg):
    """region 0: every phase mobile between the first and the last row - SWCR = SWL, SGCR = SGL, SOWCR = 1 - SWU - SGL, SOGCR =
    1 - SGU - SWL: in every relative-permeability triple two unscaled points coincide (u1 == u2 for krw in both systems, u0 == u1
    for krow and krg) and the table's value at the displacing phase's critical saturation IS its maximum (fmax > fdisp false: the
    fallback linear in S, and the constant where sr == sm).  Region 1, a piston: water moves only where the oil is gone, gas only
    where the oil of the gas-oil system is gone: SWCR + SGL == 1 - SOWCR to the bit, and the gas-oil twin (u1 == u2 for krow and
    krg) - and KRWR = KRORW = KRGR = KRORG = 0, so mode 2 on any curve must be refused."""
    sw = [0.125, 0.25, 0.5, 0.75, 1.0]
    sg = [0.0, 0.125, 0.375, 0.625, 0.875]
    pcw, pcg = [30000.0, 20000.0, 10000.0, 4000.0, 0.0], [0.0, 2000.0, 6000.0, 12000.0, 20000.0]
    r0 = dict(swof=[list(r) for r in zip(sw, [0.0, 0.1, 0.3, 0.5, 0.75], [0.8, 0.5, 0.25, 0.0625, 0.0], pcw)],
              sgof=[list(r) for r in zip(sg, [0.0, 0.125, 0.375, 0.625, 0.875], [0.8, 0.4, 0.2, 0.05, 0.0], pcg)])
    r1 = dict(swof=[list(r) for r in zip(sw, [0.0, 0.0, 0.0, 0.4, 0.75], [0.8, 0.4, 0.0, 0.0, 0.0], pcw)],
              sgof=[list(r) for r in zip(sg, [0.0, 0.0, 0.0, 0.5, 0.875], [0.8, 0.4, 0.0, 0.0, 0.0], pcg)])
    return _fluid(pkg, [r0, r1])


def sat_fluids(pkg):
    """name -> (fluid, drainage region, imbibition region, the configurations of CONFIGS it takes)"""
    deg = degenerate_fluid(pkg)
    no_mode2 = [k for k, v in CONFIGS.items() if 2 not in (v["krw"], v["kro"], v["krg"])]
    return {"corey": (corey_pair(pkg), 0, 1, list(CONFIGS)), "plateau": (plateau_fluid(pkg), 0, 1, list(CONFIGS)),
            "degenerate": (deg, 0, 1, list(CONFIGS)), "piston": (deg, 1, 1, no_mode2)}


# ---- the states of end-point scaling -------------------------------------------------------------------------------------------------
def _step(v, k):
    for _ in range(abs(k)):
        v = above(v) if k > 0 else below(v)
    return v


def _sw_for_sum(sg, t):
    """a double sw with sg + sw == t"""
    for k in (0, 1, -1, 2, -2, 3, -3):
        c = _step(t - sg, k)
        if sg + c == t:
            return c
    return None


def _split(x, SwcoS):
    """(sw, sg) with sg + max(SwcoS, sw) == x as the code forms it; None if no pair of doubles does"""
    if x - SwcoS >= 0.0625:
        sw = _sw_for_sum(0.03125, x)
        return None if sw is None else (sw, 0.03125)
    for k in (0, 1, -1, 2, -2):
        sg = _step(x - SwcoS, k)
        if sg + SwcoS == x:
            return SwcoS, sg
    return None


def _state_for(kind, v, SwcoS):
    """(sw, sg) at which the double the code compares for a curve of this kind - Sw itself ("krw_ow", "pc_ow"), 1 - SwcoS - Sg
    ("krn_go", "pc_go"), Sg + max(SwcoS, Sw) ("krn_ow"), 1 - that ("krw_go") - is v; None if no state does"""
    if kind in ("krw_ow", "pc_ow"):
        return v, (0.03125 if v < 0.9 else 0.0)
    if kind in ("krn_go", "pc_go"):
        sg = _sg_for(SwcoS, v)
        return None if sg is None else (SwcoS + 0.0625, sg)
    if kind == "krn_ow":
        return _split(v, SwcoS)
    x = _sg_for(0.0, v)
    return None if x is None else _split(x, SwcoS)


def _about(kind, v, SwcoS):
    """the states whose compared double is v ("0") and its neighbours: "-" / "+" where a state gives the double next to v, else "~-" /
    "~+", the nearest double on that side a state can give (1 - x moves in steps of ulp(x): one ulp of a small v is out of reach)"""
    out = []
    free = {"krn_go": lambda g: (1.0 - SwcoS) - g, "pc_go": lambda g: (1.0 - SwcoS) - g, "krw_go": lambda x: 1.0 - x}.get(kind, lambda x: x)
    for suf, side in (("-", -1), ("0", 0), ("+", 1)):
        want = v if side == 0 else below(v) if side < 0 else above(v)
        st = _state_for(kind, want, SwcoS)
        if st is None and side:
            best = None
            for k in range(-6, 7):
                val = free(_step(free(v), k))
                if (val < v if side < 0 else val > v) and (best is None or abs(val - v) < abs(best - v)) and _state_for(kind, val, SwcoS) is not None:
                    best = val
            if best is not None:
                st, suf = _state_for(kind, best, SwcoS), "~" + suf
        if st is not None:
            out.append((suf, st))
    return out


def _image(cfg, kind, S, u, s):
    """the unscaled saturation (double) the code looks the curve up at"""
    ut, st = eps_triples(u)[kind], eps_triples(s)[kind]
    Sv = K(S, float)
    if kind.startswith("pc"):
        return two_point(Sv, ut, st, float).f if cfg & 1 else S
    return to_unscaled(cfg, Sv, ut, st, float).f


def _preimages(cfg, kind, node, u, s):
    """scaled saturations about the one whose unscaled image is `node`: [("0", S)] with its neighbours "-" and "+" where a double
    hits the node, else [("~-", the last S whose image is below), ("~+", the first above)]; [] where the map does not reach it"""
    ut, st = eps_triples(u)[kind], eps_triples(s)[kind]
    three = bool(cfg & 2) and not kind.startswith("pc")
    if not cfg & 1:
        return triple(node)
    if three:
        if not ut[0] < node <= ut[2]:
            return []
        a, b = (0, 1) if node <= ut[1] else (1, 2)
    else:
        a, b = 0, 2
    if ut[b] == ut[a] or st[b] == st[a]:
        return []
    guess = st[a] + (node - ut[a]) * (st[b] - st[a]) / (ut[b] - ut[a])
    if not -0.05 < guess < 1.05:
        return []
    cand = [_step(guess, k) for k in range(-8, 9)]
    img = [_image(cfg, kind, c, u, s) for c in cand]
    hit = [c for c, v in zip(cand, img) if v == node]
    if hit:
        h = hit[len(hit) // 2]
        return [("-", below(h)), ("0", h), ("+", above(h))]
    lo, hi = [c for c, v in zip(cand, img) if v < node], [c for c, v in zip(cand, img) if v > node]
    return ([("~-", max(lo))] if lo else []) + ([("~+", min(hi))] if hi else [])


def states(fluid, region, es, pad_to=None):
    """-> dict(rows (N, 6), labels [N], sets (N,) the index into point_sets of every row, pts (N, 18) its scaled end points)"""
    S = tables(fluid)["sat"][region]
    u = table_end_points(S)
    sets = point_sets(u)
    cfg = cfg_of(es)
    R = _Rows(0, region)
    which = []

    def add(label, st, k):
        if st is None:
            return
        R.add(label, st[0], P_STATE, st[1], SW_PO_SG)
        which.append(k)
    for k, s in enumerate(sets):
        SwcoS = s[SWL] if cfg & 1 else S["swco"]
        tr = eps_triples(s)
        for kind in CURVES:
            for i in (0, 1, 2):
                if kind.startswith("pc") and i == 1:
                    continue
                for suf, st_ in _about(kind, tr[kind][i], SwcoS):
                    add("pt:%s:s%d%s" % (kind, i, suf), st_, k)
        for suf, v in triple(SwcoS):
            add("blend:swco%s" % suf, (v, 0.0), k)
            add("blend:swco%s" % suf, (v, 0.03125), k)
        for tname, target in (("eps", 1e-5), ("half_eps", 0.5e-5)):
            for suf, x in _diff_neighbours(SwcoS, target).items():
                add("blend:%s%s" % (tname, suf), (x, 0.0), k)
                add("blend:%s%s" % (tname, suf), _split(x, SwcoS) if x - SwcoS < 0.0625 else None, k)
        if k == 0:      # every table node through the scaling (the generic set)
            for kind in CURVES:
                nodes = S["sw"] if kind.endswith("_ow") else S["so"]
                for j, node in enumerate(nodes):
                    for suf, v in _preimages(cfg, kind, node, u, s):
                        add("node:%s:%s%s" % (kind, ts._position(j, len(nodes)), suf), _state_for(kind, v, SwcoS), k)
    n = len(R.rows)
    target = pad_to or (n if n > 256 and n % 256 else n + 1 if n > 256 else 300)
    q = 0
    while len(R.rows) < target:     # generic rows
        add("generic", (0.2 + 0.6 * ((q * 37) % 101) / 101.0, 0.15 * ((q * 53) % 97) / 97.0), q % len(sets))
        q += 1
    rows = np.array(R.rows, np.float64).reshape(-1, 6)
    which = np.array(which, np.int64)
    return dict(rows=rows, labels=list(R.labels), sets=which, pts=np.array(sets)[which], u=u, region=region)


def kind_of(label):
    """the kind of edge a label stands for: the label without the side of the edge"""
    if label.split(":")[0] in ("pt", "node", "blend", "scan"):
        for suf in ("~-", "~+", "-", "0", "+"):
            if label.endswith(suf):
                return label[:-len(suf)]
    return label


KINDS = (["pt:%s:s%d" % (c, i) for c in CURVES for i in (0, 1, 2) if not (c.startswith("pc") and i == 1)]
         + ["blend:swco", "blend:eps", "blend:half_eps"] + ["node:%s:interior" % c for c in CURVES])


def census(labels):
    """rows per kind of edge (kind_of), and per label"""
    kinds, full = {}, {}
    for l in labels:
        kinds[kind_of(l)] = kinds.get(kind_of(l), 0) + 1
        full[l] = full.get(l, 0) + 1
    return kinds, full


# ---- the states of hysteresis --------------------------------------------------------------------------------------------------------
HYST_CONFIGS = {"none": None, "own": config(three=0, krw=1, kro=1, krg=1), "scaled": config(three=1, krw=2, kro=2, krg=2)}


def _classify(y, yv):
    form = "dec" if y[0] > y[-1] else "flat" if y[0] == y[-1] else "inc"
    lo, hi = min(y[0], y[-1]), max(y[0], y[-1])
    if yv <= lo:
        where = "zero" if yv == 0.0 else "low"
    elif yv >= hi:
        where = "max"
    else:
        n = sum(1 for v in y[1:-1] if v == yv)
        where = "plateau" if n >= 2 else "on_node" if n == 1 else "between"
    return "%s:%s" % (form, where)


def hyst_states(fluid, drain, es, imb_scaled, imb_regions, pad_to=None):
    """rows whose turning points, handed in through set_hysteresis_params, put rel_perms_hyst, k_hyst_update and pwlin_inv on their
    edges.  imb_regions: the imbibition regions to take turns over in the inversion rows (the first one everywhere else).
    -> dict(rows, labels, mdc_ow, mdc_go (N,) handed in, imbnum (N,), pts, pts_imb (N, 18) or None, move_ow, move_go (N,) bool: what
    one begin_time_step must do, from the doubles k_hyst_update compares)"""
    T = tables(fluid)["sat"]
    S = T[drain]
    u = table_end_points(S)
    scaled = es is not None
    cfg = cfg_of(es) if scaled else 0
    s = point_sets(u)[0]
    SwcoS = s[SWL] if scaled and cfg & 1 else S["swco"]
    R = _Rows(0, drain)
    ow, go, imb = [], [], []

    def add(label, sw, sg, mdc_ow, mdc_go, region=None):
        R.add(label, sw, P_STATE, sg, SW_PO_SG)
        ow.append(float(mdc_ow))
        go.append(float(mdc_go))
        imb.append(imb_regions[0] if region is None else region)
    seen = lambda sw, sg: (sg + max(SwcoS, sw), (1.0 - SwcoS) - sg, 1.0 - ((1.0 - sw) - sg), 1.0 - min(1.0, max(0.0, sg)))
    bases = [(0.3, 0.1), (0.45, 0.2), (0.25, 0.03125), (0.6, 0.05), (0.35, 0.3), (0.5, 0.15), (0.7, 0.1), (0.28, 0.22)]
    for sw, sg in bases:
        Sw_ow, SoP, sOw, sGo = seen(sw, sg)
        for suf, v in triple(Sw_ow):        # rel_perms_hyst: Sw_ow <= mdcOw
            add("scan:ow%s" % suf, sw, sg, v, 0.95)
        for suf, v in triple(SoP):          # SoP <= mdcGo
            add("scan:go%s" % suf, sw, sg, 0.9, v)
        # k_hyst_update: the saturation seen against the stored turning point - "below" = one ulp below it (moves)
        for name, v in (("below", above(sOw)), ("equal", sOw), ("above", below(sOw))):
            add("upd:ow:%s" % name, sw, sg, v, 0.95)
        for name, v in (("below", above(sGo)), ("equal", sGo), ("above", below(sGo))):
            add("upd:go:%s" % name, sw, sg, 0.9, v)
    for q in range(4):                      # the clamp of Sg to [0, 1]: the gas-oil system sees 1 and 0
        add("clamp:sg_negative:equal", 0.3 + 0.05 * q, -0.02 * (q + 1), 0.9, 1.0)
        add("clamp:sg_negative:below", 0.3 + 0.05 * q, -0.02 * (q + 1), 0.9, above(1.0))
        add("clamp:sg_above_one:equal", 0.05 * q, 1.0 + 0.01 * (q + 1), 0.9, 0.0)
        add("clamp:sg_above_one:below", 0.05 * q, 1.0 + 0.01 * (q + 1), 0.9, 0.5)
    # the inputs of pwlin_inv: turning points on the images of the drainage nodes (the drainage value is then a sample, where the
    # map hits the node), between them, and beyond both ends
    pts_i = {r: (imb_point_set(table_end_points(T[r])) if imb_scaled else table_end_points(T[r])) for r in imb_regions}
    for kind, sys_ in ((KRN_OW, "ow"), (KRN_GO, "go")):
        name = _TRI[kind]
        nodes = S["sw"] if sys_ == "ow" else S["so"]
        cand = []
        for j, node in enumerate(nodes):
            pre = dict(_preimages(cfg, name, node, u, s)) if scaled else {"0": node}
            cand += [pre[k] for k in ("0", "~-", "~+") if k in pre]
            if j + 1 < len(nodes):
                cand.append(0.5 * (node + nodes[j + 1]))
        cand += [-0.01, 0.01, 0.99, 1.01]
        for r in imb_regions:
            uI, sI = table_end_points(T[r]), pts_i[r]
            for q, v in enumerate(cand):
                if not -0.1 < v < 1.1:
                    continue
                k = sat_curve(S, kind, K(v, float), scaled, cfg, u, s, float).f
                label = "inv:%s:%s" % (sys_, _classify(T[r][_XY[kind][1]], k))
                sw, sg = bases[q % len(bases)]
                add(label, sw, sg, v if sys_ == "ow" else 0.97, v if sys_ == "go" else 0.97, r)
    n = len(R.rows)
    target = pad_to or (n if n > 256 and n % 256 else n + 1 if n > 256 else 300)
    q = 0
    while len(R.rows) < target:
        sw, sg = bases[q % len(bases)]
        add("generic", sw + 0.001 * q, sg, 0.4 + 0.005 * q, 0.6 + 0.003 * q)
        q += 1
    rows = np.array(R.rows, np.float64).reshape(-1, 6)
    N = len(rows)
    imb = np.array(imb, np.int32)
    ow, go = np.array(ow), np.array(go)
    sOw = 1.0 - ((1.0 - rows[:, 0]) - rows[:, 2])
    sGo = 1.0 - np.minimum(1.0, np.maximum(0.0, rows[:, 2]))
    return dict(rows=rows, labels=list(R.labels), mdc_ow=ow, mdc_go=go, imbnum=imb, pts=np.array([s] * N) if scaled else None,
                pts_imb=np.array([pts_i[r] for r in imb]) if (scaled and imb_scaled) else None, u=u, region=drain, sOw=sOw, sGo=sGo,
                move_ow=sOw < ow, move_go=sGo < go)


HYST_KINDS = (["scan:ow", "scan:go"] + ["upd:%s:%s" % (a, b) for a in ("ow", "go") for b in ("below", "equal", "above")]
              + ["clamp:sg_negative:equal", "clamp:sg_negative:below", "clamp:sg_above_one:equal", "clamp:sg_above_one:below"]
              + ["inv:ow:dec:between", "inv:go:dec:between"])
# without scaling the drainage curve reaches the imbibition curve's ends: its zero (inverted to the LAST node) and its maximum.  Under
# scaling it need not: the scaled drainage maximum may lie under the imbibition one, and the three-point map sends every S beyond
# its last point ONTO the table node where the curve ends, which pwlin reads with the segment on its left - 4.5e-18 for the Corey
# krow, not 0.  (The Corey pair's drainage krg stays one ulp under the imbibition maximum: no "max" in its gas-oil system.)
HYST_KINDS_UNSCALED = ["inv:ow:dec:zero", "inv:ow:dec:max", "inv:go:dec:zero"]
HYST_KINDS_GO_MAX = ["inv:go:dec:max"]
# a drainage value that is an imbibition sample to the bit, on a node and on a plateau, and the other forms of pwlin_inv: where the
# tables offer them (the plateau fluid; the scaling's arithmetic leaves a node's sample only where the map hits the node)
HYST_KINDS_PLATEAU = ["inv:%s:dec:%s" % (a, b) for a in ("ow", "go") for b in ("on_node", "plateau")] + \
                     ["inv:%s:inc:%s" % (a, b) for a in ("ow", "go") for b in ("low", "max", "between", "on_node", "plateau")]
HYST_KINDS_FLAT = ["inv:%s:flat:%s" % (a, b) for a in ("ow", "go") for b in ("zero", "max")]


# ---- the exact statement -------------------------------------------------------------------------------------------------------------
def exact_sat(fluid, st, es, hyst=None, num=Fr):
    """st: states() or hyst_states(); es: the configuration (None: no end-point scaling); hyst: dict(model = kr_model) for
    hyst_states, the turning points of st handed in from "nothing seen".
    -> dict(sat (N, 5) krw, kro, krg, pcow, pcgo; iq (N, 6) 1/B and mobilities of the cache; mu; hyst (N, 4) the exact (turning
    point, shift) of both systems and hyst_f (N, 4) the doubles of the same statement - only with hyst)"""
    T = tables(fluid)
    rows = st["rows"]
    N = len(rows)
    scaled = es is not None
    cfg = cfg_of(es) if scaled else None
    u = st["u"]
    H = Hf = None
    per_cell = {}
    if hyst is not None:
        H, Hf = np.empty((N, 4), object), np.empty((N, 4))
        for c in range(N):
            Si = T["sat"][int(st["imbnum"][c])]
            uI = table_end_points(Si)
            sI = list(st["pts_imb"][c]) if st["pts_imb"] is not None else uI
            s = list(st["pts"][c]) if scaled else None
            per_cell[c] = (Si, uI, sI)
            for nm, dst in ((num, H), (float, None)):
                start = [K(2.0, nm), K(0.0, nm), K(2.0, nm), K(0.0, nm)]
                got, _ = hyst_see(T["sat"][st["region"]], Si, float(st["mdc_ow"][c]), float(st["mdc_go"][c]), start, scaled, cfg, u, s, uI, sI, nm)
                if dst is None:
                    Hf[c] = [g.f for g in got]
                else:
                    H[c] = [g.n for g in got]

    def law(c, S, sw, sg, nm):
        s = list(st["pts"][c]) if scaled else None
        hy = None
        if hyst is not None:
            Si, uI, sI = per_cell[c]
            hy = dict(Si=Si, uI=uI, sI=sI, model=hyst["model"], h=[float(v) for v in Hf[c]])
        kr = rel_perms(S, cfg, u, s, sw, sg, nm, hy)
        pc = cap_pressures(S, cfg, u, s, sw, sg, nm)
        return tuple(v.n for v in kr) + tuple(v.n for v in pc)
    P, Sx, Q, MU = ts.exact(fluid, rows, None, num, T, sat_law=law)
    return dict(sat=Sx, iq=Q, mu=MU, hyst=H, hyst_f=Hf)


def scales(fluid, st, imb=False):
    """per column of exact_sat's sat and iq arrays, the largest magnitude the quantity is interpolated or scaled from: the table's
    samples and the scaled end values of every point set in use (the imbibition tables' and points' too under hysteresis)"""
    T = tables(fluid)
    _, sat, iq = ts.scales(fluid, 0, st["region"], T)
    sat, iq = list(sat), list(iq)
    ends = [np.asarray(st["pts"])] if st.get("pts") is not None else []
    if imb:
        for r in sorted(set(int(v) for v in st["imbnum"])):
            other = ts.scales(fluid, 0, r, T)[1]
            sat = [max(a, b) for a, b in zip(sat, other)]
        if st.get("pts_imb") is not None:
            ends.append(np.asarray(st["pts_imb"]))
    for e in ends:
        mx = np.abs(e).max(axis=0)
        sat[0] = max(sat[0], mx[MAXKRW]); sat[1] = max(sat[1], mx[MAXKROW], mx[MAXKROG]); sat[2] = max(sat[2], mx[MAXKRG])
        sat[3] = max(sat[3], mx[MAXPCOW]); sat[4] = max(sat[4], mx[MAXPCGO])
    return sat, list(iq[:3]) + sat[:3]


def distances(fluid, st, ex, sat_probe, iq, hyst=None):
    """[(distance, (row, column))] of the saturation functions (None to skip), the cache and - under hysteresis - the (turning
    point, shift) arrays (a 4-tuple of (N,) arrays, scale 1) to the exact statement"""
    sat_sc, iq_sc = scales(fluid, st, imb=ex["hyst"] is not None)
    out = []
    if sat_probe is not None:
        out.append(relative_distance(sat_probe, ex["sat"], sat_sc))
    out.append(relative_distance(ts.cache_values(iq), ex["iq"], iq_sc, ex["mu"]))
    if hyst is not None:
        out.append(relative_distance(np.stack(hyst, axis=1), ex["hyst"], [1.0] * 4))
    return out


def sat_probe_by_set(probe, st, es, region):
    """the saturation functions of every row with ITS point set: `probe` (capi.HipFluid / oracle_bind.OracleFluid) takes one set a
    call"""
    import importlib
    fields = importlib.import_module("opm-autodiff_amd").capi.EPS_FIELDS
    rows = st["rows"]
    out = np.empty((len(rows), 5))
    for k in sorted(set(st["sets"].tolist())):
        sel = np.flatnonzero(st["sets"] == k)
        d = dict(es)
        d.update({name: float(st["pts"][sel[0], f]) for f, name in enumerate(fields)})
        out[sel] = probe.sat_probe(rows[sel, 0], rows[sel, 2], d, sat_region=region)
    return out


def end_value_checks(fluid, st, es, sat):
    """on a scaled end point the curve takes its end value.  To the bit where nothing rounds: the first point of a map is hit
    without rounding (S - s0 = 0), so a zero there is a zero and, without vertical scaling, the table's sample comes back as it is.
    Elsewhere the map's last product may leave the table's end point by an ulp of 1 and the vertical scaling rounds twice more:
    within (steepest slope of the curve) x 2 ulp(1) + 4 ulp(end value).  `sat`: (N, 5) from any source.
    -> (comparisons made, of those to the bit, mismatches)"""
    cfg = cfg_of(es)
    S = tables(fluid)["sat"][st["region"]]
    u = st["u"]
    n, nbit, wrong = 0, 0, []
    slope = lambda x, y: max(abs((y[j + 1] - y[j]) / (x[j + 1] - x[j])) for j in range(len(x) - 1))
    for c, l in enumerate(st["labels"]):
        if not l.startswith("pt:") or not l.endswith("0") or not cfg & 1:
            continue
        s = st["pts"][c]
        kind, i = l.split(":")[1], int(l.split(":")[2][1])
        three = bool(cfg & 2)
        want = None
        if kind == "krw_ow":
            col, mode, sl = 0, (cfg >> 2) & 3, slope(S["sw"], S["krw"])
            want = 0.0 if i == 0 else (s[MAXKRW] if mode else u[MAXKRW]) if i == 2 else s[KRWR] if (mode == 2 and three) else None
        elif kind == "krn_go":
            col, mode, sl = 2, (cfg >> 6) & 3, slope(S["so"], S["krg"])
            want = (s[MAXKRG] if mode else u[MAXKRG]) if i == 0 else 0.0 if i == 2 else s[KRGR] if (mode == 2 and three) else None
        elif kind == "pc_ow":
            col, mode, sl = 3, 1 if cfg & 256 else 0, slope(S["sw"], S["pcow"])
            want = (s[MAXPCOW] if mode else u[MAXPCOW]) if i == 0 else S["pcow"][-1] * ((s[MAXPCOW] / u[MAXPCOW]) if mode else 1.0)
        elif kind == "pc_go":
            col, mode, sl = 4, 1 if cfg & 512 else 0, slope(S["so"], S["pcgo"])
            want = (s[MAXPCGO] if mode else u[MAXPCGO]) if i == 0 else S["pcgo"][-1] * ((s[MAXPCGO] / u[MAXPCGO]) if mode else 1.0)
        if want is None:
            continue
        tr = eps_triples(s)[kind]
        if (i > 0 and tr[i] == tr[i - 1]) or (i < 2 and tr[i] == tr[i + 1]):
            # two scaled points coincide: a value on them belongs to the piece on their LEFT, so the curve does not end on its
            # end value there (krw at SWU = s1 == s2 is the table's value at ITS s1, one ulp above it the maximum; in mode 2 it is
            # scaled with the lower piece's ratio) - the exact statement holds these rows, not this check
            continue
        n += 1
        got = float(sat[c, col])
        if i == 0 and (want == 0.0 or mode == 0):
            nbit += 1
            ok = got == want
        else:
            ok = abs(got - want) <= sl * 2.0 * np.spacing(1.0) + 4.0 * np.spacing(abs(want))
        if not ok:
            wrong.append((l, c, got, want))
    return n, nbit, wrong

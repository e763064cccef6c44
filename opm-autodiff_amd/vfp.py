"""Vertical-flow-performance tables (VFPPROD / VFPINJ): the bottom-hole pressure of a well as a function of its rates and its tubing-head
pressure, and the inverse look-up - stated on the host in an order a kernel can follow, operation by operation.  The device functions
(csrc/std_wells.hip vfp_*, opmhip_vfp_probe) are this file, bit for bit; NumPy's elementwise arithmetic is IEEE arithmetic without
contraction, so every function below takes arrays (one entry per point) as well as plain floats.

What of the reference this restates:
  wells/VFPHelpers.cpp: findInterpData (:81-145), interpolate for VFPPROD (:181-287) and VFPINJ (:289-341), bhp (:343-385), findTHP
      (:387-499) with findX (:40-66), getFlo / getWFR / getGFR (:501-590);
  wells/VFPProdProperties.cpp: thp (:37-82), the AD form of bhp (:142-172); wells/VFPInjProperties.cpp: thp (:47-74), bhp (:88-112).
Rates are (aqua, liquid, vapour) = (q_w, q_o, q_g), surface volumes per second INTO the reservoir - a producer's are negative -, which
is the reference's sign and this library's; pressures in pascal; a table's flo axis is positive.

UNVERIFIED (opm-material is not in the reference tree): how Opm::max / Opm::min differentiate an Evaluation.  Stated here: a chop
max(0, .) or a threshold max(1e-12, .) that binds - ties included - has derivative zero; one that does not bind passes its argument's
derivative through.  The VALUES follow std::max(a, b) = (a < b) ? b : a, so that a NaN or a negative zero is chopped to +0.

Where the reference leaves a result undefined, this statement defines it (the device must never read out of bounds):
  find_interp_data with a NaN value takes the last interval (the reference's loop finds nothing and leaves the indices unset);
  find_thp returns -1e100, the value it starts from, where the reference throws "Unable to find THP" or its assertion would fail.
An injector's dwfr, dgfr, dalq (the reference carries -1e100 through them) are not carried: reported as 0."""
import numpy as np

PROD, INJ = 0, 1                                   # opmhip_vfp_tables.kind
FLO_PROD = {"OIL": 0, "LIQ": 1, "GAS": 2}          # VFPProdTable::FLO_TYPE
FLO_INJ = {"OIL": 0, "WAT": 1, "GAS": 2}           # VFPInjTable::FLO_TYPE
WFR = {"WOR": 0, "WCT": 1, "WGR": 2}
GFR = {"GOR": 0, "GLR": 1, "OGR": 2}
THRESHOLD = 1e-12
NOT_FOUND = -1e100
MAX_FACTOR = 3.0


class VFPTable:
    """One table, SI.  kind PROD: axes (flo, thp, wfr, gfr, alq), values[thp][wfr][gfr][alq][flo]; kind INJ: axes (flo, thp),
    values[thp][flo].  Types by name ("LIQ", "WCT", "GOR", ...) or by the C ABI's number."""

    def __init__(self, kind, table_num, datum_depth, flo_type, axes, values, wfr_type=0, gfr_type=0):
        self.kind, self.table_num, self.datum_depth = int(kind), int(table_num), float(datum_depth)
        if self.kind not in (PROD, INJ):
            raise ValueError("VFPTable: kind 0 (VFPPROD) or 1 (VFPINJ)")
        names = FLO_PROD if self.kind == PROD else FLO_INJ
        self.flo_type = names[flo_type] if isinstance(flo_type, str) else int(flo_type)
        self.wfr_type = WFR[wfr_type] if isinstance(wfr_type, str) else int(wfr_type)
        self.gfr_type = GFR[gfr_type] if isinstance(gfr_type, str) else int(gfr_type)
        if not (0 <= self.flo_type < 3 and 0 <= self.wfr_type < 3 and 0 <= self.gfr_type < 3):
            raise ValueError("VFPTable: unknown flo / wfr / gfr type")
        axes = [np.asarray(a, float).reshape(-1) for a in axes]
        if len(axes) != (5 if self.kind == PROD else 2) or any(len(a) == 0 for a in axes):
            raise ValueError("VFPTable: %d non-empty axes" % (5 if self.kind == PROD else 2))
        for a in axes:
            if not np.all(np.isfinite(a)) or np.any(np.diff(a) < 0.0):
                raise ValueError("VFPTable: an axis decreases or is not finite")
        self.axes = axes
        self.flo_axis, self.thp_axis = axes[0], axes[1]
        shape = tuple(len(axes[i]) for i in ((1, 2, 3, 4, 0) if self.kind == PROD else (1, 0)))
        self.values = np.ascontiguousarray(np.asarray(values, float).reshape(shape))
        if not np.all(np.isfinite(self.values)):
            raise ValueError("VFPTable: a value is not finite")
        if self.kind == PROD:
            self.wfr_axis, self.gfr_axis, self.alq_axis = axes[2], axes[3], axes[4]

    @classmethod
    def from_deck_units(cls, rec, pressure, rate, length=1.0):
        """a VFPPROD record in deck units (tests/golden/vfpprod2_table.json's keys) -> SI: pressures * pressure, the flo axis * rate, the datum
        * length; the ratio axes and ALQ as written"""
        axes = [np.asarray(rec["flo_axis"], float) * rate, np.asarray(rec["thp_axis"], float) * pressure, rec["wfr_axis"], rec["gfr_axis"], rec["alq_axis"]]
        return cls(PROD, rec["table_num"], rec["datum_depth"] * length, rec["flo_type"], axes, np.asarray(rec["values"], float) * pressure,
                   wfr_type=rec["wfr_type"], gfr_type=rec["gfr_type"])


# ---- findInterpData ------------------------------------------------------------------------------------------------------------------
def find_interp_data(value, axis):
    """-> (i0, i1, inv_dist, factor), VFPHelpers.cpp:81-145.  A negative value is taken as 0; an axis of one entry gives (0, 0, 0.0, 0.0);
    below the first entry the first interval (factor may be negative), at or above the last entry the last interval, else the first i
    with axis[i] >= value closes the interval; inv_dist = 1.0 / (end - start), factor = (value - start) * inv_dist where end > start,
    both 0.0 otherwise; factor is capped at 3.0.  value: a float (-> ints and floats) or an array (-> arrays)."""
    axis = np.asarray(axis, float)
    scalar = np.ndim(value) == 0
    v = np.atleast_1d(np.asarray(value, float))
    v = np.where(v < 0.0, 0.0, v)
    n = len(axis)
    if n == 1:
        i0 = i1 = np.zeros(v.shape, np.int64)
        inv = fac = np.zeros(v.shape)
    else:
        i1 = np.minimum(np.searchsorted(axis[1:], v, side="left") + 1, n - 1)     # the first i >= 1 with axis[i] >= v (none, a NaN: the last)
        i1 = np.where(v < axis[0], 1, np.where(v >= axis[-1], n - 1, i1))
        i0 = i1 - 1
        start, end = axis[i0], axis[i1]
        wide = end > start
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = np.where(wide, 1.0 / (end - start), 0.0)
            fac = np.where(wide, (v - start) * inv, 0.0)
        fac = np.where(fac > MAX_FACTOR, MAX_FACTOR, fac)
    if scalar:
        return int(i0[0]), int(i1[0]), float(inv[0]), float(fac[0])
    return i0, i1, inv, fac


def _as_arrays(interp):
    return tuple(np.atleast_1d(np.asarray(a)) for a in interp)


def _reduce(c, factors):
    """c: (2, ..., 2, n) corner values, the LAST corner axis reduced first: (t1 * a) + (t2 * b), t2 = factor, t1 = 1.0 - t2"""
    for fac in factors:
        t2 = fac
        t1 = 1.0 - t2
        c = (t1 * c[..., 0, :]) + (t2 * c[..., 1, :])
    return c


def _both(c, k, inv):
    """the derivative along corner axis k: (hi - lo) * inv_dist per corner pair, the same at both ends"""
    d = (np.take(c, 1, axis=k) - np.take(c, 0, axis=k)) * inv
    return np.stack([d, d], axis=k)


def interpolate_prod(table, flo_i, thp_i, wfr_i, gfr_i, alq_i):
    """-> (value, dthp, dwfr, dgfr, dalq, dflo), VFPHelpers.cpp:181-287: the 32 corner values nn[t][w][g][a][f] gathered, each partial
    derivative formed per corner pair, all six fields reduced along flo, alq, gfr, wfr, thp in that order"""
    f, t, w, g, a = (_as_arrays(i) for i in (flo_i, thp_i, wfr_i, gfr_i, alq_i))
    n = max(len(i[0]) for i in (f, t, w, g, a))
    c = np.empty((2, 2, 2, 2, 2, n))
    for it in range(2):
        for iw in range(2):
            for ig in range(2):
                for ia in range(2):
                    for jf in range(2):
                        c[it, iw, ig, ia, jf] = table.values[t[it], w[iw], g[ig], a[ia], f[jf]]
    factors = (f[3], a[3], g[3], w[3], t[3])
    fields = [c] + [_both(c, k, i[2]) for k, i in ((0, t), (1, w), (2, g), (3, a), (4, f))]
    return tuple(_reduce(x, factors) for x in fields)


def interpolate_inj(table, flo_i, thp_i):
    """-> (value, dthp, dflo), VFPHelpers.cpp:289-341: four corners nn[t][f], reduced along flo, then thp"""
    f, t = _as_arrays(flo_i), _as_arrays(thp_i)
    n = max(len(f[0]), len(t[0]))
    c = np.empty((2, 2, n))
    for it in range(2):
        for jf in range(2):
            c[it, jf] = table.values[t[it], f[jf]]
    factors = (f[3], t[3])
    return tuple(_reduce(x, factors) for x in (c, _both(c, 0, t[2]), _both(c, 1, f[2])))


# ---- flo, wfr, gfr with their derivatives by (aqua, liquid, vapour) -----------------------------------------------------------------------
def _rates(*values):
    """the arguments as float arrays of one common length (one entry per point)"""
    q = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, float)) for v in values))
    return [np.array(v) for v in q]


def _unit(n, *ones, sign=1.0):
    """the derivative of a signed sum of rates by (aqua, liquid, vapour): `sign` for the rates named, 0.0 for the others"""
    d = np.zeros((3, n))
    for j in ones:
        d[j] = sign
    return d


def _chop(x, dx):
    """chopNegativeValues: max(0, x); zero derivative where it binds (x not > 0)"""
    keep = 0.0 < x
    return np.where(keep, x, 0.0), np.where(keep, dx, 0.0)


def _quotient(a, da, c, dc):
    """chop(a) / max(1e-12, chop(c)) with the quotient rule (a' - v * b') / b, v = a / b"""
    a, da = _chop(a, da)
    c, dc = _chop(c, dc)
    keep = THRESHOLD < c
    b, db = np.where(keep, c, THRESHOLD), np.where(keep, dc, 0.0)
    v = a / b
    return v, (da - v * db) / b


def flo(table, aqua, liquid, vapour):
    """-> (flo, d flo / d(aqua, liquid, vapour) as (3, n)): getFlo, the sign of the rates kept (VFPHelpers.cpp:501-543)"""
    aq, li, va = _rates(aqua, liquid, vapour)
    n = len(aq)
    if table.kind == PROD:
        return ((li, _unit(n, 1)), (aq + li, _unit(n, 0, 1)), (va, _unit(n, 2)))[table.flo_type]
    return ((li, _unit(n, 1)), (aq, _unit(n, 0)), (va, _unit(n, 2)))[table.flo_type]


def wfr(table, aqua, liquid, vapour):
    """getWFR (VFPHelpers.cpp:547-568): WOR -aqua / -liquid, WCT -aqua / (-aqua - liquid), WGR -aqua / -vapour, chopped and thresholded"""
    aq, li, va = _rates(aqua, liquid, vapour)
    n = len(aq)
    num = (-aq, _unit(n, 0, sign=-1.0))
    den = ((-li, _unit(n, 1, sign=-1.0)), (-aq - li, _unit(n, 0, 1, sign=-1.0)), (-va, _unit(n, 2, sign=-1.0)))[table.wfr_type]
    return _quotient(*num, *den)


def gfr(table, aqua, liquid, vapour):
    """getGFR (VFPHelpers.cpp:570-590): GOR -vapour / -liquid, GLR -vapour / (-liquid - aqua), OGR -liquid / -vapour"""
    aq, li, va = _rates(aqua, liquid, vapour)
    n = len(aq)
    if table.gfr_type == 0:
        return _quotient(-va, _unit(n, 2, sign=-1.0), -li, _unit(n, 1, sign=-1.0))
    if table.gfr_type == 1:
        return _quotient(-va, _unit(n, 2, sign=-1.0), -li - aq, _unit(n, 0, 1, sign=-1.0))
    return _quotient(-li, _unit(n, 1, sign=-1.0), -va, _unit(n, 2, sign=-1.0))


# ---- bhp ---------------------------------------------------------------------------------------------------------------------------
def bhp(table, aqua, liquid, vapour, thp, alq=0.0):
    """-> (n, 9): value, dthp, dwfr, dgfr, dalq, dflo (VFPHelpers.cpp:343-385; producers search with -flo, injectors with flo) and
    d bhp / d(aqua, liquid, vapour) as the AD form has it (VFPProdProperties.cpp:142-172): (dwfr * wfr') + (dgfr * gfr') - (dflo * flo');
    injectors dflo * flo' (VFPInjProperties.cpp:88-112).  alq is ignored for an injector.  Floats in: (9,) out."""
    scalar = all(np.ndim(v) == 0 for v in (aqua, liquid, vapour, thp, alq))
    aq, li, va, th, al = _rates(aqua, liquid, vapour, thp, alq)
    n = len(aq)
    out = np.zeros((n, 9))
    f, df = flo(table, aq, li, va)
    thp_i = find_interp_data(th, table.thp_axis)
    if table.kind == PROD:
        w, dw = wfr(table, aq, li, va)
        g, dg = gfr(table, aq, li, va)
        r = interpolate_prod(table, find_interp_data(-f, table.flo_axis), thp_i, find_interp_data(w, table.wfr_axis),
                             find_interp_data(g, table.gfr_axis), find_interp_data(al, table.alq_axis))
        for k in range(6):
            out[:, k] = r[k]
        for j in range(3):
            out[:, 6 + j] = ((r[2] * dw[j]) + (r[3] * dg[j])) - (r[5] * df[j])
    else:
        r = interpolate_inj(table, find_interp_data(f, table.flo_axis), thp_i)
        out[:, 0], out[:, 1], out[:, 5] = r
        for j in range(3):
            out[:, 6 + j] = r[2] * df[j]
    return out[0] if scalar else out


# ---- thp ---------------------------------------------------------------------------------------------------------------------------
def find_x(x0, x1, y0, y1, y):
    """findX (VFPHelpers.cpp:40-66): x0 + (y - y0) * (dx / dy); x1 where dy == 0"""
    dx = x1 - x0
    dy = y1 - y0
    if dy != 0.0:
        return x0 + (y - y0) * (dx / dy)
    return x1


def find_thp(bhp_array, thp_array, bhp):
    """findTHP (VFPHelpers.cpp:387-499) on plain floats; -1e100 where the reference throws.  Needs two entries at least."""
    b, t = [float(v) for v in bhp_array], [float(v) for v in thp_array]
    n = len(t)
    if n < 2 or len(b) != n:
        raise ValueError("find_thp: needs a THP axis of two entries or more, and as many BHP values")
    bhp = float(bhp)

    def line(i):
        return find_x(t[i], t[i + 1], b[i], b[i + 1], bhp)

    def inside():
        for i in range(n - 1):
            if b[i] < bhp and bhp <= b[i + 1]:
                return i
        return -1
    if all(not (b[i + 1] < b[i]) for i in range(n - 1)):       # std::is_sorted
        if bhp <= b[0]:
            return line(0)
        if bhp > b[n - 1]:
            return line(n - 2)
        i = inside()
        return line(i) if i >= 0 else NOT_FOUND
    i = inside()
    if i >= 0:
        return line(i)
    if bhp <= b[0]:
        return line(0)
    if bhp > b[n - 1]:
        return line(n - 2)
    return NOT_FOUND


def bhp_of_thp_axis(table, aqua, liquid, vapour, alq=0.0):
    """-> (nthp, n): the table's BHP at every entry of its THP axis for the given rates, as thp() forms it (VFPProdProperties.cpp:45-78,
    VFPInjProperties.cpp:55-70): a producer with all-zero rates takes the first entry of the flo axis and zero fractions"""
    aq, li, va, al = _rates(aqua, liquid, vapour, alq)
    n = len(aq)
    f, _ = flo(table, aq, li, va)
    if table.kind == PROD:
        zero = (aq == 0.0) & (li == 0.0) & (va == 0.0)
        w, _ = wfr(table, aq, li, va)
        g, _ = gfr(table, aq, li, va)
        f, w, g = np.where(zero, table.flo_axis[0], -f), np.where(zero, 0.0, w), np.where(zero, 0.0, g)
        fi, wi, gi, ai = (find_interp_data(v, ax) for v, ax in ((f, table.flo_axis), (w, table.wfr_axis), (g, table.gfr_axis), (al, table.alq_axis)))
    else:
        fi = find_interp_data(f, table.flo_axis)
    out = np.empty((len(table.thp_axis), n))
    for i, t in enumerate(table.thp_axis):
        ti = find_interp_data(np.full(n, t), table.thp_axis)
        out[i] = interpolate_prod(table, fi, ti, wi, gi, ai)[0] if table.kind == PROD else interpolate_inj(table, fi, ti)[0]
    return out


def thp(table, aqua, liquid, vapour, bhp, alq=0.0):
    """the tubing-head pressure that gives `bhp` at these rates: VFPProdProperties::thp (:37-82) / VFPInjProperties::thp (:47-74).  A table
    whose THP axis has fewer than two entries is refused (findTHP reads thp_array[1])."""
    if len(table.thp_axis) < 2:
        raise ValueError("vfp.thp: table %d has a THP axis of fewer than two entries" % table.table_num)
    scalar = all(np.ndim(v) == 0 for v in (aqua, liquid, vapour, bhp, alq))
    aq, li, va, target, al = _rates(aqua, liquid, vapour, bhp, alq)
    arr = bhp_of_thp_axis(table, aq, li, va, al)
    out = np.array([find_thp(arr[:, k], table.thp_axis, target[k]) for k in range(arr.shape[1])])
    return float(out[0]) if scalar else out


def probe(table, aqua, liquid, vapour, thp_value, alq=0.0, bhp_target=None):
    """what opmhip_vfp_probe returns, (n, 10): bhp()'s nine and thp(..., bhp_target) - 0 without a target and for a table whose THP axis has
    fewer than two entries"""
    aq, li, va, th, al, target = _rates(aqua, liquid, vapour, thp_value, alq, 0.0 if bhp_target is None else bhp_target)
    out = np.zeros((len(aq), 10))
    out[:, :9] = bhp(table, aq, li, va, th, al)
    if bhp_target is not None and len(table.thp_axis) >= 2:
        out[:, 9] = thp(table, aq, li, va, target, al)
    return out
